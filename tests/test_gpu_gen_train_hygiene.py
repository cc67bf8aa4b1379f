"""The contract on caller-owned memory (tests/buffer_hygiene_common.py as it is) for every entry of
include/i2v_hip_gen_train.h: each case runs plain, on buffers filled with 0x00 and on buffers filled with 0xFF; the guard bands around
every allocation of the binding stay intact, the three results agree bit for bit, and nothing non-finite comes back on 0xFF.  Then one
live handle across shapes A -> larger B -> A (its workspace poisoned before each step) against a fresh handle per step."""
import numpy as np
import pytest
import torch

import buffer_hygiene_common as bh
import gen_train_common as gt
import i2v_native

pytestmark = pytest.mark.gpu
DEV = "cuda"
NF, Z = 16, 8


def dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def rnd(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def _params(seed=5):
    return {"fc.weight": rnd(seed, 256 * NF, Z) * 0.3, "fc.bias": rnd(seed + 1, 256 * NF) * 0.2,
            "conv_img.weight": rnd(seed + 2, 3, NF, 3, 3, 3) * 0.05, "conv_img.bias": rnd(seed + 3, 3) * 0.2}


def _handle():
    h = i2v_native.NativeGenTrain(NF, Z, device=DEV)
    params = {k: v.to(DEV) for k, v in _params().items()}
    return i2v_native.bind_in_place(h, params), params


def _grads(params):
    """Gradient tensors from the binding's own (guarded) allocator."""
    return {k: i2v_native.torch.empty(tuple(p.shape), dtype=torch.float32, device=DEV) for k, p in params.items()}


def _step(hp, shape):
    """Every handle entry once: fc forward and backward, head forward (kept and not kept) and backward."""
    h, params = hp
    B, T, H, W = shape
    z, g_fc = dev(rnd(11, B, Z), rnd(12, B, 256 * NF))
    x, g = dev(rnd(13, B, NF, T, H, W), rnd(14, B, T, 3, H, W))
    grads = _grads(params)
    i2v_native.bind_in_place(h, params, grads)
    fc = h.fc_forward(z)
    dz = h.fc_backward(g_fc, z, need_dz=True, param_grads=True)
    y, saved = h.head_forward(x, save=True)
    y2, _ = h.head_forward(x, save=False)
    dx = h.head_backward(g, saved, tuple(x.shape), need_dx=True, param_grads=True)
    return [fc, dz, y, y2, dx, *grads.values()]


def _fc_units():
    z, w, b, g = rnd(21, 3, Z), rnd(22, 256 * NF, Z), rnd(23, 256 * NF), rnd(24, 3, 256 * NF)
    return (lambda: i2v_native.gen_train_fc_forward_unit(*dev(z, w, b))), (lambda: i2v_native.gen_train_fc_backward_unit(*dev(g, z, w)))


def _up_units(ut, us, thw):
    x = rnd(31, 2, 16, *thw)
    g = rnd(32, 2, 16, thw[0] * ut, thw[1] * us, thw[2] * us)
    return (lambda: i2v_native.gen_train_upsample(x.to(DEV), ut, us)), (lambda: i2v_native.gen_train_upsample_backward(g.to(DEV), ut, us))


def _head_units(nf, B, thw):
    x, w, b, g = rnd(41, B, nf, *thw), rnd(42, 3, nf, 3, 3, 3) * 0.05, rnd(43, 3) * 0.2, rnd(44, B, thw[0], 3, *thw[1:])
    x[0, :, 0, 0, :2] = 0.0

    def both():
        y, saved = i2v_native.gen_train_head_forward_unit(*dev(x, w, b))
        return [y, *i2v_native.gen_train_head_backward_unit(g.to(DEV), saved, w.to(DEV), tuple(x.shape))]

    def gate(outs):
        y, dx, dw, db = (o.cpu() for o in outs)
        n = 27 * nf + 4
        y64, S, _, _ = gt.head_forward_ref(x, w, b)
        r = gt.head_backward_ref(x, w, g, y)
        for name, got, ref, s, nn in (("frames", y, y64, S, n), ("dx", dx, r["dx"], r["S_dx"], n), ("dW", dw, r["dw"], r["S_dw"], n),
                                      ("db", db[None], r["db"][None], r["S_db"][None], 1)):
            ok, ratio, l2 = gt.gate(got, ref, s, nn)
            assert ok, f"float64 gate on the 0xFF run: head {name}: |err|/bound {ratio:.3f}, rel-L2 {l2:.2e}"
    return both, gate, (lambda: i2v_native.gen_train_head_forward_unit(*dev(x, w, b), save=False)[0])


CASES = []


def add(name, fn, gate=None):
    CASES.append(pytest.param(fn, gate, id=name))


_f = _fc_units()
add("fc-forward-unit", _f[0])
add("fc-backward-unit", _f[1])
for _ut, _us, _thw in ((2, 2, (1, 4, 4)), (1, 4, (3, 5, 6)), (4, 1, (3, 5, 6)), (2, 2, (2, 3, 5))):
    _u = _up_units(_ut, _us, _thw)
    add(f"upsample-{_ut}x{_us}-{'x'.join(map(str, _thw))}", _u[0])
    add(f"upsample-backward-{_ut}x{_us}-{'x'.join(map(str, _thw))}", _u[1])
for _nf, _b, _thw in ((16, 1, (1, 4, 4)), (48, 2, (3, 5, 6))):
    _h = _head_units(_nf, _b, _thw)
    add(f"head-units-nf{_nf}-{'x'.join(map(str, _thw))}", _h[0], _h[1])
    add(f"head-forward-unit-unsaved-nf{_nf}", _h[2])
add("handle-every-entry", lambda: _step(_handle(), (2, 3, 5, 6)))


@pytest.mark.parametrize("fn,gate", CASES)
def test_entry_on_poisoned_guard_banded_buffers(fn, gate, monkeypatch, request):
    stats = {}
    outs = bh.run_three(fn, i2v_native, monkeypatch, request.node.callspec.id, stats)
    assert stats["runs"] == 2 and stats["allocations"] > 0 and stats["foreign"] == 0
    if gate is not None:
        gate(outs)
    print(f"  HYGIENE {request.node.callspec.id}: {len(outs)} tensors, 3 runs agree bit for bit, guards intact; workspace / saved bytes as reported "
          f"{stats['last_uint8']}")


def test_handle_reuse_across_shapes():
    """A = 2 x (3, 5, 6), B = 3 x (4, 8, 8) (more samples, the larger map and workspace), A again."""
    live = _handle()
    for shape in ((2, 3, 5, 6), (3, 4, 8, 8), (2, 3, 5, 6)):
        if live[0]._ws.buf is not None:
            live[0]._ws.buf.fill_(0xFF)
        got = [t.clone() for t in _step(live, shape)]
        want = _step(_handle(), shape)
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert bh.same_bits(a, b), f"handle reuse across shapes: {shape}, output {i} {tuple(a.shape)} differs from a fresh handle's"
