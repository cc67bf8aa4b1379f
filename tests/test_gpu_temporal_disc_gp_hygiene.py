"""The contract on caller-owned memory (tests/buffer_hygiene_common.py as it is) for every entry of
include/i2v_hip_disc3d_gp.h: each case runs plain, on buffers filled with 0x00 and on buffers filled with 0xFF; the guard bands around
every allocation of the binding stay intact, the three results agree bit for bit, and nothing non-finite comes back on 0xFF.  Then one
live handle across clip shapes A -> larger B -> A (its workspace poisoned before each step) against a fresh handle per step."""
import pytest
import torch

import buffer_hygiene_common as bh
import i2v_native
import temporal_disc_common as tc
import temporal_disc_gp_common as gp

pytestmark = pytest.mark.gpu
DEV = "cuda"
# two clip shapes that fixture B's network takes (it ends on [1, 4, 4] from 3 or 4 frames of 32 x 32): B has more samples and frames
SHAPE_A, SHAPE_B = (2, 3, 3, 32, 32), (4, 3, 4, 32, 32)


def _handle(cfg=tc.CFG_B):
    h = i2v_native.NativeDisc3D(cfg["channels"], cfg["stride_s"], cfg["stride_t"], cfg["use_max_pool"], cfg["spectral_norm"], device=DEV)
    params = {k: v.to(DEV) for k, v in tc.synthetic_state(cfg, tc.SEED_B).items()}
    return i2v_native.bind_in_place(h, params), params


def _grads(params):
    """Gradient tensors from the binding's own (guarded) allocator."""
    return {k: i2v_native.torch.empty(tuple(p.shape), dtype=torch.float32, device=DEV) for k, p in params.items() if not k.endswith(("weight_u", "weight_v"))}


def _step(hp, shape, dev_scale=False):
    """Every handle entry once: the sizes, one saved forward (no power iteration: the handle's state stays what it was), gp_backward
    written, then accumulated onto zeros with the device scale, the layout."""
    h, params = hp
    x = tc.randn(76000 + shape[2], shape).to(DEV)
    grads = _grads(params)
    i2v_native.bind_in_place(h, params, grads)
    _, _, saved = h.forward(x, iterate=False, save=True, want_fmaps=False)
    l_gp, gsv = h.gp_backward(saved, shape, scale=gp.W_GP, accumulate=False)
    out = [l_gp.reshape(1), *grads.values()]
    if dev_scale:
        more = {k: i2v_native.torch.zeros(tuple(g.shape), dtype=torch.float32, device=DEV) for k, g in grads.items()}
        i2v_native.bind_in_place(h, params, more)
        l2, gsv = h.gp_backward(saved, shape, scale=0.5, scale_dev=torch.full((1,), 3.0, dtype=torch.float32, device=DEV), accumulate=True)
        out += [l2.reshape(1), *more.values()]
    return out + list(h.gp_saved_maps(gsv, shape).values())


def _gn_units(c):
    def both():
        x, xd, resd, act, g, gd, w, b = (t.to(DEV) if t.dim() == 1 else tc.cl(t).to(DEV) for t in gp.gn_case_inputs(c))
        _, stats = i2v_native.disc3d_groupnorm_unit(x, w, b)
        out, tstats = i2v_native.disc3d_gp_groupnorm_tangent_unit(x, xd, stats, w, resd, act)
        plain, _ = i2v_native.disc3d_gp_groupnorm_tangent_unit(x, xd, stats, w)
        return [out, tstats, plain, *i2v_native.disc3d_gp_groupnorm_dual_backward_unit(g, gd, x, xd, stats, tstats, w, mask=act)]
    return both


def _pool_unit():
    x, xd = tc.cl(tc.randn(77001, (2, 16, 3, 8, 7))), tc.cl(tc.randn(77002, (2, 16, 3, 8, 7)))
    return lambda: i2v_native.disc3d_gp_maxpool_tangent_unit(xd.to(DEV), i2v_native.disc3d_maxpool_unit(x.to(DEV))[1])


def _head_unit():
    xd, w = tc.cl(tc.randn(77003, (3, 48, 1, 4, 4))), tc.randn(77004, (1, 48))
    return lambda: list(i2v_native.disc3d_gp_head_dual_unit(xd.to(DEV), w.to(DEV), gp.W_GP))


CASES = [pytest.param(_gn_units(gp.GN_CASES[1]), id="groupnorm-units-c16-2x5x7-b3"), pytest.param(_gn_units(gp.GN_CASES[6]), id="groupnorm-units-c48-sliced"),
         pytest.param(_pool_unit(), id="maxpool-tangent-unit"), pytest.param(_head_unit(), id="head-dual-unit"),
         pytest.param(lambda: _step(_handle(), SHAPE_A, dev_scale=True), id="handle-every-entry"),
         pytest.param(lambda: _step(_handle(tc.CFG_C), (3, 3, 4, 16, 16)), id="handle-without-the-pool")]


@pytest.mark.parametrize("fn", CASES)
def test_entry_on_poisoned_guard_banded_buffers(fn, monkeypatch, request):
    stats = {}
    outs = bh.run_three(fn, i2v_native, monkeypatch, request.node.callspec.id, stats)
    assert stats["runs"] == 2 and stats["allocations"] > 0 and stats["foreign"] == 0
    assert all(bool(torch.isfinite(o).all()) for o in outs if o.is_floating_point())
    print(f"  HYGIENE {request.node.callspec.id}: {len(outs)} tensors, 3 runs agree bit for bit, guards intact; workspace / saved bytes as reported "
          f"{stats['last_uint8']}")


def test_handle_reuse_across_shapes():
    """A = [2, 3, 3, 32, 32], B = [4, 3, 4, 32, 32] (more samples, the longer clip, the larger workspace), A again."""
    live = _handle()
    for shape in (SHAPE_A, SHAPE_B, SHAPE_A):
        if live[0]._ws.buf is not None:
            live[0]._ws.buf.fill_(0xFF)
        got = [t.clone() for t in _step(live, shape)]
        want = _step(_handle(), shape)
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert bh.same_bits(a, b), f"handle reuse across shapes: {shape}, output {i} {tuple(a.shape)} differs from a fresh handle's"
