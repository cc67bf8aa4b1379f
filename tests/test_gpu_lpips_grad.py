"""GPU checks of the LPIPS backward pass (csrc/i2v_vgg.hip, csrc/i2v_lpips.hip): the input-gradient convolution and its first-layer form against float64 at
the dot-product bound, the max-pool backward bit for bit against torch, the LPIPS head backward against its closed form, and
``LPIPS(x0, x1).backward()`` / ``vgg16(X)`` end to end against the float64 graph that takes its ReLU masks and pool arg-max from the GPU's
own saved activations, and against the gradients of the reference's module (tests/golden/vgg_lpips_grad.npz).  Run with ``-s`` to see the
figures of profiles/lpips_grad_gate.md."""
import ctypes

import pytest
import torch

import i2v_native
import lpips_grad_common as lg
import vgg_common as vc
from stage2_cINN.AE.modules.LPIPS import LPIPS
from stage2_cINN.AE.modules.vgg16 import vgg16

pytestmark = pytest.mark.gpu
DEV = "cuda"
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
    """Other modules of the suite switch grad mode off for the process; these tests are about gradients."""
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


def model(kind):
    """vgg16 / LPIPS filled from the synthesiser with the fixture's seeds (no file involved), one per process."""
    if kind not in _MODELS:
        own = {k: torch.from_numpy(v) for k, v in zip(vc.holder_keys(), vc.vgg_state_dict(lg.SEED_W).values())}
        if kind == "vgg":
            m = vgg16(pretrained=False)
            m.load_state_dict(own, strict=True)
        else:
            m = LPIPS()
            sd = {"net." + k: v for k, v in own.items()}
            sd.update({k: torch.from_numpy(v) for k, v in vc.lin_state_dict(lg.SEED_LIN).items()})
            m.load_state_dict(sd, strict=False)
        _MODELS[kind] = m.to(DEV).eval()
    return _MODELS[kind]


def weights():
    return vc.vgg_state_dict(lg.SEED_W), vc.lin_state_dict(lg.SEED_LIN)


# ---------------------------------------------------------------------------------------------------------------- dgrad unit

def _dgrad_gpu(case, g, w, add, y):
    cl = lambda t: None if t is None else vc.to_cl(t).to(DEV)  # noqa: E731
    return lg.to_nchw(i2v_native.vgg_dgrad_unit(cl(g), w, cl(add), cl(y)))


@pytest.mark.parametrize("case", lg.dgrad_cases(), ids=lambda c: c["id"])
def test_dgrad_unit_vs_float64_at_the_dot_product_bound(case):
    g, w, add, y, other = lg.dgrad_inputs(case)
    ref, S, n = lg.dgrad_oracle(g, w, add, y)
    got = _dgrad_gpu(case, g, w, add, y)
    ok, ratio, l2 = lg.gate(got, ref, S, n)
    print(f"dgrad {case['id']}: worst |err| / bound {ratio:.3f}, worst rel-L2 {l2:.2e} (n = {n})")
    assert n == 9 * case["cout"] and ok, (ratio, l2)


@pytest.mark.parametrize("cin,cout,hw", [(64, 64, (9, 17)), (128, 48, (17, 33)), (64, 16, (5, 7))])
def test_dgrad_gate_tells_the_mutated_oracles_apart(cin, cout, hw):
    case = {"cin": cin, "cout": cout, "hw": hw, "batch": 2, "mask": 1, "add": 1, "seed": 17700 + cin + cout}
    g, w, add, y, other = lg.dgrad_inputs(case)
    got = _dgrad_gpu(case, g, w, add, y)
    ref, S, n = lg.dgrad_oracle(g, w, add, y)
    assert lg.gate(got, ref, S, n)[0]
    for m in lg.DGRAD_MUTATIONS:
        if m == "kernel_not_transposed" and cin != cout:
            continue
        assert not lg.gate(got, lg.dgrad_oracle(g, w, add, y, mutate=m, other=other)[0], S, n)[0], m


@pytest.mark.parametrize("case", lg.first_cases(), ids=lambda c: c["id"])
def test_first_layer_dgrad_vs_float64(case):
    g, w, _, _, _ = lg.dgrad_inputs(case)
    ref, S, n = lg.dgrad_oracle(g, w, scale=vc.LPIPS_SCALE if case["frames"] else None)
    got = i2v_native.vgg_dgrad_unit(vc.to_cl(g).to(DEV), w, frames=bool(case["frames"])).cpu()
    if not case["frames"]:
        assert torch.count_nonzero(got[..., 3]) == 0
        got = got[..., :3].permute(0, 3, 1, 2)
    ok, ratio, l2 = lg.gate(got, ref, S, n)
    print(f"dgrad {case['id']}: worst |err| / bound {ratio:.3f}, worst rel-L2 {l2:.2e} (n = {n})")
    assert n == 576 + case["frames"] and ok, (ratio, l2)
    for m in ("taps_not_flipped", "drop_border_tap"):
        assert not lg.gate(got, lg.dgrad_oracle(g, w, scale=vc.LPIPS_SCALE if case["frames"] else None, mutate=m)[0], S, n)[0], m


def test_dgrad_batch_rows_equal_single_image_runs_bit_for_bit():
    for case in ({"cin": 128, "cout": 48, "hw": (17, 33), "batch": 3, "mask": 1, "add": 1, "seed": 17800},
                 {"cin": 3, "cout": 64, "hw": (17, 33), "batch": 3, "mask": 0, "add": 0, "seed": 17801}):
        g, w, add, y, _ = lg.dgrad_inputs(case)
        cl = lambda t, i=None: None if t is None else vc.to_cl(t if i is None else t[i:i + 1]).to(DEV)  # noqa: E731
        full = i2v_native.vgg_dgrad_unit(cl(g), w, cl(add), cl(y), frames=case["cin"] == 3)
        for i in range(3):
            assert torch.equal(full[i:i + 1], i2v_native.vgg_dgrad_unit(cl(g, i), w, cl(add, i), cl(y, i), frames=case["cin"] == 3)), i
        assert torch.equal(full, i2v_native.vgg_dgrad_unit(cl(g), w, cl(add), cl(y), frames=case["cin"] == 3))


@pytest.mark.parametrize("cin,cout", [(32, 16), (96, 64), (64, 8), (64, 24), (3, 32), (4, 64)])
def test_dgrad_bad_channel_counts_are_refused(cin, cout):
    with pytest.raises(i2v_native.I2VError, match="channels"):
        i2v_native.vgg_dgrad_unit(torch.zeros(1, 5, 5, cout, device=DEV), torch.zeros(cout, cin, 3, 3))


# ---------------------------------------------------------------------------------------------------------------- pool backward

@pytest.mark.parametrize("shape", lg.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["rnd", "neg", "ties", "ties12"])
def test_pool_backward_bit_for_bit_vs_torch(shape, kind):
    n, c, h, w = shape
    y = lg.pool_input(kind, shape, 18500 + h * w + c)
    g = vc.randn(18600 + h * w + c, (n, c, h // 2, w // 2))
    ref = lg.pool_backward_torch(y, g)
    got = lg.to_nchw(i2v_native.vgg_maxpool2_backward(vc.to_cl(g).to(DEV), vc.to_cl(y).to(DEV)))
    assert torch.equal(got, ref)
    if kind in ("ties", "ties12"):      # the constructed ties: all at window position 0, resp. 1
        k = 0 if kind == "ties" else 1
        assert torch.equal(got[:, :, 0:2 * (h // 2):2, k:2 * (w // 2):2], g)
    # the fused form of the trunk: + the tap gradient, x the ReLU mask of y (one fp32 add: exact against torch as well)
    add, yr = vc.randn(18700 + h * w + c, shape), torch.relu(y)
    got = lg.to_nchw(i2v_native.vgg_maxpool2_backward(vc.to_cl(g).to(DEV), vc.to_cl(yr).to(DEV), vc.to_cl(add).to(DEV), relu_mask=True))
    assert torch.equal(got, (lg.pool_backward_torch(yr, g) + add) * (yr > 0))


# ---------------------------------------------------------------------------------------------------------------- head backward

@pytest.mark.parametrize("case", lg.HEAD_CASES, ids=lambda c: c["id"])
@pytest.mark.parametrize("which", ["side0", "side1", "both"])
def test_head_backward_vs_float64(case, which):
    f0, f1, lin, u = lg.head_inputs(case)
    d0, d1, B0, B1 = lg.head_backward_oracle(f0, f1, lin, u)
    g0, g1 = i2v_native.lpips_layer_backward(vc.to_cl(f0).to(DEV), vc.to_cl(f1).to(DEV), lin.to(DEV), u.to(DEV), which != "side1", which != "side0")
    assert (g0 is None) == (which == "side1") and (g1 is None) == (which == "side0")
    for name, got, ref, B in (("f0", g0, d0, B0), ("f1", g1, d1, B1)):
        if got is None:
            continue
        got = lg.to_nchw(got)
        ok, ratio, l2 = lg.head_gate(got, ref, B, case["c"])
        print(f"head {case['id']} {which} d{name}: worst |err| / bound {ratio:.3f}, worst rel-L2 {l2:.2e}")
        assert torch.isfinite(got).all() and ok, (name, ratio, l2)
    if case["hw"] != (1, 1) and g0 is not None:      # the all-zero feature vector: dn / eps, finite and not zero
        z = lg.to_nchw(g0)[0, :, 0, 1]
        assert torch.isfinite(z).all() and float(z.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- end to end

def _acts(saved):
    return None if saved is None else [lg.to_nchw(t) for t in saved.activations()]


def _lpips_case(a, b, wts, which):
    """(out, GPU gradients, oracle value, oracle gradients, fragile-unit figures) of one LPIPS forward + backward."""
    m = model("lpips")
    x0 = a.to(DEV).requires_grad_(which in ("input", "both"))
    x1 = b.to(DEV).requires_grad_(which in ("target", "both"))
    out = m(x0, x1)
    assert out.grad_fn is not None and out.dtype == torch.float32 and tuple(out.shape) == (a.shape[0], 1, 1, 1)
    saved = out.grad_fn.saved
    (wts.float().to(DEV).view(-1, 1, 1, 1) * out).sum().backward()
    sd, lin = weights()
    y0 = a.double().requires_grad_(x0.requires_grad)
    y1 = b.double().requires_grad_(x1.requires_grad)
    val, t0, t1 = lg.lpips_masked(sd, lin, y0, y1, _acts(saved[0]), _acts(saved[1]))
    (wts * val).sum().backward()
    fragile = [lg.fragile_units(t[1], _acts(s)) for t, s in ((t0, saved[0]), (t1, saved[1])) if s is not None]
    return out, (x0.grad, x1.grad), val.detach(), (y0.grad, y1.grad), (sum(f[0] for f in fragile), max(f[1] for f in fragile))


def _check_grads(tag, got, ref, fragile):
    count, worst = fragile
    for name, g, r in zip(("input", "target"), got, ref):
        assert (g is None) == (r is None), name
        if g is None:
            continue
        l2 = max(vc.rel_l2_rows(g.cpu(), r))
        print(f"e2e {tag} d{name}: worst rel-L2 per image {l2:.2e}; mask differences {count} (worst |pre| / rms {worst:.1e})")
        assert tuple(g.shape) == tuple(r.shape) and torch.isfinite(g).all() and l2 <= lg.TOL_L2, (name, l2)
    assert count <= lg.FRAGILE_MAX and worst <= lg.FRAGILE_REL, fragile


@pytest.mark.parametrize("case", lg.e2e_cases(), ids=lambda c: c["id"])
def test_lpips_backward_vs_float64_with_the_gpu_masks(case):
    a, b, wts = lg.e2e_frames(case)
    out, got, val, ref, fragile = _lpips_case(a, b, wts, case["which"])
    assert float(((out.detach().flatten().cpu().double() - val).abs() / val).max()) <= 1e-5
    _check_grads(case["id"], got, ref, fragile)


@pytest.mark.parametrize("tag", list(lg.GOLDEN))
def test_lpips_backward_vs_the_reference_module(tag):
    arr, meta = vc.load_fixture("vgg_lpips_grad")
    a, b, wts = lg.golden_frames(tag)
    out, got, _, _, _ = _lpips_case(a, b, wts, "both")
    for name, g in zip(("input", "target"), got):
        l2 = max(vc.rel_l2_rows(g.cpu(), torch.from_numpy(arr[f"grad_{name}_{tag}"])))
        print(f"reference {tag} d{name}: worst rel-L2 per image {l2:.2e}")
        assert l2 <= meta["gate_rel_l2"] == lg.TOL_L2, (name, l2)


def test_grad_mode_keeps_the_forward_bits_and_runs_repeat():
    m = model("lpips")
    a, b, wts = lg.e2e_frames({"hw": (24, 40), "n": 3, "seed": 19800})
    a, b = a.to(DEV), b.to(DEV)
    with torch.no_grad():
        plain = m(a, b.clone().requires_grad_(True))
    assert plain.grad_fn is None and m(a, b).grad_fn is None            # nothing requires grad: the existing path
    grads = []
    for _ in range(2):
        x0, x1 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = m(x0, x1)
        assert out.grad_fn is not None and torch.equal(out, plain)
        (wts.float().to(DEV).view(-1, 1, 1, 1) * out).sum().backward()
        grads.append((x0.grad, x1.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    for need0, need1 in ((True, False), (False, True)):                  # one side alone: the same values, the same gradient bits
        x0, x1 = a.clone().requires_grad_(need0), b.clone().requires_grad_(need1)
        out = m(x0, x1)
        assert torch.equal(out, plain)
        (wts.float().to(DEV).view(-1, 1, 1, 1) * out).sum().backward()
        assert torch.equal(x0.grad if need0 else x1.grad, grads[0][0 if need0 else 1]) and (x1.grad if need0 else x0.grad) is None
    for i in range(3):                                                   # a batch row equals its single-image run
        x0, x1 = a[i:i + 1].clone().requires_grad_(True), b[i:i + 1].clone().requires_grad_(True)
        out = m(x0, x1)
        assert torch.equal(out, plain[i:i + 1])
        (float(wts[i]) * out).sum().backward()
        assert torch.equal(x0.grad, grads[0][0][i:i + 1]) and torch.equal(x1.grad, grads[0][1][i:i + 1]), i
    with pytest.raises(RuntimeError):                                    # once differentiable
        x1 = b.clone().requires_grad_(True)
        g, = torch.autograd.grad(m(a, x1).sum(), x1, create_graph=True)
        g.sum().backward()


@pytest.mark.parametrize("hw", [(16, 16), (35, 29)])
def test_vgg16_taps_are_differentiable(hw):
    m = model("vgg")
    x = vc.randn(19900 + hw[0], (2, 3, *hw))
    X = x.to(DEV).requires_grad_(True)
    taps = m(X)
    assert taps._fields == vc.TAPS and all(t.grad_fn is not None for t in taps)
    with torch.no_grad():
        for t, p in zip(taps, m(X)):
            assert torch.equal(t, p)
    saved = taps[0].grad_fn.saved
    G = [vc.randn(19910 + k, tuple(t.shape)) for k, t in enumerate(taps)]           # NCHW-contiguous: not the taps' channels-last strides
    torch.autograd.backward(list(taps), [g.to(DEV) for g in G])
    Y = x.double().requires_grad_(True)
    t64, pres, _ = lg.trunk_masked(weights()[0], Y, _acts(saved))
    sum((t * g.double()).sum() for t, g in zip(t64, G)).backward()
    _check_grads(f"vgg16 taps {hw[0]}x{hw[1]}", (X.grad, None), (Y.grad, None), lg.fragile_units(pres, _acts(saved)))
    # one tap alone (the others get zeros), through a torch op behind it
    X2 = x.to(DEV).requires_grad_(True)
    m(X2).relu3_3.square().sum().backward()
    Y2 = x.double().requires_grad_(True)
    lg.trunk_masked(weights()[0], Y2, _acts(saved))[0][2].square().sum().backward()
    assert max(vc.rel_l2_rows(X2.grad.cpu(), Y2.grad)) <= lg.TOL_L2


def test_native_backward_under_graph_capture():
    native = model("lpips").net.native()
    a, _, _ = lg.e2e_frames({"hw": (20, 36), "n": 2, "seed": 19850})
    x = i2v_native.vgg_input_stage(a.to(DEV), i2v_native.VGG_INPUT_LPIPS)
    taps, saved = native.features(x, save=True)
    for t, p in zip(taps, native.features(x)):
        assert torch.equal(t, p)                                          # the saving variant returns the same tap bits
    g = [vc.randn(19860 + k, tuple(t.shape)).to(DEV) for k, t in enumerate(taps)]
    eager = {fr: native.backward(g, saved, frames=fr).clone() for fr in (False, True)}
    assert torch.equal(eager[True], native.backward(g, saved, frames=True))
    assert torch.count_nonzero(eager[False][..., 3]) == 0
    scale = torch.tensor(vc.LPIPS_SCALE, device=DEV).view(1, 3, 1, 1)
    assert torch.equal(eager[True], eager[False][..., :3].permute(0, 3, 1, 2) / scale)
    out = torch.zeros_like(eager[True])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        native.backward(g, saved, frames=True, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[True])


def test_gradient_steps_lower_lpips():
    m = model("lpips")
    a, b, _ = lg.e2e_frames({"hw": (16, 16), "n": 2, "seed": 19870})
    x0, x1 = a.to(DEV), b.to(DEV).requires_grad_(True)
    values, lr = [], None
    for _ in range(6):
        x1.grad = None
        loss = m(x0, x1).sum()
        values.append(float(loss.detach()))
        loss.backward()
        if lr is None:
            lr = 0.02 / float(x1.grad.abs().max())        # the largest pixel moves by 0.02 in the first step; the rate then stays
        with torch.no_grad():
            x1 -= lr * x1.grad
    print("LPIPS over five gradient steps on x1:", " ".join(f"{v:.6f}" for v in values))
    assert all(values[i + 1] < values[i] for i in range(5)), values


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refusals():
    native = model("lpips").net.native()
    x = i2v_native.vgg_input_stage(torch.zeros(1, 3, 16, 16, device=DEV), i2v_native.VGG_INPUT_LPIPS)
    taps, saved = native.features(x, save=True)
    with pytest.raises(i2v_native.I2VError, match="saved"):
        native.backward([torch.zeros_like(t) for t in taps], None)
    with pytest.raises(i2v_native.I2VError, match="five"):
        native.backward([torch.zeros_like(t) for t in taps[:4]], saved)
    with pytest.raises(i2v_native.I2VError, match="shape"):
        native.backward([torch.zeros_like(t) for t in taps[:4]] + [torch.zeros_like(taps[3])], saved)
    with pytest.raises(i2v_native.I2VError, match="16"):
        native.features(torch.zeros(1, 8, 8, 4, device=DEV), save=True)
    lib, ptrs = i2v_native.lib(), (ctypes.c_void_p * 5)(*[t.data_ptr() for t in taps])
    out, ws = torch.zeros(1, 16, 16, 4, device=DEV), torch.zeros(lib.i2v_vgg_backward_workspace_bytes(native._h, 1, 16, 16), dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.i2v_vgg_backward(native._h, ptrs, ptrs, None, 0, 1, 16, 16, out.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream) != 0
    assert b"saved" in lib.i2v_last_error()
    assert lib.i2v_vgg_backward(native._h, ptrs, ptrs, saved.buf.data_ptr(), saved.buf.numel(), 1, 8, 8, out.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                                stream) != 0
    assert lib.i2v_vgg_saved_bytes(native._h, 1, 8, 16) == 0 and lib.i2v_vgg_saved_bytes(native._h, 1, 16, 16) == saved.buf.numel()
    with pytest.raises(i2v_native.I2VError, match="channels"):
        i2v_native.lpips_layer_backward(torch.zeros(1, 2, 2, 32, device=DEV), torch.zeros(1, 2, 2, 32, device=DEV), torch.zeros(32, device=DEV),
                                        torch.zeros(1, dtype=torch.float64, device=DEV))
    with pytest.raises(NotImplementedError):
        vgg16(requires_grad=True, pretrained=False)                       # weight gradients stay refused
