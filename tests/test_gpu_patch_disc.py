"""GPU checks of the patch discriminator (csrc/i2v_patchdisc.hip, stage1_VAE/modules/patch_disc.py, i2v_train.PatchDiscTrainer): every
kernel against float64 at the derived bound of tests/patch_disc_common.py, the module against the fixture made from the reference's own
module (tests/golden/patch_disc*.npz) and against the float64 oracle that takes the GPU's LeakyReLU masks, the bit-level properties
(two runs, batch rows, autograd form = fused step) and two short trainings.  Run with ``-s`` to see the figures of profiles/patch_disc_gate.md."""
import os

import numpy as np
import pytest
import torch

import i2v_native
import i2v_train
import patch_disc_common as pc
from stage1_VAE.modules.patch_disc import ActNorm, NLayerDiscriminator

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYERS = pc.spec(16, 3)


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
    """Other modules of the suite switch grad mode off for the process; these tests are about gradients."""
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "patch_disc.npz")) as a, np.load(os.path.join(GOLDEN, "patch_disc_grads.npz")) as g:
        return {k: a[k] for k in a.files}, {k: g[k] for k in g.files}


def params_of(main, prefix="p."):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in main.items() if k.startswith(prefix)}


def fixture_module(main, after=False):
    net = NLayerDiscriminator(dict(pc.FIXTURE_CFG))
    sd = params_of(main)
    if after:
        sd.update({k: v.to(sd[k].dtype) for k, v in params_of(main, "after.").items()})
    net.load_state_dict(sd)
    return net.to(DEV)


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def report(name, ok, ratio, l2):
    print(f"  {name}: |err|/bound {ratio:.3f}  rel-L2 {l2:.2e}")
    assert ok, (name, ratio, l2)


# ---------------------------------------------------------------------------------------------------------------- units

@pytest.mark.parametrize("case", pc.conv_cases(), ids=lambda c: c["id"])
def test_conv_forward_unit(case):
    x, w, bias, loc, scale = pc.conv_inputs(case)
    ep = case["epilogue"]
    norm, lrelu = ep == "actnorm_lrelu", ep != "bias"
    ref, pre, S, n = pc.conv_oracle(x, w, bias, loc if norm else None, scale if norm else None, case["stride"], lrelu)
    out, gpre = i2v_native.patchdisc_conv_unit(pc.cl(x).to(DEV), w.to(DEV), bias.to(DEV), loc.to(DEV) if norm else None, scale.to(DEV) if norm else None,
                                               stride=case["stride"], lrelu=lrelu, want_pre=True)
    report(case["id"] + " " + ep, *pc.gate(pc.uncl(out.cpu()), ref, S, n))
    Sp = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=case["stride"], padding=1)
    report(case["id"] + " pre", *pc.gate(pc.uncl(gpre.cpu()), pre, Sp, 16 * case["cin"] + 1))


@pytest.mark.parametrize("case", pc.conv_cases(), ids=lambda c: c["id"])
def test_dgrad_unit(case):
    g, w, act, scale = pc.dgrad_inputs(case)
    k = case["seed"] // 10
    use_act, use_scale, frames = k % 2 == 0, k % 4 < 2, case["cin"] == 3 and k % 3 == 0
    ref, S, n = pc.dgrad_oracle(g, w, act if use_act else None, scale if use_scale else None, case["hw"], case["stride"])
    out = i2v_native.patchdisc_dgrad_unit(pc.cl(g).to(DEV), w.to(DEV), case["hw"], pc.cl(act).to(DEV) if use_act else None, scale.to(DEV) if use_scale else None,
                                          stride=case["stride"], frames=frames).cpu()
    if not frames:
        if case["cin"] == 3:
            assert float(out[..., 3].abs().max()) == 0.0
            out = out[..., :3]
        out = pc.uncl(out)
    report(f"{case['id']} mask{int(use_act)} scale{int(use_scale)} frames{int(frames)}", *pc.gate(out, ref, S, n))


@pytest.mark.parametrize("case", pc.big_cases(), ids=lambda c: c["id"])
def test_large_maps_take_the_128_row_tile(case):
    """The 16- and 32-column forms of the two GEMM kernels past the threshold of their 128-row tile (the 64-column forms and the frames form:
    test_module_at_128_runs_the_128_row_kernels), at the same bound as the small cases."""
    bn = lambda c: 64 if c % 64 == 0 else 32 if c % 32 == 0 else 16
    h, w_, s_ = case["hw"][0], case["hw"][1], case["stride"]
    if case["kind"] == "conv":
        assert pc.rows_per_workgroup(((h - 2) // s_ + 1) * ((w_ - 2) // s_ + 1), case["cout"] // bn(case["cout"])) == 128
        test_conv_forward_unit(case)
    else:
        rows = ((h + 1) // 2) * ((w_ + 1) // 2) * 4 if s_ == 2 else h * w_
        assert pc.rows_per_workgroup(rows, case["cin"] // bn(case["cin"])) == 128
        g, w, act, scale = pc.dgrad_inputs(case)
        ref, S, n = pc.dgrad_oracle(g, w, act, scale, case["hw"], s_)
        out = i2v_native.patchdisc_dgrad_unit(pc.cl(g).to(DEV), w.to(DEV), case["hw"], pc.cl(act).to(DEV), scale.to(DEV), stride=s_).cpu()
        report(case["id"], *pc.gate(pc.uncl(out), ref, S, n))


@pytest.mark.parametrize("case", pc.wgrad_cases(), ids=lambda c: c["id"])
def test_wgrad_unit(case):
    x, w, _, _, _ = pc.conv_inputs(case)
    g, _, act, scale = pc.dgrad_inputs(case)
    positions = g.shape[0] * g.shape[2] * g.shape[3]
    slices, slice_len = i2v_native.patchdisc_wgrad_plan(case["cout"], case["cin"], positions)
    want = {"one-slice": lambda: slices == 1, "even-slices": lambda: slices > 1 and slices * slice_len == positions,
            "ragged": lambda: slices > 1 and slices * slice_len > positions}
    assert want.get(case["id"], lambda: True)(), (slices, slice_len, positions)
    u = v = sigma = None
    if case["project"]:
        u, v, sigma = pc.power_iteration(w.double().reshape(w.shape[0], -1), pc.randn(case["seed"] + 7, (w.shape[0],)).double(),
                                         pc.randn(case["seed"] + 8, (w[0].numel(),)).double())
        u, v, sigma = u.float(), v.float(), sigma.float().reshape(1)
    ref, refb, bound, boundb = pc.wgrad_oracle(g, x, w, act, scale, case["stride"], u, v, sigma)
    dev = lambda t: None if t is None else t.to(DEV)
    args = (pc.cl(g).to(DEV), pc.cl(x).to(DEV), w.to(DEV), pc.cl(act).to(DEV), scale.to(DEV), dev(u), dev(v), dev(sigma))
    dw, db = i2v_native.patchdisc_wgrad_unit(*args, stride=case["stride"])
    report(f"{case['id']} {slices}x{slice_len} dW", *pc.gate_bound(dw.cpu(), ref, bound))
    report(f"{case['id']} db", *pc.gate_bound(db.cpu().view(1, -1), refb.view(1, -1), boundb.view(1, -1)))
    dw2, db2 = i2v_native.patchdisc_wgrad_unit(*args, stride=case["stride"])
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    base_w, base_b = pc.randn(case["seed"] + 9, tuple(w.shape)).to(DEV), pc.randn(case["seed"] + 10, (w.shape[0],)).to(DEV)
    acc_w, acc_b = i2v_native.patchdisc_wgrad_unit(*args, stride=case["stride"], dweight=base_w.clone(), dbias=base_b.clone())
    assert torch.equal(acc_w, base_w + dw) and torch.equal(acc_b, base_b + db)


@pytest.mark.parametrize("case", pc.HEAD_CASES, ids=lambda c: c["id"])
def test_head_unit(case):
    cin, (h, w_), b = case["cin"], case["hw"], case["batch"]
    x = pc.randn(case["seed"], (b, cin, h, w_))
    w = pc.randn(case["seed"] + 1, (1, cin, 4, 4)) * float(np.sqrt(1.0 / (16 * cin)))
    bias, g = pc.randn(case["seed"] + 2, (1,)), pc.randn(case["seed"] + 3, (b, 1, h - 1, w_ - 1))
    ref, _, S, n = pc.conv_oracle(x, w, bias, None, None, 1, False)
    out, dx, dw, db = i2v_native.patchdisc_head_unit(pc.cl(x).to(DEV), w.to(DEV), bias.to(DEV), g.reshape(b, h - 1, w_ - 1).contiguous().to(DEV))
    report(case["id"] + " out", *pc.gate(out.cpu().unsqueeze(1), ref, S, n))
    rx, Sx, nx = pc.dgrad_oracle(g, w, None, None, (h, w_), 1)
    report(case["id"] + " dx", *pc.gate(pc.uncl(dx.cpu()), rx, Sx, nx))
    rw, rb, bw, bb = pc.wgrad_oracle(g, x, w, None, None, 1)
    report(case["id"] + " dW", *pc.gate_bound(dw.cpu(), rw, bw))
    report(case["id"] + " db", *pc.gate_bound(db.cpu().view(1, 1), rb.view(1, 1), bb.view(1, 1)))


@pytest.mark.parametrize("shape", pc.POWER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_power_iteration_unit(shape):
    rows, cols = shape
    W = pc.randn(44000 + rows, (rows, cols)) * float(np.sqrt(1.0 / cols))
    u0 = torch.nn.functional.normalize(pc.randn(44001 + rows, (rows,)), dim=0)
    v0 = torch.nn.functional.normalize(pc.randn(44002 + rows, (cols,)), dim=0)
    ru, rv, rs = pc.power_iteration(W.double(), u0.double(), v0.double())
    u, v = u0.clone().to(DEV), v0.clone().to(DEV)
    sigma = i2v_native.patchdisc_power_iteration_unit(W.to(DEV), u, v, iterate=True)
    # every sum is float64 from exact fp32 products: the results are the float64 ones rounded once, v's rounding carried into u and sigma
    tol = 8 * pc.U
    print(f"  {rows}x{cols}: u {rel(u, ru):.2e} v {rel(v, rv):.2e} sigma {abs(float(sigma) - float(rs)) / abs(float(rs)):.2e}")
    assert float((u.cpu().double() - ru).abs().max()) <= tol * float(ru.abs().max()) + 1e-30
    assert float((v.cpu().double() - rv).abs().max()) <= tol * float(rv.abs().max()) + 1e-30
    assert abs(float(sigma) - float(rs)) <= tol * abs(float(rs))
    same = i2v_native.patchdisc_power_iteration_unit(W.to(DEV), u0.clone().to(DEV), v0.clone().to(DEV), iterate=False)
    assert abs(float(same) - float(torch.dot(u0.double(), W.double() @ v0.double()))) <= tol * float(W.double().abs().sum(1).max())


@pytest.mark.parametrize("shape", ((1, 6, 7, 16), (3, 8, 8, 48), (20, 16, 16, 128)), ids=lambda s: "x".join(map(str, s)))
def test_actnorm_init_unit(shape):
    n, h, w, c = shape
    pre = (pc.randn(45000 + c, (n * h * w, c)) * 1.7 + 0.4).to(DEV)
    loc, scale = i2v_native.patchdisc_actnorm_init_unit(pre)
    p64 = pre.cpu().double()
    rl, rs = -p64.mean(0), 1.0 / (p64.std(0) + 1e-6)
    ulp = lambda got, ref: float(((got.cpu().double() - ref).abs() / (ref.abs() * 2.0 ** -23)).max())
    print(f"  {shape}: loc {ulp(loc, rl):.2f} ulp  scale {ulp(scale, rs):.2f} ulp")
    assert ulp(loc, rl) <= 2 and ulp(scale, rs) <= 2


def test_hinge_entry():
    fake, real = pc.randn(46000, (4, 1, 6, 6)) * 1.5, pc.randn(46001, (4, 1, 6, 6)) * 1.5
    fake.view(-1)[:3] = torch.tensor([-1.0, -1.0, 1.0])      # exactly at the hinge: relu'(0) = 0
    real.view(-1)[:3] = torch.tensor([1.0, -1.0, 1.0])
    out, df, dr = i2v_native.patchdisc_hinge(fake.to(DEV), real.to(DEV), "disc")
    rf, rr = pc.hinge_disc_grads(fake.double(), real.double())
    want = [float(pc.hinge_disc(fake.double(), real.double())), float(real.double().mean()), float(fake.double().mean())]
    assert np.allclose(out.cpu().numpy(), want, rtol=1e-14, atol=1e-15)
    assert torch.equal(df.cpu(), rf.float()) and torch.equal(dr.cpu(), rr.float())
    assert float(df.view(-1)[0]) == 0.0 and float(dr.view(-1)[0]) == 0.0 and float(df.view(-1)[2]) > 0 and float(dr.view(-1)[1]) < 0
    out, df, dr = i2v_native.patchdisc_hinge(fake.to(DEV), None, "gen")
    assert abs(float(out[0]) + float(fake.double().mean())) < 1e-15 and dr is None
    assert torch.equal(df.cpu(), torch.full_like(fake, -1.0 / fake.numel()))


# ---------------------------------------------------------------------------------------------------------------- the module

def test_eval_forward_matches_the_reference_fixture(fx):
    main, _ = fx
    net = fixture_module(main, after=True).eval()
    u_before = net.main[0].weight_u.clone()
    with torch.no_grad():
        for tag in pc.EVAL_SHAPES:
            x = pc.eval_inputs(tag).to(DEV)
            pred = net(x)
            l2 = pc.rel_l2_rows(pred.cpu(), torch.from_numpy(main["eval_" + tag]))
            print(f"  eval {tag}: rel-L2 per image {max(l2):.2e}")
            assert pred.shape == main["eval_" + tag].shape and max(l2) <= pc.TOL_L2
            for i in range(x.shape[0]):     # a batch row has the bits of its single-image run
                assert torch.equal(net(x[i:i + 1].contiguous())[0], pred[i])
    assert torch.equal(net.main[0].weight_u, u_before)       # eval mode: no iteration


def gpu_masks(net, saved, shape):
    acts = net._handle().saved_activations(saved, shape)
    return [pc.uncl(a.cpu()) > 0 for a, _ in acts]


def check_fragile(masks, cache, limit=pc.FRAGILE_MAX):
    total = 0
    for m, st in zip(masks, cache["steps"]):
        n, outside = pc.fragile_units(m, st["h"])
        assert outside == 0, "a mask differs from float64 away from zero"
        total += n
    assert total <= limit
    return total


def test_training_step_matches_the_reference_fixture(fx):
    """From initialized = 0: forward on the fake batch (it initialises ActNorm), forward on the real batch, hinge, backward, through
    autograd.  Against the reference's numbers, and against the float64 oracle on the GPU's masks."""
    main, grads = fx
    net = fixture_module(main).train()
    fake, real = pc.train_inputs()
    xf, xr = fake.to(DEV).requires_grad_(True), real.to(DEV).requires_grad_(True)
    pf, pr = net(xf), net(xr)
    assert pf.grad_fn is not None
    loss = pc.hinge_disc(pf, pr)
    loss.backward()
    assert all(int(m.initialized) == 1 for m in net.main if isinstance(m, ActNorm))
    rows = {"pred_fake": (pf, main["train_pred_fake"]), "pred_real": (pr, main["train_pred_real"]), "dx_fake": (xf.grad, main["train_dx_fake"]),
            "dx_real": (xr.grad, main["train_dx_real"])}
    for k, (got, ref) in rows.items():
        l2 = max(pc.rel_l2_rows(got.detach().cpu(), torch.from_numpy(ref)))
        print(f"  {k}: rel-L2 per image {l2:.2e}")
        assert l2 <= pc.TOL_L2, k
    assert abs(float(loss.detach()) - float(main["train_loss"])) <= 1e-5 * float(main["train_loss"])
    for k, p in net.named_parameters():
        l2 = rel(p.grad, grads[k])
        print(f"  grad {k}: rel-L2 {l2:.2e}")
        assert l2 <= pc.TOL_L2, k
    for k, v in net.state_dict().items():
        if ("after." + k) in main and not k.endswith("initialized"):
            l2 = rel(v, main["after." + k])
            print(f"  after {k}: rel-L2 {l2:.2e}")
            assert l2 <= pc.TOL_L2, k


def oracle_check(net, sd, x, d_pred_of, init, tag, fragile_limit=pc.FRAGILE_MAX):
    """One saved forward + backward of ``net`` on the handle against the oracle with the GPU's masks -> the updated oracle state."""
    layers = pc.spec(net.cfg["ndf"], net.cfg["n_layers"])
    pred, saved = net._run(x.to(DEV), save=True)
    masks = gpu_masks(net, saved, tuple(x.shape))
    ref, cache = pc.forward_oracle(sd, x, layers, training=True, init=init, masks=masks)
    print(f"  {tag}: {check_fragile(masks, cache, fragile_limit)} mask units differ from float64 (all within 1e-5 rms)")
    assert max(pc.rel_l2_rows(pred.cpu(), ref)) <= pc.TOL_L2
    d_pred = d_pred_of(ref)
    names = [k for k, _ in net.named_parameters()]
    gbuf = {k: torch.zeros_like(p) for k, p in net.named_parameters()}
    dx = net._handle(gbuf).backward(d_pred.float().to(DEV), saved, tuple(x.shape), need_dx=True, param_grads=True, accumulate=False)
    rg, rdx = pc.backward_oracle(cache, d_pred)
    worst = max(pc.rel_l2_rows(dx.cpu(), rdx))
    assert worst <= pc.TOL_L2, ("dx", worst)
    for k in names:
        l2 = rel(gbuf[k], rg[k])
        worst = max(worst, l2)
        assert l2 <= pc.TOL_L2, (k, l2)
    print(f"  {tag}: worst rel-L2 over dx rows and parameter gradients {worst:.2e}")
    return dict(sd, **cache["state"])


def test_training_step_matches_the_oracle_on_the_gpu_masks(fx):
    main, _ = fx
    net = fixture_module(main).train()
    fake, real = pc.train_inputs()
    sd = params_of(main)
    with torch.no_grad():
        sd = oracle_check(net, sd, fake, lambda p: pc.hinge_disc_grads(p, -p)[0], True, "fake")
        oracle_check(net, sd, real, lambda p: pc.hinge_disc_grads(-p, p)[1], False, "real")


def test_shipped_shape_once():
    """ndf 64, 20 frames at 64 x 64: forward + backward against the float64 oracle on the GPU's masks."""
    torch.manual_seed(4200)
    net = NLayerDiscriminator({"in_channels": 3, "ndf": 64, "n_layers": 3, "use_actnorm": True, "spectral_norm": True})
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(DEV).train()
    x = 0.6 * pc.randn(4201, (20, 3, 64, 64))
    with torch.no_grad():
        oracle_check(net, sd, x, lambda p: torch.cos(torch.arange(p.numel(), dtype=torch.float64)).view_as(p) / p.numel(), True, "shipped")


def test_module_at_128_runs_the_128_row_kernels():
    """ndf 64, 16 frames at 128 x 128 (the frame size of the larger rows of profiles/patch_disc_ab.md; 16 frames are the fewest that cross the
    threshold): conv 0 (64 columns) and the input gradients of conv 1 (64 columns) and conv 0 (16 columns, writing the frames' layout) run
    the 128-row tile.  Forward + backward against the oracle on the GPU's masks.  Masks: the allowance of 4 units was stated for cases up to
    the shipped shape; a sign flips where fp32 rounding exceeds |h|, a fixed chance per unit, so this case gets the same RATE: 4 per as many
    units as the shipped shape has, rounded up."""
    units = lambda n, s: n * sum(c * (s // d) ** 2 for c, d in ((64, 2), (128, 4), (256, 8))) + n * 512 * (s // 8 - 1) ** 2
    limit = pc.FRAGILE_MAX * -(-units(16, 128) // units(20, 64))
    assert limit == 16 and pc.rows_per_workgroup(16 * 64 * 64, 1) == 128 and pc.rows_per_workgroup(16 * 128 * 128, 1) == 128
    torch.manual_seed(4210)
    net = NLayerDiscriminator({"in_channels": 3, "ndf": 64, "n_layers": 3, "use_actnorm": True, "spectral_norm": True})
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(DEV).train()
    x = 0.6 * pc.randn(4211, (16, 3, 128, 128))
    with torch.no_grad():
        oracle_check(net, sd, x, lambda p: torch.cos(torch.arange(p.numel(), dtype=torch.float64)).view_as(p) / p.numel(), True, "128 x 128", fragile_limit=limit)


def test_without_spectral_norm():
    """spectral_norm: False is the same code with sigma = 1 and no u, v: forward + backward against the oracle, and the autograd form."""
    torch.manual_seed(4220)
    cfg = dict(pc.FIXTURE_CFG, spectral_norm=False)
    net = NLayerDiscriminator(cfg)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    assert "main.0.weight" in sd and not any(k.endswith(("weight_u", "weight_orig")) for k in sd)
    net = net.to(DEV).train()
    fake, real = pc.train_inputs()
    with torch.no_grad():
        sd = oracle_check(net, sd, fake, lambda p: pc.hinge_disc_grads(p, -p)[0], True, "no spectral norm, fake")
        oracle_check(net, sd, real, lambda p: pc.hinge_disc_grads(-p, p)[1], False, "no spectral norm, real")
    loss = pc.hinge_disc(net(fake.to(DEV)), net(real.to(DEV)))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def test_too_small_inputs_are_refused_before_any_launch():
    """An input that shrinks below a 1 x 1 output raises from the handle and from the module; 24 px, the smallest, passes."""
    net = NLayerDiscriminator(dict(pc.FIXTURE_CFG)).to(DEV).eval()
    h = net._handle()
    assert h.out_shape(24, 24) == (1, 1) and h.out_shape(24, 40) == (1, 3) and h.out_shape(64, 64) == (6, 6)
    assert h.saved_bytes(2, 24, 24) > 0 and h.saved_bytes(2, 23, 64) == 0
    with torch.no_grad():
        assert net(torch.zeros(2, 3, 24, 24, device=DEV)).shape == (2, 1, 1, 1)
        for shape in ((2, 3, 23, 64), (2, 3, 64, 23), (1, 3, 8, 8)):
            with pytest.raises(i2v_native.I2VError, match="shrinks below"):
                h.out_shape(shape[2], shape[3])
            with pytest.raises(i2v_native.I2VError, match="shrinks below"):
                net(torch.zeros(*shape, device=DEV))
    deep = NLayerDiscriminator(dict(pc.FIXTURE_CFG, n_layers=4)).to(DEV).eval()
    with torch.no_grad():
        with pytest.raises(i2v_native.I2VError, match="shrinks below"):
            deep._handle().out_shape(24, 24)
        with pytest.raises(i2v_native.I2VError, match="shrinks below"):
            deep(torch.zeros(1, 3, 24, 24, device=DEV))
        assert deep(torch.zeros(1, 3, 48, 48, device=DEV)).shape == (1, 1, 1, 1)
    with pytest.raises(i2v_native.I2VError, match="shrinks below"):     # the backward refuses the shape too (nothing is read before the check)
        d = torch.zeros(1, 1, 1, 1, device=DEV)
        h.backward(d, torch.zeros(1024, dtype=torch.uint8, device=DEV), (1, 3, 23, 23), need_dx=True, param_grads=False)


def test_copies_of_a_module_that_has_run_get_their_own_handle(fx):
    import copy
    main, _ = fx
    net = fixture_module(main, after=True).eval()
    x = pc.eval_inputs("e32").to(DEV)
    with torch.no_grad():
        a = net(x)
        twin = copy.deepcopy(net)
        assert twin._native is None and net._native is not None
        assert torch.equal(twin(x), a) and torch.equal(net(x), a)


def test_bits_autograd_trainer_repeat_and_frozen(fx):
    """The autograd form and PatchDiscTrainer.step give the same gradient bits; two runs give the same bits; generator_loss leaves .grad
    untouched and equals the autograd input gradient; a frozen module returns only the input gradient."""
    main, _ = fx
    fake, real = (t.to(DEV) for t in pc.train_inputs())

    def auto():
        net = fixture_module(main).train()
        loss = pc.hinge_disc(net(fake), net(real))
        loss.backward()
        return net, loss

    a, la = auto()
    b, lb = auto()
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters())) and torch.equal(la, lb)

    net = fixture_module(main).train()
    tr = i2v_train.PatchDiscTrainer(net, lr=0.0, weight_decay=0.0)
    l, mr, mf = tr.step(fake, real)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), net.parameters()))
    assert abs(float(l) - float(la)) <= 1e-6 * float(la)
    for k in ("weight_u", "weight_v"):
        assert torch.equal(getattr(a.main[0], k), getattr(net.main[0], k))
    assert torch.equal(a.main[3].scale, net.main[3].scale)

    before = [p.grad.clone() for p in net.parameters()]
    lg, dx = tr.generator_loss(fake)
    assert all(torch.equal(p.grad, q) for p, q in zip(net.parameters(), before))
    a.requires_grad_(False)
    xf = fake.clone().requires_grad_(True)
    (-a(xf).mean()).backward()
    assert torch.equal(xf.grad, dx)
    assert all(torch.equal(p.grad, q) for p, q in zip(a.parameters(), before))      # frozen: nothing was added
    assert np.isfinite(float(lg))


def test_three_forwards_move_u_three_times_and_actnorm_inits_once(fx):
    main, _ = fx
    net = fixture_module(main).train()
    fake, real = (t.to(DEV) for t in pc.train_inputs())
    sd = params_of(main)
    seen = []
    with torch.no_grad():
        for i, x in enumerate((fake, real, fake)):
            net(x)
            seen.append(net.main[5].weight_u.clone())
            _, cache = pc.forward_oracle(sd, x.cpu(), LAYERS, training=True, init=i == 0)
            sd = dict(sd, **cache["state"])
            assert rel(seen[-1], sd["main.5.weight_u"]) <= 1e-6
            if i == 0:
                loc = net.main[6].loc.clone()
            assert torch.equal(net.main[6].loc, loc)          # set by the first forward only
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert rel(net.main[6].loc, sd["main.6.loc"]) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- training

def test_six_sgd_steps_follow_the_reference(fx):
    main, _ = fx
    net = fixture_module(main).train()
    fake, real = (t.to(DEV) for t in pc.train_inputs())
    losses = []
    for _ in range(pc.SGD_STEPS):
        net.zero_grad()
        loss = pc.hinge_disc(net(fake), net(real))
        loss.backward()
        with torch.no_grad():
            for p in net.parameters():
                p -= pc.SGD_LR * p.grad
        losses.append(float(loss))
    print("  losses:", [f"{v:.6f}" for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert np.allclose(losses, main["sgd_losses"], rtol=1e-4, atol=0)


def test_fused_adam_trainer_five_steps(fx):
    main, _ = fx
    net = fixture_module(main).train()
    tr = i2v_train.PatchDiscTrainer(net)
    fake, real = (t.to(DEV) for t in pc.train_inputs())
    losses = [float(tr.step(fake, real)[0]) for _ in range(5)]
    print("  losses:", [f"{v:.6f}" for v in losses])
    assert losses[-1] < losses[0] and all(torch.isfinite(p).all() for p in net.parameters())
