"""GPU checks of the temporal discriminator (csrc/i2v_disc3d.hip, stage1_VAE/modules/resnet3D.py ``Discriminator``,
i2v_train.TemporalDiscTrainer): every kernel against float64 at the derived bound of tests/temporal_disc_common.py, the module against the
fixtures made from the reference's own module (tests/golden/temporal_disc_*.npz) and against the float64 oracle that takes the GPU's ReLU
masks and pool argmaxes, the bit-level properties (two runs, accumulate, autograd form = backward entry) and the trainer.  Run with ``-s``
to see the figures of profiles/temporal_disc_gate.md."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i2v_native
import i2v_train
import temporal_disc_common as tc
from stage1_VAE.modules.resnet3D import Discriminator

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHIPPED_T = 12     # the float64 oracle of the shipped widths at B = 1, T = 12, 64 x 64 takes under 20 s on 16 CPU threads


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
    """Other modules of the suite switch grad mode off for the process; these tests are about gradients."""
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


def load(pattern):
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, pattern))):
        with np.load(path) as a:
            out.update({k: a[k] for k in a.files})
    return out


def load_dx(name):
    return torch.from_numpy(np.stack([load(f"temporal_disc_a_dx_{name}{i}.npz")["dx"] for i in range(2)]))


@pytest.fixture(scope="module")
def fxa():
    params = {k: torch.from_numpy(v) for k, v in load("temporal_disc_a_params*.npz").items()}
    return load("temporal_disc_a.npz"), params, load("temporal_disc_a_grads*.npz")


@pytest.fixture(scope="module")
def fxb():
    return load("temporal_disc_b.npz"), load("temporal_disc_b_grads*.npz")


def module(cfg, sd, update=None):
    net = Discriminator(dict(cfg))
    sd = dict(sd)
    if update:
        sd.update({k: torch.as_tensor(v).to(sd[k].dtype) for k, v in update.items()})
    net.load_state_dict(sd)
    return net.to(DEV)


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rel_rows(a, b):
    """the worst relative L2 over the samples"""
    return max(tc.rel_l2_rows(torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()))


def report(name, ok, ratio, l2):
    print(f"  {name}: |err|/bound {ratio:.3f}  rel-L2 {l2:.2e}")
    assert ok, (name, ratio, l2)


def strides(case):
    return dict(stride_t=case["st"], stride_s=case["ss"])


# ---------------------------------------------------------------------------------------------------------------- units

@pytest.mark.parametrize("case", tc.conv_cases() + tc.STEM_CASES, ids=lambda c: c["id"])
def test_conv_forward_unit(case):
    x, w, _, _ = tc.conv_case_inputs(case)
    ref, S, n = tc.conv_oracle(x, w, case["st"], case["ss"])
    out = i2v_native.disc3d_conv_unit(tc.cl(x).to(DEV), w.to(DEV), **strides(case))
    report(case["id"], *tc.gate(tc.uncl(out.cpu()), ref, S, n))


@pytest.mark.parametrize("case", tc.dgrad_cases(), ids=lambda c: c["id"])
def test_dgrad_unit(case):
    """The conv grid, each case with a named variant (upstream mask, added tensor, its mask); both stem maps in both output layouts.  The
    bound's chain length is per position: the taps of its parity class times Cout."""
    _, w, g, act = tc.conv_case_inputs(case)
    stem, frames = case["cin"] == 3, case["frames"]
    in_shape = (case["batch"], case["cin"]) + tuple(case["thw"])
    add = tc.randn(case["seed"] + 4, in_shape) if case["add"] else None
    add_mask = tc.randn(case["seed"] + 5, in_shape) if case["add_mask"] else None
    ref, S, n = tc.dgrad_oracle(g, w, act if case["act"] else None, case["thw"], case["st"], case["ss"], add, add_mask)
    assert tuple(n.shape[2:]) == tuple(case["thw"]) and (case["st"] == case["ss"] == 1 or stem or float(n.min()) < float(n.max()) or min(case["thw"]) == 1)
    out = i2v_native.disc3d_dgrad_unit(tc.cl(g).to(DEV), w.to(DEV), case["thw"], tc.cl(act).to(DEV) if case["act"] else None,
                                       None if add is None else tc.cl(add).to(DEV), None if add_mask is None else tc.cl(add_mask).to(DEV),
                                       frames=frames, **strides(case)).cpu()
    if not frames:
        if stem:
            assert float(out[..., 3].abs().max()) == 0.0
            out = out[..., :3]
        out = tc.uncl(out)
    report(case["id"], *tc.gate(out, ref, S, n))


@pytest.mark.parametrize("case", tc.big_cases(), ids=lambda c: c["id"])
def test_large_maps_take_the_128_row_tile(case):
    """One case past the threshold of the 128-row tile per GEMM kernel (the only tile-size threshold of the launch code), ragged tail."""
    t, h, w_ = case["thw"]
    x, w, g, act = tc.conv_case_inputs(case)
    if case["kind"] == "conv":
        assert tc.rows_per_workgroup(int(np.prod(g.shape[2:])), 1) == 128 and int(np.prod(g.shape[2:])) % 128
        ref, S, n = tc.conv_oracle(x, w, case["st"], case["ss"])
        out = i2v_native.disc3d_conv_unit(tc.cl(x).to(DEV), w.to(DEV), **strides(case))
        report(case["id"], *tc.gate(tc.uncl(out.cpu()), ref, S, n))
    else:
        st, ss = case["st"], case["ss"]
        largest = -(-t // st) * -(-h // ss) * -(-w_ // ss)
        assert tc.rows_per_workgroup(largest * st * ss * ss, 1) == 128 and largest % 128
        ref, S, n = tc.dgrad_oracle(g, w, act, case["thw"], st, ss)
        out = i2v_native.disc3d_dgrad_unit(tc.cl(g).to(DEV), w.to(DEV), case["thw"], tc.cl(act).to(DEV), **strides(case)).cpu()
        report(case["id"], *tc.gate(tc.uncl(out), ref, S, n))


@pytest.mark.parametrize("case", tc.wgrad_cases(), ids=lambda c: c["id"])
def test_wgrad_unit(case):
    """1, 2 and 3 slices with ragged last slices; projection on and off; accumulate on and off."""
    x, w, g, act = tc.conv_case_inputs(case)
    p = g.shape[0] * int(np.prod(g.shape[2:]))
    assert i2v_native.disc3d_wgrad_plan(case["cout"], case["cin"], p, taps=w[0, 0].numel())[0] == case["slices"]
    u0, v0 = tc.randn(case["seed"] + 6, (w.shape[0],)).double(), tc.randn(case["seed"] + 7, (w[0].numel(),)).double()
    u, v, sigma = tc.power_iteration(w.double().reshape(w.shape[0], -1), u0 / u0.norm(), v0 / v0.norm())
    for project in (False, True):
        sn = (u.float(), v.float(), sigma.float()) if project else (None, None, None)   # the kernel projects with the fp32 u, v, sigma it is given
        ref, bound = tc.wgrad_oracle(g, x, w, act, case["st"], case["ss"], *sn)
        args = dict(act=tc.cl(act).to(DEV), **strides(case))
        if project:
            args.update(u=sn[0].to(DEV), v=sn[1].to(DEV), sigma=sn[2].reshape(1).to(DEV))
        dw = i2v_native.disc3d_wgrad_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), w.to(DEV), **args)
        report(f"{case['id']} project{int(project)}", *tc.gate_bound(dw.cpu(), ref, bound))
        prior = tc.randn(case["seed"] + 8, tuple(w.shape)).to(DEV)
        acc = i2v_native.disc3d_wgrad_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), w.to(DEV), dweight=prior.clone(), **args)
        assert torch.equal(acc, prior + dw), "accumulate is not write-then-add"


@pytest.mark.parametrize("case", tc.conv_cases() + tc.STEM_CASES, ids=lambda c: c["id"])
def test_wgrad_unit_on_the_conv_grid(case):
    """The weight gradient on the grid of the forward and the input gradient (every channel pair, stride pair and map, both batch sizes, a
    single frame under temporal stride 2, both stem maps), with the upstream mask, projection off and on."""
    x, w, g, act = tc.conv_case_inputs(case)
    u0, v0 = tc.randn(case["seed"] + 6, (w.shape[0],)).double(), tc.randn(case["seed"] + 7, (w[0].numel(),)).double()
    u, v, sigma = tc.power_iteration(w.double().reshape(w.shape[0], -1), u0 / u0.norm(), v0 / v0.norm())
    for project in (False, True):
        sn = (u.float(), v.float(), sigma.float()) if project else (None, None, None)
        ref, bound = tc.wgrad_oracle(g, x, w, act, case["st"], case["ss"], *sn)
        args = dict(act=tc.cl(act).to(DEV), **strides(case))
        if project:
            args.update(u=sn[0].to(DEV), v=sn[1].to(DEV), sigma=sn[2].reshape(1).to(DEV))
        dw = i2v_native.disc3d_wgrad_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), w.to(DEV), **args)
        report(f"{case['id']} grid project{int(project)}", *tc.gate_bound(dw.cpu(), ref, bound))


GN_CASES = [{"id": f"gn-c{c}-{'x'.join(map(str, thw))}-b{b}-res{int(res)}-relu{int(relu)}", "c": c, "thw": thw, "batch": b, "res": res, "relu": relu,
             "seed": 55000 + 10 * i}
            for i, (c, thw, b, res, relu) in enumerate(((16, (1, 4, 4), 1, False, False), (48, (3, 5, 7), 2, True, True), (64, (2, 8, 8), 3, False, True),
                                                        (48, (1, 5, 7), 1, True, False), (16, (12, 32, 32), 2, False, True)))]


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c["id"])
def test_groupnorm_units(case):
    """Forward and backward, C / 16 = 1, 3 and 4 channels per group, one group with all values equal, statistics over one and several slices."""
    c, b = case["c"], case["batch"]
    shape = (b, c) + case["thw"]
    x = tc.randn(case["seed"], shape) * 2 + 0.5
    cpg = c // 16
    x[0, cpg: 2 * cpg] = 0.75                                                  # group 1 of sample 0: all equal
    w, bias = 1 + 0.3 * tc.randn(case["seed"] + 1, (c,)), 0.2 * tc.randn(case["seed"] + 2, (c,))
    res = tc.randn(case["seed"] + 3, shape) if case["res"] else None
    g = tc.randn(case["seed"] + 4, shape)
    y64, xhat, rstd = tc.group_norm(x.double(), w.double(), bias.double())
    S = (xhat * w.double().view(1, -1, 1, 1, 1)).abs() + bias.double().abs().view(1, -1, 1, 1, 1)
    if res is not None:
        y64, S = y64 + res.double(), S + res.double().abs()
    out64 = torch.relu(y64) if case["relu"] else y64
    out, stats = i2v_native.disc3d_groupnorm_unit(tc.cl(x).to(DEV), w.to(DEV), bias.to(DEV), None if res is None else tc.cl(res).to(DEV), relu=case["relu"])
    report(case["id"] + " fwd", *tc.gate(tc.uncl(out.cpu()), out64, S, 3))
    assert float(tc.uncl(out.cpu())[0, cpg: 2 * cpg].sub(out64[0, cpg: 2 * cpg].float()).abs().max()) < 1e-6
    assert rel(stats[..., 1].cpu(), rstd) < 1e-9
    # backward with the GPU's own mask (a sign flip of an output within rounding of 0 is the forward's matter)
    mask = tc.uncl(out.cpu()) > 0 if case["relu"] else None
    dy = g.double() if mask is None else g.double() * mask
    dx64, dw64, db64 = tc.group_norm_backward(dy, xhat, rstd, w.double())
    dyw = (dy * w.double().view(1, -1, 1, 1, 1)).reshape(b, 16, -1)
    m = dyw.shape[2]
    s1, s2 = dyw.sum(2, keepdim=True).abs(), (dyw * xhat.reshape(b, 16, -1)).sum(2, keepdim=True).abs()
    Sx = (rstd.reshape(b, 16, 1) * (dyw.abs() + s1 / m + xhat.reshape(b, 16, -1).abs() * s2 / m)).reshape(shape)
    dx, dw, db = i2v_native.disc3d_groupnorm_backward_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), stats, w.to(DEV), mask=out if case["relu"] else None)
    report(case["id"] + " dx", *tc.gate(tc.uncl(dx.cpu()), dx64, Sx, 2))
    report(case["id"] + " dweight", *tc.gate(dw.cpu()[None], dw64[None], dw64.abs()[None], 1))
    report(case["id"] + " dbias", *tc.gate(db.cpu()[None], db64[None], db64.abs()[None], 1))
    pw, pb = tc.randn(case["seed"] + 5, (c,)).to(DEV), tc.randn(case["seed"] + 6, (c,)).to(DEV)
    _, aw, ab = i2v_native.disc3d_groupnorm_backward_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), stats, w.to(DEV), mask=out if case["relu"] else None,
                                                          dweight=pw.clone(), dbias=pb.clone())
    assert torch.equal(aw, pw + dw) and torch.equal(ab, pb + db)


@pytest.mark.parametrize("thw", ((3, 6, 6), (1, 5, 7)), ids=lambda s: "x".join(map(str, s)))
def test_maxpool_units(thw):
    """Bit for bit against torch's MaxPool3d, a window of tied values resolved to the first in (t, h, w) scan order; the backward gathers."""
    x = tc.randn(56000 + thw[0], (2, 16) + thw)
    x[0, 0, :, 0:3, 0:3] = 5.0                       # ties: the window of output (t, 0, 0) and its neighbours
    ref, idx = F.max_pool3d(x, 3, (1, 2, 2), 1, return_indices=True)
    out, arg = i2v_native.disc3d_maxpool_unit(tc.cl(x).to(DEV))
    assert torch.equal(tc.uncl(out.cpu()), ref)
    assert torch.equal(tc.uncl(arg.cpu()).long(), idx)
    assert int(tc.uncl(arg.cpu())[0, 0, 0, 0, 0]) == 0 and int(tc.uncl(arg.cpu())[0, 0, -1, 0, 0]) == (max(thw[0] - 2, 0)) * thw[1] * thw[2]
    g = tc.randn(56100 + thw[0], tuple(ref.shape))
    flat = lambda t: t.reshape(2, 16, -1)
    dx64 = torch.zeros(2, 16, int(np.prod(thw)), dtype=torch.float64).scatter_add_(2, flat(idx), flat(g.double())).reshape(x.shape)
    S = torch.zeros(2, 16, int(np.prod(thw)), dtype=torch.float64).scatter_add_(2, flat(idx), flat(g.double().abs())).reshape(x.shape)
    dx = i2v_native.disc3d_maxpool_backward_unit(tc.cl(g).to(DEV), arg, tuple(tc.cl(x).shape))
    report(f"maxpool-bwd {thw}", *tc.gate(tc.uncl(dx.cpu()), dx64, S, 12))


@pytest.mark.parametrize("c,b", ((32, 1), (48, 3), (512, 2)))
def test_head_unit(c, b):
    x, w, g = tc.randn(57000 + c, (b, c, 1, 4, 4)), tc.randn(57001 + c, (1, c)) * float(c ** -0.5), tc.randn(57002 + c, (b, 1))
    pooled = x.double().mean((2, 3, 4))
    pred64, S = pooled @ w.double().t(), pooled.abs() @ w.double().abs().t()
    pred, dx, dw = i2v_native.disc3d_head_unit(tc.cl(x).to(DEV), w.to(DEV), g.to(DEV))
    report(f"head-c{c} pred", *tc.gate(pred.cpu(), pred64, S, 17))
    dx64 = (g.double() @ w.double() / 16).view(b, c, 1, 1, 1).expand(x.shape)
    report(f"head-c{c} dx", *tc.gate(tc.uncl(dx.cpu()), dx64, dx64.abs(), 2))
    report(f"head-c{c} dweight", *tc.gate(dw.cpu(), g.double().t() @ pooled, g.double().abs().t() @ x.double().abs().mean((2, 3, 4)), 17))
    assert torch.equal(i2v_native.disc3d_head_unit(tc.cl(x).to(DEV), w.to(DEV)), pred)


@pytest.mark.parametrize("metric", ("L1", "L2"))
def test_fmap_loss_unit(metric):
    shapes = [(2, 6, 16, 16, 16), (2, 3, 16, 16, 16), (2, 2, 8, 8, 32), (2, 1, 4, 4, 32)]
    a = [tc.randn(58000 + i, s) for i, s in enumerate(shapes)]
    b = [tc.randn(58010 + i, s) for i, s in enumerate(shapes)]
    for x, y in zip(a, b):
        x.view(-1)[::7] = y.view(-1)[::7]                # exact zero differences: sign(0) = 0
    d32 = [(x - y).double() for x, y in zip(a, b)]       # the kernel subtracts in fp32, then sums in float64
    loss64, grads64 = tc.fmap_loss_oracle(d32, [torch.zeros_like(d) for d in d32], metric)
    out, grads = i2v_native.disc3d_fmap_loss([t.to(DEV) for t in a], [t.to(DEV) for t in b], metric, grad_scale=10.0)
    assert abs(float(out[0]) / float(loss64) - 1) < 1e-12
    for i, (gq, gr) in enumerate(zip(grads, grads64)):
        assert float(gq.view(-1)[::7].abs().max()) == 0.0
        report(f"fmap-{metric} d_a[{i}]", *tc.gate(gq.cpu(), 10.0 * gr, (10.0 * gr).abs(), 3))
    one, _ = i2v_native.disc3d_fmap_loss([a[0].to(DEV)], [b[0].to(DEV)], metric, need_grads=False)
    assert abs(float(one[0]) - float(out[1])) < 1e-15


def test_sum_of_squares_unit():
    x = tc.randn(59000, (3, 3, 5, 33, 31))
    out = i2v_native.disc3d_sumsq(x.to(DEV))
    assert out.dtype == torch.float64 and rel(out, x.double().pow(2).reshape(3, -1).sum(1)) < 1e-13


# ---------------------------------------------------------------------------------------------------------------- module against the fixtures

def check(name, got, want, rows=True):
    r = rel_rows(got, want) if rows else rel(got, want)
    print(f"  {name}: rel-L2 {r:.2e}")
    assert r <= tc.TOL_L2, (name, r)
    return r


def test_fixture_a_training_step(fxa):
    """The training forwards and the 'disc' hinge backward through the autograd path, against the reference's own module."""
    main, sd, grads = fxa
    net = module(tc.CFG_A, sd).train()
    fake, real = (t.to(DEV).requires_grad_(True) for t in tc.clips_a())
    (pf, ff), (pr, fr) = net(fake), net(real)
    assert pf.grad_fn is not None and all(f.grad_fn is not None and f.shape[1] == c for f, c in zip(ff, tc.CFG_A["channels"][1:]))
    loss = tc.hinge_disc(pf, pr)
    loss.backward()
    check("pred fake", pf.detach().T, main["train_pred_fake"].T)
    check("pred real", pr.detach().T, main["train_pred_real"].T)
    assert abs(float(loss.detach()) - float(main["train_loss"])) < 1e-5
    for name, fm in (("fake", ff), ("real", fr)):
        sums = np.array([[float(f.detach().double().sum()), float(f.detach().double().pow(2).sum())] for f in fm])
        print("  fmap checksums (sum, sum of squares) rel:", np.abs(sums / main["train_fmaps_" + name] - 1).max(0))
        assert np.allclose(sums, main["train_fmaps_" + name], rtol=1e-4, atol=0)          # the maps are post-ReLU: both sums are positive
        check(f"fmap3 {name}", fm[3].detach(), main["train_fmap3_" + name])
    for k, v in net.state_dict().items():
        if k.endswith(("weight_u", "weight_v")):
            check("after " + k, v, main["after." + k], rows=False)
    worst = max(check("grad " + k, p.grad, grads[k], rows=False) for k, p in net.named_parameters())
    print(f"  worst parameter gradient: {worst:.2e}")
    check("dx fake", fake.grad, load_dx("fake"))
    check("dx real", real.grad, load_dx("real"))


def test_fixture_a_eval_mode_leaves_u_and_v(fxa):
    main, sd, _ = fxa
    net = module(tc.CFG_A, sd, {k[6:]: v for k, v in main.items() if k.startswith("after.")}).eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        for t in (12, 5):
            pred, fmaps = net(tc.clips_a_eval(t).to(DEV))
            check(f"eval T={t}", pred.T, main[f"eval_t{t}"].T)
            assert pred.grad_fn is None and len(fmaps) == 4
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


def test_fixtures_b_and_c(fxb):
    main, grads = fxb
    net = module(tc.CFG_B, tc.synthetic_state(tc.CFG_B, tc.SEED_B)).train()
    x = tc.clips_b().to(DEV).requires_grad_(True)
    d_pred, d_fmaps = tc.upstream_b()
    pred, fmaps = net(x)
    ((pred * d_pred.to(DEV)).sum() + sum((f * g.to(DEV)).sum() for f, g in zip(fmaps, d_fmaps))).backward()
    check("B pred", pred.detach().T, main["b_pred"].T)
    for i, f in enumerate(fmaps):
        check(f"B fmap{i}", f.detach(), main[f"b_fmap{i}"])
    check("B dx", x.grad, main["b_dx"])
    worst = max(check("B grad " + k, p.grad, grads[k], rows=False) for k, p in net.named_parameters())
    print(f"  worst parameter gradient: {worst:.2e}")
    netc = module(tc.CFG_C, tc.synthetic_state(tc.CFG_C, tc.SEED_B)).train()
    with torch.no_grad():
        pred, fmaps = netc(tc.clips_c().to(DEV))
    check("C pred", pred.T, main["c_pred"].T)
    for i, f in enumerate(fmaps):
        check(f"C fmap{i}", f, main[f"c_fmap{i}"])


def test_refusal_names_the_final_map(fxa):
    net = module(tc.CFG_A, fxa[1])
    with pytest.raises(i2v_native.I2VError, match=r"\[1, 2, 2\]"):
        net(torch.zeros(1, 3, 12, 32, 32, device=DEV))
    h = net._handle()
    assert h.out_shape(12, 64, 64) == [(6, 16, 16, 16), (3, 16, 16, 16), (2, 8, 8, 32), (1, 4, 4, 32)]
    for t in range(1, 17):
        assert h.out_shape(t, 64, 64)[3][:3] == (1, 4, 4)
    big = i2v_native.NativeDisc3D([16, 16, 16, 32, 32], [1, 2, 2, 2], [2, 2, 2, 2], device=DEV)
    assert big.out_shape(12, 128, 128)[3][:3] == (1, 4, 4)


@pytest.mark.parametrize("cfg,clips", ((tc.CFG_A, lambda: tc.clips_a()[0]), (tc.CFG_B, tc.clips_b), (tc.CFG_C, tc.clips_c)), ids=("A", "B", "C-no-pool"))
def test_saved_layout_is_consistent(cfg, clips):
    """The entries of ``saved_maps``: inside ``saved``, on 256-byte offsets, disjoint, two per conv plus the pool's two; the last conv's
    activation is the fourth feature map; the workspace holds a forward that does not save."""
    net = module(cfg, tc.synthetic_state(cfg, tc.SEED_B)).eval()
    x = clips().to(DEV)
    n, _, t, hh, w = shape = tuple(x.shape)
    _, fmaps, saved = net._run(x, save=True)
    h = net._handle()
    assert saved.numel() == h.saved_bytes(n, t, hh, w) <= h.workspace_bytes(n, t, hh, w)
    maps = h.saved_maps(saved, shape)
    nconv = 1 + sum(3 if b["ds"] else 2 for b in tc.blocks(cfg))
    assert len(maps) == 2 * nconv + (2 if cfg["use_max_pool"] else 0)
    spans = sorted((m.data_ptr() - saved.data_ptr(), m.data_ptr() - saved.data_ptr() + m.numel() * m.element_size()) for m in maps.values())
    assert all(a % 256 == 0 and 0 <= a < b <= saved.numel() for a, b in spans)
    assert all(p[1] <= q[0] for p, q in zip(spans, spans[1:]))          # sorted by their starts: no two overlap
    assert torch.equal(maps[(i2v_native.DISC3D_ACT, nconv - 1)], fmaps[3])


# ---------------------------------------------------------------------------------------------------------------- oracle on the GPU's decisions

def gpu_decisions(handle, saved, shape, cfg):
    """The ReLU masks and the pool's argmax of a saved forward, keyed as the oracle keys them."""
    maps = handle.saved_maps(saved, shape)
    names, i = {0: "norm1"}, 1
    for b in tc.blocks(cfg):
        names[i], names[i + 1] = b["prefix"] + "bn1", b["prefix"] + "bn2"
        i += 3 if b["ds"] else 2
    dec = {name: tc.uncl(maps[(i2v_native.DISC3D_ACT, ci)]).cpu() > 0 for ci, name in names.items()}
    if cfg["use_max_pool"]:
        dec["pool"] = tc.uncl(maps[(i2v_native.DISC3D_POOL_ARGMAX, -1)]).cpu().long().contiguous()
    return dec


def against_oracle(name, cfg, sd, x, d_pred, d_fmaps):
    """One saved training forward and one backward through the entries against the oracle run on the GPU's decisions."""
    net = module(cfg, sd).train()
    grads = {k: torch.zeros_like(p) for k, p in net.named_parameters()}
    pred, fmaps, saved = net._run(x.to(DEV), save=True, grads=grads)
    shape = tuple(x.shape)
    h = net._handle(grads)
    cl = None if d_fmaps is None else [tc.cl(g).to(DEV) for g in d_fmaps]
    dx = h.backward(d_pred.to(DEV), cl, saved, shape, need_dx=True, param_grads=True, accumulate=False)
    dec = gpu_decisions(h, saved, shape, cfg)
    _, _, own = tc.forward_oracle(sd, x, cfg, training=True)
    rep = tc.decision_report(dec, own)
    print(f"  {name}: decisions that differ from float64's (all, outside the band):", {k: v for k, v in rep.items() if v[0]})
    assert sum(v[1] for v in rep.values()) == 0 and sum(v[0] for v in rep.values()) <= tc.FRAGILE_MAX, rep
    p64, f64, c = tc.forward_oracle(sd, x, cfg, training=True, decisions=dec)
    g64, dx64 = tc.backward_oracle(c, d_pred, d_fmaps)
    # every conv's raw output, before its GroupNorm: the one place of the module where a conv's scale (W / sigma or W) shows
    maps, convs = h.saved_maps(saved, shape), [c["stem"]]
    for st in c["steps"]:
        convs += [st["c1"], st["c2"]] + ([st["cd"]] if st["cd"] is not None else [])
    raw = max(rel_rows(tc.uncl(maps[(i2v_native.DISC3D_CONV_OUT, ci)]), cv["y"]) for ci, cv in enumerate(convs))
    print(f"  {name}: worst rel-L2 of the {len(convs)} raw conv outputs {raw:.2e}")
    assert raw <= tc.TOL_L2, raw
    worst = max([check(f"{name} pred", pred.T, p64.T), check(f"{name} dx", dx, dx64)] + [check(f"{name} fmap{i}", tc.uncl(f), q) for i, (f, q) in enumerate(zip(fmaps, f64))]
                + [rel(grads[k], g64[k]) for k in g64])
    for k in g64:
        assert rel(grads[k], g64[k]) <= tc.TOL_L2, (k, rel(grads[k], g64[k]))
    for k, v in c["state"].items():
        assert rel(net.state_dict()[k], v) < 1e-6, k
    print(f"  {name}: worst rel-L2 over outputs, input gradient and {len(g64)} parameter gradients {worst:.2e}")


def test_oracle_on_the_gpus_decisions_fixture_a(fxa):
    fake, _ = tc.clips_a()
    d_fmaps = [tc.randn(60000 + i, s) * 0.01 for i, s in enumerate(((2, 16, 6, 16, 16), (2, 16, 3, 16, 16), (2, 32, 2, 8, 8), (2, 32, 1, 4, 4)))]
    against_oracle("A", tc.CFG_A, fxa[1], fake, torch.tensor([[0.5], [-0.25]]), d_fmaps)


def test_oracle_on_the_gpus_decisions_fixture_b():
    d_pred, d_fmaps = tc.upstream_b()
    against_oracle("B", tc.CFG_B, tc.synthetic_state(tc.CFG_B, tc.SEED_B), tc.clips_b(), d_pred, d_fmaps)


def test_oracle_on_the_gpus_decisions_without_the_pool():
    """use_max_pool False is the same plan minus one step: its backward too (fixture C's net; the maps are fixture B's)."""
    d_pred, d_fmaps = tc.upstream_b()
    against_oracle("C", tc.CFG_C, tc.synthetic_state(tc.CFG_C, tc.SEED_B), tc.clips_c(), d_pred, d_fmaps)


def test_shipped_widths_against_the_oracle():
    """[64, 64, 128, 256, 512] at B = 1, 64 x 64: every layer at its width, the 64-column GEMM forms, T 12 -> 6 -> 3 -> 2 -> 1."""
    sd = tc.synthetic_state(tc.CFG_SHIPPED, 6100)
    against_oracle("shipped", tc.CFG_SHIPPED, sd, tc.randn(6101, (1, 3, SHIPPED_T, 64, 64)), torch.tensor([[1.0]]), None)


# ---------------------------------------------------------------------------------------------------------------- bit-level properties

def test_two_runs_give_the_same_bits_and_accumulate_is_write_then_add():
    sd = tc.synthetic_state(tc.CFG_B, tc.SEED_B)
    d_pred, d_fmaps = tc.upstream_b()
    cl = [tc.cl(g).to(DEV) for g in d_fmaps]
    x = tc.clips_b().to(DEV)
    runs = []
    for _ in range(2):
        net = module(tc.CFG_B, sd).train()
        grads = {k: torch.zeros_like(p) for k, p in net.named_parameters()}
        pred, fmaps, saved = net._run(x, save=True, grads=grads)
        dx = net._handle(grads).backward(d_pred.to(DEV), cl, saved, tuple(x.shape), accumulate=False)
        runs.append((pred, fmaps, dx, grads, net, saved))
    (p0, f0, dx0, g0, net, saved), (p1, f1, dx1, g1, _, _) = runs
    assert torch.equal(p0, p1) and torch.equal(dx0, dx1) and all(torch.equal(a, b) for a, b in zip(f0, f1))
    assert all(torch.equal(g0[k], g1[k]) for k in g0)
    prior = {k: tc.randn(61000 + i, tuple(v.shape)).to(DEV) for i, (k, v) in enumerate(g0.items())}
    acc = {k: v.clone() for k, v in prior.items()}
    dx2 = net._handle(acc).backward(d_pred.to(DEV), cl, saved, tuple(x.shape), accumulate=True)
    assert torch.equal(dx2, dx0) and all(torch.equal(acc[k], prior[k] + g0[k]) for k in g0)


def test_autograd_path_equals_the_backward_entry_and_refuses_a_second_order_graph():
    sd = tc.synthetic_state(tc.CFG_B, tc.SEED_B)
    d_pred, d_fmaps = tc.upstream_b()
    x = tc.clips_b().to(DEV)
    net = module(tc.CFG_B, sd).train()
    grads = {k: torch.zeros_like(p) for k, p in net.named_parameters()}
    pred, fmaps, saved = net._run(x, save=True, grads=grads)
    dx = net._handle(grads).backward(d_pred.to(DEV), [tc.cl(g).to(DEV) for g in d_fmaps], saved, tuple(x.shape))
    twin = module(tc.CFG_B, sd).train()
    xa = x.clone().requires_grad_(True)
    pa, fa = twin(xa)
    ((pa * d_pred.to(DEV)).sum() + sum((f * g.to(DEV)).sum() for f, g in zip(fa, d_fmaps))).backward()
    assert torch.equal(pa.detach(), pred) and torch.equal(xa.grad, dx)
    assert all(torch.equal(p.grad, grads[k]) for k, p in twin.named_parameters())
    # a frozen module: no parameter gradient, the same input gradient
    for p in twin.parameters():
        p.requires_grad_(False)
    twin.load_state_dict(sd)
    xb = x.clone().requires_grad_(True)
    pb, fb = twin(xb)
    ((pb * d_pred.to(DEV)).sum() + sum((f * g.to(DEV)).sum() for f, g in zip(fb, d_fmaps))).backward()
    assert torch.equal(xb.grad, dx)
    xc = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(twin(xc)[0].mean(), xc, create_graph=True)


# ---------------------------------------------------------------------------------------------------------------- trainer

def test_trainer_step_follows_the_references_six_sgd_steps(fxa):
    """TemporalDiscTrainer.step with plain SGD in place of the fused Adam against the reference's float64 loss sequence; the bound per step
    is 4 x |reference in fp32 - reference in float64| (the reference's own fp32 run sets the scale; the factor covers another summation
    order), floor 1e-6."""
    main, sd, _ = fxa
    net = module(tc.CFG_A, sd).train()
    tr = i2v_train.TemporalDiscTrainer(net, optimizer=torch.optim.SGD(net.parameters(), lr=tc.SGD_LR))
    fake, real = (t.to(DEV) for t in tc.clips_a())
    losses = [tr.step(fake, real)[0] for _ in range(tc.SGD_STEPS)]
    losses = np.array([float(v) for v in losses])
    bound = np.maximum(4 * np.abs(main["sgd_losses_f32"] - main["sgd_losses"]), 1e-6)
    diff = np.abs(losses - main["sgd_losses"])
    print("  losses:", [f"{v:.6f}" for v in losses])
    print("  |gpu - f64|:", [f"{v:.2e}" for v in diff], " bound:", [f"{v:.2e}" for v in bound])
    assert np.all(diff <= bound), (diff, bound)


def test_fused_adam_trainer_five_steps(fxa):
    net = module(tc.CFG_A, fxa[1]).train()
    tr = i2v_train.TemporalDiscTrainer(net)
    fake, real = (t.to(DEV) for t in tc.clips_a())
    out = [tr.step(fake.transpose(1, 2), real.transpose(1, 2)) for _ in range(5)]      # [B, T, 3, H, W], as the step holds its clips
    losses = [float(o[0]) for o in out]
    print("  losses:", [f"{v:.6f}" for v in losses])
    assert losses[-1] < losses[0] and all(torch.isfinite(p).all() for p in net.parameters())
    assert out[0][1].dtype == torch.float64 and out[0][1].dim() == 0


def test_generator_loss_and_gradient_penalty_match_the_fixture(fxa):
    main, sd, _ = fxa
    fake, real = (t.to(DEV) for t in tc.clips_a())
    net = module(tc.CFG_A, sd).train()
    tr = i2v_train.TemporalDiscTrainer(net)
    for p in net.parameters():
        p.grad = torch.full_like(p, 3.0)
    (coup, fm, total), dx = tr.generator_loss(fake, real)
    print(f"  coup_t {float(coup):.6f} ({main['gen_coup']:.6f})  L_fmap_t {float(fm):.6f} ({main['gen_fmap']:.6f})")
    assert abs(float(coup) - main["gen_coup"]) < 1e-5 and abs(float(fm) / main["gen_fmap"] - 1) < 1e-4 and abs(float(total) / main["gen_loss"] - 1) < 1e-4
    check("generator dx", dx, load_dx("gen"))
    assert all(bool((p.grad == 3.0).all()) for p in net.parameters())                  # .grad is left untouched
    tr2 = i2v_train.TemporalDiscTrainer(module(tc.CFG_A, sd).train())
    gp = tr2.gradient_penalty(real)
    print(f"  L_GP {float(gp):.6e} ({main['gp_value']:.6e})")
    assert gp.dtype == torch.float64 and abs(float(gp) / main["gp_value"] - 1) < 2e-4   # a squared norm: twice the gate's relative error
    with pytest.raises(NotImplementedError, match="double backward"):
        i2v_train.TemporalDiscTrainer(net, w_GP=10)
