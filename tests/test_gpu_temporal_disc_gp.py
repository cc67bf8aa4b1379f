"""GPU checks of the gradient penalty's gradient on the temporal discriminator (csrc/i2v_res3d_gp.h, include/i2v_hip_disc3d_gp.h,
``NativeDisc3D.gp_backward``, ``Discriminator.forward_with_penalty``, ``i2v_train.TemporalDiscPenaltyTrainer``): the new kernels against
float64 at the derived bounds of tests/temporal_disc_gp_common.py, the module's tangent maps and penalty gradients against the hand-written
float64 oracle on the GPU's own decisions and against the fixtures made from the reference's module (tests/golden/disc3d_gp_*.npz), the
bit-level properties, the autograd surface and the trainer.  Run with ``-s`` to see the figures of profiles/temporal_disc_gp_gate.md."""
import glob
import os

import numpy as np
import pytest
import torch

import i2v_native
import i2v_train
import temporal_disc_common as tc
import temporal_disc_gp_common as gp
from stage1_VAE.modules import loss as loss_mod
from stage1_VAE.modules.resnet3D import Discriminator

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZERO_KEY = "layer.3.1.bn2.bias"


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


def case(name):
    """-> (cfg, state dict, clips) of fixture ``name``"""
    if name == "a":
        return tc.CFG_A, {k: torch.from_numpy(v) for k, v in load("temporal_disc_a_params*.npz").items()}, tc.clips_a()[1]
    cfg = tc.CFG_B if name == "b" else tc.CFG_C
    return cfg, tc.synthetic_state(cfg, tc.SEED_B), (tc.clips_b if name == "b" else tc.clips_c)()


def module(cfg, sd):
    net = Discriminator(dict(cfg))
    net.load_state_dict(dict(sd))
    return net.to(DEV)


def report(name, ok, ratio, l2):
    print(f"  {name}: |err|/bound {ratio:.3f}  rel-L2 {l2:.2e}")
    assert ok, (name, ratio, l2)


def zero_grads(net):
    return {k: torch.zeros_like(p) for k, p in net.named_parameters()}


def run_penalty(name, scale=1.0, scale_dev=None, grads=None, accumulate=False):
    """A fresh module in training mode, one saved forward on the fixture's clips, gp_backward -> (net, handle, saved, shape, grads, l_gp, gp_saved)"""
    cfg, sd, x = case(name)
    net = module(cfg, sd).train()
    grads = zero_grads(net) if grads is None else grads
    _, _, saved = net._run(x.to(DEV), save=True, grads=grads, want_fmaps=False)
    h = net._handle(grads)
    l_gp, gsv = h.gp_backward(saved, tuple(x.shape), scale=scale, scale_dev=scale_dev, accumulate=accumulate)
    return net, h, saved, tuple(x.shape), grads, l_gp, gsv


@pytest.fixture(scope="module")
def runs():
    """gp_backward at scale 1 on the three fixtures, once for the tests that only read it"""
    return {n: run_penalty(n) for n in "abc"}


# ---------------------------------------------------------------------------------------------------------------- units

@pytest.mark.parametrize("full", (False, True), ids=("plain", "mask-res"))
@pytest.mark.parametrize("c", gp.GN_CASES, ids=lambda c: c["id"])
def test_groupnorm_tangent_unit(c, full):
    x, xd, resd, act, _, _, w, b = gp.gn_case_inputs(c)
    out0, stats = i2v_native.disc3d_groupnorm_unit(tc.cl(x).to(DEV), w.to(DEV), b.to(DEV))
    mask = (act > 0) if full else None
    ref, bound, M, C = gp.gn_tangent_oracle(x, xd, w, resd if full else None, mask)
    out, tstats = i2v_native.disc3d_gp_groupnorm_tangent_unit(tc.cl(x).to(DEV), tc.cl(xd).to(DEV), stats, w.to(DEV), tc.cl(resd).to(DEV) if full else None,
                                                              tc.cl(act).to(DEV) if full else None)
    report(c["id"], *tc.gate_bound(tc.uncl(out.cpu()), ref, bound))
    scale = xd.double().abs().mean()
    assert float((tstats.cpu()[..., 0] - M).abs().max()) <= 1e-12 * scale and float((tstats.cpu()[..., 1] - C).abs().max()) <= 1e-12 * scale * 4
    if full:
        assert float(tc.uncl(out.cpu())[~mask].abs().max()) == 0.0


@pytest.mark.parametrize("full", (False, True), ids=("plain", "mask"))
@pytest.mark.parametrize("c", gp.GN_CASES, ids=lambda c: c["id"])
def test_groupnorm_dual_backward_unit(c, full):
    x, xd, _, act, g, gd, w, b = gp.gn_case_inputs(c)
    xs, xds = tc.cl(x).to(DEV), tc.cl(xd).to(DEV)
    _, stats = i2v_native.disc3d_groupnorm_unit(xs, w.to(DEV), b.to(DEV))
    _, tstats = i2v_native.disc3d_gp_groupnorm_tangent_unit(xs, xds, stats, w.to(DEV))
    mask = (act > 0) if full else None
    want = gp.gn_dual_oracle(g, gd, x, xd, w, mask)
    args = (tc.cl(g).to(DEV), tc.cl(gd).to(DEV), xs, xds, stats, tstats, w.to(DEV))
    dx, dxd, dw, db = i2v_native.disc3d_gp_groupnorm_dual_backward_unit(*args, mask=tc.cl(act).to(DEV) if full else None)
    for name, got in (("dx", tc.uncl(dx.cpu())), ("dxd", tc.uncl(dxd.cpu())), ("dweight", dw.cpu()[None]), ("dbias", db.cpu()[None])):
        ref, bound = want[name]
        report(f"{c['id']} {name}", *tc.gate_bound(got, ref if ref.dim() > 1 else ref[None], bound if bound.dim() > 1 else bound[None]))
    # accumulate adds to what is there, and without parameter gradients the two adjoints keep their bits
    pw, pb = tc.randn(c["seed"] + 8, (c["c"],)).to(DEV), tc.randn(c["seed"] + 9, (c["c"],)).to(DEV)
    aw, ab = pw.clone(), pb.clone()
    dx2, dxd2, _, _ = i2v_native.disc3d_gp_groupnorm_dual_backward_unit(*args, mask=tc.cl(act).to(DEV) if full else None, dweight=aw, dbias=ab)
    assert torch.equal(aw, pw + dw) and torch.equal(ab, pb + db) and torch.equal(dx2, dx) and torch.equal(dxd2, dxd)
    dx3, dxd3, nw, nb = i2v_native.disc3d_gp_groupnorm_dual_backward_unit(*args, mask=tc.cl(act).to(DEV) if full else None, param_grads=False)
    assert nw is None and nb is None and torch.equal(dx3, dx) and torch.equal(dxd3, dxd)


@pytest.mark.parametrize("shape", ((2, 3, 8, 8), (1, 1, 4, 4), (3, 2, 5, 7)), ids=lambda s: "x".join(map(str, s)))
def test_maxpool_tangent_unit_is_a_gather_bit_for_bit(shape):
    n, t, h, w = shape
    x, xd = tc.randn(72000 + h, (n, 16, t, h, w)), tc.randn(72100 + h, (n, 16, t, h, w))
    _, arg = i2v_native.disc3d_maxpool_unit(tc.cl(x).to(DEV))
    out = i2v_native.disc3d_gp_maxpool_tangent_unit(tc.cl(xd).to(DEV), arg)
    want = gp.pool_tangent_oracle(xd, tc.uncl(arg.cpu()).long().contiguous())
    assert torch.equal(tc.uncl(out.cpu()), want)
    _, idx = torch.nn.functional.max_pool3d(x, 3, (1, 2, 2), 1, return_indices=True)
    assert torch.equal(tc.uncl(out.cpu()), gp.pool_tangent_oracle(xd, idx))


@pytest.mark.parametrize("c,n", ((16, 1), (48, 3)))
def test_head_dual_unit(c, n):
    xd, w = tc.randn(73000 + c, (n, c, 1, 4, 4)), tc.randn(73001 + c, (1, c)) * 0.3
    want = gp.head_dual_oracle(xd, w, gp.W_GP)
    pdot, dx, dxd, dw = i2v_native.disc3d_gp_head_dual_unit(tc.cl(xd).to(DEV), w.to(DEV), gp.W_GP)
    assert float(dx.abs().max()) == 0.0
    for name, got in (("pdot", pdot.cpu()), ("dxd", tc.uncl(dxd.cpu())), ("dweight", dw.cpu())):
        report(f"head c{c} {name}", *tc.gate_bound(got, *want[name]))


# ---------------------------------------------------------------------------------------------------------------- module against the oracle

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


def rel_rows(a, b):
    return max(tc.rel_l2_rows(torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()))


@pytest.mark.parametrize("name", ("a", "b", "c"))
def test_tangent_maps_and_gradients_against_the_oracle_on_the_gpus_decisions(name, runs):
    """Every tangent map (through the layout entry) and every parameter's penalty gradient at 1e-4 relative L2 per tensor against the
    hand-written float64 oracle that takes the GPU's ReLU masks and argmaxes; a decision may differ from float64's own only inside the
    fragile band, at most FRAGILE_MAX per case."""
    cfg, sd, x = case(name)
    net, h, saved, shape, grads, l_gp, gsv = runs[name]
    dec = gpu_decisions(h, saved, shape, cfg)
    own = tc.forward_oracle(sd, x, cfg, training=True)[2]
    rep = tc.decision_report(dec, own)
    print(f"  {name}: decisions that differ from float64's (all, outside the band):", {k: v for k, v in rep.items() if v[0]})
    assert sum(v[1] for v in rep.values()) == 0 and sum(v[0] for v in rep.values()) <= tc.FRAGILE_MAX, rep
    o = gp.penalty_oracle(sd, x, cfg, scale=1.0, decisions=dec)
    assert abs(float(l_gp) / float(o["l_gp"]) - 1) < 2e-4            # a squared norm: twice the gate's relative error
    maps = h.gp_saved_maps(gsv, shape)
    convs = [o["cache"]["stem"]]
    for st in o["cache"]["steps"]:
        convs += [st["c1"], st["c2"]] + ([st["cd"]] if st["cd"] is not None else [])
    assert len(maps) == 2 * len(convs) + (2 if cfg["use_max_pool"] else 1)
    xd4 = maps[(i2v_native.DISC3D_GP_INPUT, -1)].cpu()
    assert float(xd4[..., 3].abs().max()) == 0.0
    worst = rel_rows(tc.uncl(xd4[..., :3]), o["xd"])
    for ci, cv in enumerate(convs):
        t = o["T"][cv["key"]]
        worst = max(worst, rel_rows(tc.uncl(maps[(i2v_native.DISC3D_GP_CONV_OUT, ci)]), t["xd"]), rel_rows(tc.uncl(maps[(i2v_native.DISC3D_GP_ACT, ci)]), t["out"]))
    if cfg["use_max_pool"]:
        worst = max(worst, rel_rows(tc.uncl(maps[(i2v_native.DISC3D_GP_POOL_OUT, -1)]), o["T"]["pool"]))
    print(f"  {name}: worst rel-L2 over the tangent clip and the {2 * len(convs)} tangent maps {worst:.2e}")
    assert worst <= tc.TOL_L2, worst
    assert set(o["grads"]) == set(grads)
    figures = {k: gp.rel(grads[k], v) for k, v in o["grads"].items() if k != ZERO_KEY}
    top = max(figures.items(), key=lambda kv: kv[1])
    print(f"  {name}: worst rel-L2 over {len(figures)} parameter gradients {top[1]:.2e} at {top[0]}")
    for k, r in figures.items():
        assert r <= tc.TOL_L2, (name, k, r)
    assert float(grads[ZERO_KEY].abs().max()) == 0.0 and float(o["grads"][ZERO_KEY].abs().max()) == 0.0


@pytest.mark.parametrize("name", ("a", "b", "c"))
def test_gradients_against_the_reference_fixtures(name, runs):
    """Against the reference module's own float64 double backward (its decisions are float64's own).  The gate per tensor comes from the
    fixture, never from the code under test: 1e-4 where the reference's own fp32 run is within 1e-4 / 4 of its float64 run, else four times
    that recorded distance (the rule of gen_train)."""
    main, want = load(f"disc3d_gp_{name}.npz"), load(f"disc3d_gp_{name}_grads*.npz")
    grads, l_gp = runs[name][4], runs[name][5]
    print(f"  {name}: L_GP {float(l_gp):.8e}  reference float64 {float(main['l_gp']):.8e}  reference fp32 {float(main['l_gp_f32']):.8e}")
    assert abs(float(l_gp) / float(main["l_gp"]) - 1) < max(2e-4, 4 * abs(float(main["l_gp_f32"]) / float(main["l_gp"]) - 1))
    assert set(want) == set(grads)
    print(f"  GATE {name} | tensor | reference fp32 vs float64 | gate | GPU vs float64 | ratio")
    worst = 0.0
    for k, v in want.items():
        if k == ZERO_KEY:
            assert float(grads[k].abs().max()) == 0.0 and float(np.abs(v).max()) == 0.0
            continue
        dist = float(main["dist." + k])
        gate = tc.TOL_L2 if dist <= tc.TOL_L2 / 4 else 4 * dist
        r = gp.rel(grads[k], v)
        worst = max(worst, r / gate)
        print(f"  GATE {name} | {k} | {dist:.2e} | {gate:.2e} | {r:.2e} | {r / gate:.3f}")
        assert r <= gate, (name, k, r, gate)
    print(f"  {name}: worst ratio to the gate {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- bit-level properties

def test_l_gp_has_the_bits_of_the_trainers_gradient_penalty(runs):
    cfg, sd, x = case("a")
    l_gp = runs["a"][5]
    tr = i2v_train.TemporalDiscTrainer(module(cfg, sd).train())
    want = tr.gradient_penalty(x.to(DEV))
    assert l_gp.dtype == torch.float64 and l_gp.dim() == 0 and torch.equal(l_gp, want)


def test_two_runs_give_the_same_bits_and_accumulate_adds_to_a_prefilled_grad(runs):
    for name in ("b", "c"):
        _, _, _, _, g0, l0, gsv0 = runs[name]
        net, h, saved, shape, g1, l1, gsv1 = run_penalty(name)
        assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
        m0, m1 = h.gp_saved_maps(gsv0, shape), h.gp_saved_maps(gsv1, shape)
        assert all(torch.equal(m0[k], m1[k]) for k in m0)
        prior = {k: tc.randn(74000 + i, tuple(v.shape)).to(DEV) for i, (k, v) in enumerate(g0.items())}
        acc = {k: v.clone() for k, v in prior.items()}
        l2, _ = net._handle(acc).gp_backward(saved, shape, scale=1.0, accumulate=True)
        assert torch.equal(l2, l0) and all(torch.equal(acc[k], prior[k] + g0[k]) for k in g0)
        assert torch.equal(acc[ZERO_KEY], prior[ZERO_KEY])


def test_scale_is_linear_and_zero_leaves_an_accumulating_grad_unchanged(runs):
    _, _, _, _, g1, l1, _ = runs["b"]
    net, h, saved, shape, g2, l2, _ = run_penalty("b", scale=2.0)
    assert torch.equal(l1, l2)                                            # the value does not depend on the scale
    assert all(torch.equal(g2[k], 2.0 * g1[k]) for k in g1)               # a power of two: exactly
    _, _, _, _, g10, _, _ = run_penalty("b", scale=gp.W_GP)
    for k in g1:
        if k != ZERO_KEY:
            assert gp.rel(g10[k], gp.W_GP * g1[k].double()) <= 1e-5, k
    # the device scalar: 1 x [10] has the bits of the host's 10, 2 x [5] too
    ten = torch.tensor([gp.W_GP], dtype=torch.float32, device=DEV)
    _, _, _, _, gd, _, _ = run_penalty("b", scale=1.0, scale_dev=ten)
    assert all(torch.equal(gd[k], g10[k]) for k in g10)
    _, _, _, _, gd, _, _ = run_penalty("b", scale=2.0, scale_dev=ten / 2)
    assert all(torch.equal(gd[k], g10[k]) for k in g10)
    prior = {k: tc.randn(75000 + i, tuple(v.shape)).to(DEV) for i, (k, v) in enumerate(g1.items())}
    acc = {k: v.clone() for k, v in prior.items()}
    l0, _ = net._handle(acc).gp_backward(saved, shape, scale=0.0, accumulate=True)
    assert torch.equal(l0, l1) and all(torch.equal(acc[k], prior[k]) for k in prior)


def test_refusals_on_the_device(runs):
    net, h, saved, shape, grads, _, _ = runs["c"]
    with pytest.raises(i2v_native.I2VError, match="bytes"):
        h.gp_backward(saved[:-256], shape)
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        h.gp_backward(saved.cpu(), shape)
    with pytest.raises(i2v_native.I2VError, match="gp_saved"):
        h.gp_backward(saved, shape, gp_saved=torch.empty(16, dtype=torch.uint8, device=DEV))
    n, _, t, hh, w = shape
    assert h.gp_saved_bytes(n, t, hh, w) > 0 and h.gp_workspace_bytes(n, t, hh, w) > h.workspace_bytes(n, t, hh, w)
    assert h.gp_saved_bytes(n, t, 2 * hh, w) == 0                        # a shape the network refuses
    bare = i2v_native.NativeDisc3D(device=DEV, **net.cfg)
    i2v_native.bind_in_place(bare, net._tensors())
    with pytest.raises(i2v_native.I2VError, match="gradient tensors"):
        bare.gp_backward(saved, shape)
    with pytest.raises(i2v_native.I2VError, match="gp_backward_dev|null"):
        i2v_native._call("i2v_disc3d_gp_backward_dev", h._h, saved.data_ptr(), saved.numel(), n, t, hh, w, 1.0, None, saved.data_ptr(), saved.numel(),
                         saved.data_ptr(), 0, saved.data_ptr(), saved.numel(), None)


# ---------------------------------------------------------------------------------------------------------------- autograd surface

def test_forward_with_penalty_is_the_forward_plus_the_trainers_gradient():
    cfg, sd, _ = case("a")
    fake, real = (t.to(DEV) for t in tc.clips_a())
    plain = module(cfg, sd).train()
    with torch.no_grad():
        pred0, fmaps0 = plain(real)
    net = module(cfg, sd).train()
    pred, fmaps, l_gp = net.forward_with_penalty(real)
    assert pred.grad_fn is not None and l_gp.grad_fn is pred.grad_fn and all(f.grad_fn is pred.grad_fn for f in fmaps)
    assert torch.equal(pred.detach(), pred0) and all(torch.equal(a.detach(), b) for a, b in zip(fmaps, fmaps0))
    assert l_gp.dtype == torch.float64 and l_gp.dim() == 0
    # loss.py:98-108 on the autograd surface against the trainer's step, both from the same state: fake first, then real
    net = module(cfg, sd).train()
    pred_f, _ = net(fake)
    pred_r, _, l_gp = loss_mod.gradient_penalty(net, real)
    (loss_mod.hinge_loss(pred_f, pred_r, "disc") + gp.W_GP * l_gp).backward()
    twin = module(cfg, sd).train()
    tr = i2v_train.TemporalDiscPenaltyTrainer(twin, w_GP=gp.W_GP, optimizer=torch.optim.SGD(twin.parameters(), lr=0.0))
    out = tr.step(fake, real)
    assert torch.equal(out[3], l_gp.detach()) and abs(float(out[0]) - float(loss_mod.hinge_loss(pred_f, pred_r, "disc").detach())) < 1e-6
    for (k, p), q in zip(net.named_parameters(), twin.parameters()):
        assert torch.equal(p.grad, q.grad), k


def test_forward_with_penalty_frozen_module_input_gradient_and_second_order_refusal():
    cfg, sd, x = case("b")
    x = x.to(DEV)
    d_pred, d_fmaps = tc.upstream_b()
    net = module(cfg, sd).train()
    xa = x.clone().requires_grad_(True)
    pa, fa = net(xa)
    ((pa * d_pred.to(DEV)).sum() + sum((f * g.to(DEV)).sum() for f, g in zip(fa, d_fmaps))).backward()
    # x.grad receives the pred / fmaps part only, with and without the penalty in the loss
    twin = module(cfg, sd).train()
    xb = x.clone().requires_grad_(True)
    pb, fb, l_gp = twin.forward_with_penalty(xb)
    ((pb * d_pred.to(DEV)).sum() + sum((f * g.to(DEV)).sum() for f, g in zip(fb, d_fmaps)) + 3.0 * l_gp).backward()
    assert torch.equal(xb.grad, xa.grad)
    moved = [k for (k, p), q in zip(twin.named_parameters(), net.parameters()) if not torch.equal(p.grad, q.grad)]
    assert len(moved) == len(list(net.parameters())) - 1 and ZERO_KEY not in moved          # every parameter but one has a penalty gradient
    # only the penalty in the loss: the parameters get it, the clips nothing
    solo = module(cfg, sd).train()
    xs = x.clone().requires_grad_(True)
    solo.forward_with_penalty(xs)[2].backward()
    _, _, _, _, g1, _, _ = run_penalty("b")
    assert xs.grad is None and all(torch.equal(p.grad, g1[k]) for k, p in solo.named_parameters())
    # a frozen module: the values, the input gradient, no parameter gradient
    frozen = module(cfg, sd).train()
    for p in frozen.parameters():
        p.requires_grad_(False)
    xc = x.clone().requires_grad_(True)
    pc, fc_, lc = frozen.forward_with_penalty(xc)
    ((pc * d_pred.to(DEV)).sum() + sum((f * g.to(DEV)).sum() for f, g in zip(fc_, d_fmaps)) + 3.0 * lc).backward()
    assert torch.equal(xc.grad, xa.grad) and torch.equal(lc.detach(), l_gp.detach()) and all(p.grad is None for p in frozen.parameters())
    with torch.no_grad():
        pn, fn, ln = module(cfg, sd).train().forward_with_penalty(x)
    assert pn.grad_fn is None and ln.grad_fn is None and torch.equal(pn, pb.detach()) and torch.equal(ln, l_gp.detach())
    xd = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(twin.forward_with_penalty(xd)[2], list(twin.parameters()), create_graph=True, allow_unused=True)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(twin(xd)[0].mean(), xd, create_graph=True)


# ---------------------------------------------------------------------------------------------------------------- trainer

def test_trainer_step_follows_the_references_six_sgd_steps():
    """TemporalDiscPenaltyTrainer.step (w_GP = 10) with plain SGD against the reference's float64 pairs (L_d_t, L_GP); the bound per step is
    4 x |reference in fp32 - reference in float64|, floor 1e-6, as test_trainer_step_follows_the_references_six_sgd_steps of the plain step."""
    cfg, sd, _ = case("a")
    main = load("disc3d_gp_a.npz")
    net = module(cfg, sd).train()
    tr = i2v_train.TemporalDiscPenaltyTrainer(net, w_GP=gp.W_GP, optimizer=torch.optim.SGD(net.parameters(), lr=tc.SGD_LR))
    fake, real = (t.to(DEV) for t in tc.clips_a())
    outs = [tr.step(fake, real) for _ in range(tc.SGD_STEPS)]
    pairs = np.array([[float(o[0]), float(o[3])] for o in outs])
    bound = np.maximum(4 * np.abs(main["sgd_pairs_f32"] - main["sgd_pairs"]), 1e-6)
    diff = np.abs(pairs - main["sgd_pairs"])
    for i in range(tc.SGD_STEPS):
        print(f"  step {i}: L_d_t {pairs[i, 0]:.6f} (|gpu - f64| {diff[i, 0]:.2e}, bound {bound[i, 0]:.2e})  L_GP {pairs[i, 1]:.6e} "
              f"(|gpu - f64| {diff[i, 1]:.2e}, bound {bound[i, 1]:.2e})")
    assert np.all(diff <= bound), (diff, bound)
    assert len(set(np.round(main["sgd_pairs"][:, 1], 12))) == tc.SGD_STEPS      # the penalty moves with the steps: the sequence tests them


def test_fused_adam_trainer_five_steps_and_w_gp_zero():
    cfg, sd, _ = case("a")
    net = module(cfg, sd).train()
    tr = i2v_train.TemporalDiscPenaltyTrainer(net)
    assert tr.w_GP == 10.0 and isinstance(tr.optimizer, i2v_train.FusedAdam)
    fake, real = (t.to(DEV) for t in tc.clips_a())
    out = [tr.step(fake.transpose(1, 2), real.transpose(1, 2)) for _ in range(5)]      # [B, T, 3, H, W], as the step holds its clips
    print("  (L_d_t, L_GP):", [(round(float(o[0]), 6), float(o[3])) for o in out])
    assert all(len(o) == 4 and all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in o) for o in out)
    assert all(np.isfinite([float(v) for v in o]).all() for o in out) and all(torch.isfinite(p).all() for p in net.parameters())
    # w_GP = 0 in this class is the parent's step, bit for bit, and returns L_GP = 0
    a, b = module(cfg, sd).train(), module(cfg, sd).train()
    oa = i2v_train.TemporalDiscPenaltyTrainer(a, w_GP=0).step(fake, real)
    ob = i2v_train.TemporalDiscTrainer(b).step(fake, real)
    assert float(oa[3]) == 0.0 and oa[3].dtype == torch.float64 and all(torch.equal(x, y) for x, y in zip(oa[:3], ob))
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    gpv = i2v_train.TemporalDiscPenaltyTrainer(module(cfg, sd).train()).gradient_penalty(real)          # inherited
    assert gpv.dtype == torch.float64


def test_shipped_widths_one_step_twice():
    """[64, 64, 128, 256, 512] at 2 clips of 12 x 64 x 64: every launcher at the shipped widths; finite, and two runs give the same bits."""
    sd = tc.synthetic_state(tc.CFG_SHIPPED, 6100)
    fake, real = tc.randn(6102, (2, 3, 12, 64, 64)).to(DEV), tc.randn(6103, (2, 3, 12, 64, 64)).to(DEV)
    res = []
    for _ in range(2):
        net = module(tc.CFG_SHIPPED, sd).train()
        tr = i2v_train.TemporalDiscPenaltyTrainer(net, optimizer=torch.optim.SGD(net.parameters(), lr=tc.SGD_LR))
        out = tr.step(fake, real)
        res.append((out, [p.grad.clone() for p in net.parameters()], [p.detach().clone() for p in net.parameters()]))
    (o0, g0, p0), (o1, g1, p1) = res
    print(f"  shipped widths: L_d_t {float(o0[0]):.6f}  L_GP {float(o0[3]):.6e}")
    assert all(np.isfinite(float(v)) for v in o0) and float(o0[3]) > 0 and all(bool(torch.isfinite(g).all()) for g in g0)
    assert all(torch.equal(a, b) for a, b in zip(o0, o1)) and all(torch.equal(a, b) for a, b in zip(g0, g1)) and all(torch.equal(a, b) for a, b in zip(p0, p1))
