"""GPU checks of the motion encoder's training path (csrc/i2v_encoder_train.hip, stage1_VAE/modules/resnet3D.py
``Encoder.differentiable``, stage1_VAE/modules/loss.py ``KL``): the posterior head's kernels against float64 at the derived bounds of
tests/encoder_train_common.py, the stem at stride (2, 2, 2) through the shared trunk's unit entries, the module against the fixtures made
from the reference's own module (tests/golden/encoder_train_*.npz) and against the float64 oracle that takes the GPU's ReLU masks, the
shipped widths and the agreement with the inference handle, the bit-level properties and six SGD steps.  Run with ``-s`` to see the
figures of profiles/encoder_train_gate.md."""
import glob
import os

import numpy as np
import pytest
import torch

import encoder_train_common as ec
import i2v_native
import i2v_train
import temporal_disc_common as tc
from stage1_VAE.modules.loss import KL
from stage1_VAE.modules.resnet3D import Encoder

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"a": (ec.CFG_A, ec.CLIP_A, ec.SEED_A), "b": (ec.CFG_B, ec.CLIP_B, ec.SEED_B)}


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


def module(cfg, sd, differentiable=True):
    net = Encoder(dict(cfg))
    net.load_state_dict(dict(sd))
    net = net.to(DEV)
    net.differentiable = differentiable
    return net


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rel_rows(a, b):
    return max(ec.rel_l2_rows(torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()))


def report(name, ok, ratio, l2):
    print(f"  {name}: |err|/bound {ratio:.3f}  rel-L2 {l2:.2e}")
    assert ok, (name, ratio, l2)
    return ratio


def check(name, got, want, rows=True):
    r = rel_rows(got, want) if rows else rel(got, want)
    print(f"  {name}: rel-L2 {r:.2e}")
    assert r <= ec.TOL_L2, (name, r)
    return r


def dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


# ---------------------------------------------------------------------------------------------------------------- the head's kernels

@pytest.mark.parametrize("case", ec.head_cases(), ids=lambda c: c["id"])
def test_head_forward_unit(case):
    emb, w_mu, b_mu, w_var, b_var, eps, _, _, _ = ec.head_inputs(case)
    (mu64, S_mu, n), (lv64, S_lv, _) = ec.head_forward_oracle(emb, w_mu, b_mu, w_var, b_var)
    sample, mu, logvar = i2v_native.enc3d_head_forward_unit(*dev(emb, w_mu, b_mu, w_var, b_var, eps))
    report(case["id"] + " mu", *ec.gate(mu.cpu(), mu64, S_mu, n))
    report(case["id"] + " logvar", *ec.gate(logvar.cpu(), lv64, S_lv, n))
    report(case["id"] + " sample", *ec.gate(sample.cpu(), *ec.sample_oracle(eps, mu.cpu(), logvar.cpu())))
    none, mu2, lv2 = i2v_native.enc3d_head_forward_unit(*dev(emb, w_mu, b_mu, w_var, b_var))
    assert none is None and torch.equal(mu2, mu) and torch.equal(lv2, logvar)


UPSTREAMS = ({"name": "all-kl", "ds": True, "dm": True, "dl": True, "kl": 0.7}, {"name": "all-nokl", "ds": True, "dm": True, "dl": True, "kl": 0.0},
             {"name": "no-dsample", "ds": False, "dm": True, "dl": True, "kl": 0.7}, {"name": "no-dmu", "ds": True, "dm": False, "dl": True, "kl": 0.0},
             {"name": "no-dlogvar", "ds": True, "dm": True, "dl": False, "kl": 0.7}, {"name": "kl-alone", "ds": False, "dm": False, "dl": False, "kl": 1.0})


@pytest.mark.parametrize("case", ec.head_cases(), ids=lambda c: c["id"])
def test_head_backward_unit(case):
    """Every case with every upstream pointer NULL in turn, kl_scale zero and nonzero (the variants rotate over the cases; the first case
    runs them all), and accumulate = write-then-add, bit for bit."""
    emb, w_mu, b_mu, w_var, b_var, eps, d_s, d_m, d_l = ec.head_inputs(case)
    _, mu, logvar = i2v_native.enc3d_head_forward_unit(*dev(emb, w_mu, b_mu, w_var, b_var))
    idx = ec.head_cases().index(case)
    variants = UPSTREAMS if idx == 0 else (UPSTREAMS[idx % len(UPSTREAMS)], UPSTREAMS[(idx + 3) % len(UPSTREAMS)])
    for v in variants:
        ups = (d_s if v["ds"] else None, d_m if v["dm"] else None, d_l if v["dl"] else None)
        fold = ec.fold_oracle(mu.cpu(), logvar.cpu(), eps, *ups, v["kl"])
        want = ec.head_backward_oracle(emb, w_mu, w_var, *fold)
        got = i2v_native.enc3d_head_backward_unit(*dev(emb, w_mu, w_var), mu, logvar, *dev(eps if v["ds"] else None, *ups), kl_scale=v["kl"])
        for name, g in zip(("d_emb", "dw_mu", "db_mu", "dw_var", "db_var"), got):
            ref, S, n = want[name]
            if g.dim() == 1:
                g, ref, S = g[None], ref[None], S[None]
            report(f"{case['id']} {v['name']} {name}", *ec.gate(g.cpu(), ref, S, n))
        only_dx = i2v_native.enc3d_head_backward_unit(*dev(emb, w_mu, w_var), mu, logvar, *dev(eps if v["ds"] else None, *ups), kl_scale=v["kl"],
                                                      param_grads=False)
        assert only_dx[1] is None and torch.equal(only_dx[0], got[0])
    prior = [ec.randn(case["seed"] + 20 + i, tuple(g.shape)).to(DEV) for i, g in enumerate(got[1:])]
    acc = [p.clone() for p in prior]
    again = i2v_native.enc3d_head_backward_unit(*dev(emb, w_mu, w_var), mu, logvar, *dev(eps if v["ds"] else None, *ups), kl_scale=v["kl"], into=acc)
    assert torch.equal(again[0], got[0]) and all(torch.equal(a, p + g) for a, p, g in zip(acc, prior, got[1:]))
    with pytest.raises(i2v_native.I2VError):
        i2v_native.enc3d_head_backward_unit(*dev(emb, w_mu, w_var), mu, logvar)


@pytest.mark.parametrize("case", [ec.head_cases()[0], ec.head_cases()[5], ec.head_cases()[-1]], ids=lambda c: c["id"])
def test_kl_backward_entry_and_kl_with_a_grad_fn(case):
    """i2v_enc3d_kl_backward against float64; loss.KL with grad has the value bits of KL without and the kernel's gradient."""
    _, _, _, _, _, mu, logvar, _, _ = ec.head_inputs(case)
    logvar = 0.5 * logvar
    g_mu, g_lv, S_mu, S_lv = ec.fold_oracle(mu, logvar, None, None, None, None, 1.0)
    d_mu, d_lv = i2v_native.enc3d_kl_backward(*dev(mu, logvar), 1.0)
    report(case["id"] + " d_mu", *ec.gate(d_mu.cpu(), g_mu, S_mu, 1))
    report(case["id"] + " d_logvar", *ec.gate(d_lv.cpu(), g_lv, S_lv, 1))
    m, l = (t.to(DEV).requires_grad_(True) for t in (mu, logvar))
    with torch.no_grad():
        plain = KL(m, l)
    val = KL(m, l)
    assert val.grad_fn is not None and plain.grad_fn is None and val.dtype == torch.float64 and torch.equal(val.detach(), plain)
    assert abs(float(val.detach()) - float(ec.kl_value(mu.double(), logvar.double()))) <= 1e-12 * abs(float(val.detach()))
    val.backward()
    assert m.grad.dtype == torch.float32 and torch.equal(m.grad, d_mu) and torch.equal(l.grad, d_lv)
    assert KL(m.detach(), l.detach()).grad_fn is None


STEM_S2_CASES = [{"id": f"stem-s222-{t}x{h}x{w}-b{b}", "cin": 3, "cout": 16, "st": 2, "ss": 2, "k": 7, "thw": (t, h, w), "batch": b, "seed": 62000 + 10 * i}
                 for i, (t, h, w, b) in enumerate(((2, 16, 16, 1), (3, 10, 12, 2)))]


@pytest.mark.parametrize("case", STEM_S2_CASES, ids=lambda c: c["id"])
def test_stem_at_stride_2_2_2_through_the_shared_unit_entries(case):
    """The discriminator's tests run the (3, 7, 7) stem at temporal stride 1 only; the encoder's has stride (2, 2, 2): conv, weight gradient
    and the frames-layout input gradient at T = 2 and T = 3, at the bounds of temporal_disc_common."""
    x, w, g, act = tc.conv_case_inputs(case)
    st = dict(stride_t=2, stride_s=2)
    ref, S, n = tc.conv_oracle(x, w, 2, 2)
    report(case["id"] + " conv", *tc.gate(tc.uncl(i2v_native.disc3d_conv_unit(tc.cl(x).to(DEV), w.to(DEV), **st).cpu()), ref, S, n))
    ref, S, n = tc.dgrad_oracle(g, w, act, case["thw"], 2, 2)
    assert float(n.min()) < float(n.max())
    out = i2v_native.disc3d_dgrad_unit(tc.cl(g).to(DEV), w.to(DEV), case["thw"], tc.cl(act).to(DEV), frames=True, **st).cpu()
    report(case["id"] + " dgrad frames", *tc.gate(out, ref, S, n))
    ref, bound = tc.wgrad_oracle(g, x, w, act, 2, 2)
    dw = i2v_native.disc3d_wgrad_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), w.to(DEV), act=tc.cl(act).to(DEV), **st).cpu()
    report(case["id"] + " wgrad", *tc.gate_bound(dw, ref, bound))


# ---------------------------------------------------------------------------------------------------------------- the module

def run_entries(net, x, eps, ups, kl_scale, accumulate=False, grads=None):
    """One saved forward and one backward through the handle's entries -> (outs, dx, grads, saved, handle)"""
    grads = grads if grads is not None else {k: torch.zeros_like(p) for k, p in net.named_parameters()}
    h = net._train_handle(grads)
    sample, mu, logvar, saved = h.forward(x, eps, save=True)
    dx = h.backward(*ups, saved, tuple(x.shape), kl_scale=kl_scale, need_dx=True, param_grads=True, accumulate=accumulate)
    return (sample, mu, logvar), dx, grads, saved, h


@pytest.mark.parametrize("tag", ["a", "b"])
def test_module_against_the_reference_fixture(tag):
    cfg, clip, seed = FIXTURES[tag]
    main, ref_grads = load(f"encoder_train_{tag}.npz"), load(f"encoder_train_{tag}_grads*.npz")
    sd = ec.synthetic_state(cfg, seed)
    x, eps, *coefs = dev(*ec.inputs(cfg, clip, seed))
    net = module(cfg, sd)
    outs, dx, grads, saved, h = run_entries(net, x, eps, coefs, ec.KL_WEIGHT)
    worst = [check(f"{tag} {name}", got, main[name]) for name, got in zip(("sample", "mu", "logvar"), outs)]
    worst.append(check(f"{tag} dx", dx, main["dx"]))
    assert set(grads) == set(ref_grads)
    per = {k: rel(grads[k], v) for k, v in ref_grads.items()}
    k_worst = max(per, key=per.get)
    print(f"  {tag}: worst of {len(per)} parameter gradients: {k_worst} rel-L2 {per[k_worst]:.2e}")
    assert per[k_worst] <= ec.TOL_L2, (k_worst, per[k_worst])
    # the KL term alone
    dxk = h.backward(None, None, None, saved, tuple(x.shape), kl_scale=ec.KL_WEIGHT)
    check(f"{tag} dx under KL alone", dxk, main["kl.dx"])
    kper = {k[3:]: rel(grads[k[3:]], v) for k, v in main.items() if k.startswith("kl.") and k != "kl.dx"}
    k_worst = max(kper, key=kper.get)
    print(f"  {tag}: under KL alone, worst of {len(kper)} stored gradients: {k_worst} rel-L2 {kper[k_worst]:.2e}")
    assert kper[k_worst] <= ec.TOL_L2, (k_worst, kper[k_worst])


def gpu_decisions(handle, saved, shape, cfg):
    """The ReLU masks of a saved forward, keyed as the oracle keys them."""
    maps = handle.saved_maps(saved, shape)
    names, i = {0: "norm1"}, 1
    for b in ec.blocks(cfg):
        names[i], names[i + 1] = b["prefix"] + "bn1", b["prefix"] + "bn2"
        i += 3 if b["ds"] else 2
    return {name: ec.uncl(maps[(i2v_native.ENC3D_TRAIN_ACT, ci)]).cpu() > 0 for ci, name in names.items()}


def against_oracle(name, cfg, sd, x, eps, coefs, kl_scale):
    """One saved forward and one backward through the entries against the float64 oracle run on the GPU's own ReLU decisions."""
    net = module(cfg, sd)
    outs, dx, grads, saved, h = run_entries(net, *dev(x, eps), dev(*coefs), kl_scale)
    shape = tuple(x.shape)
    dec = gpu_decisions(h, saved, shape, cfg)
    *_, own = ec.forward_oracle(sd, x, eps, cfg)
    rep = ec.decision_report(dec, own)
    print(f"  {name}: decisions that differ from float64's (all, outside the band):", {k: v for k, v in rep.items() if v[0]})
    assert sum(v[1] for v in rep.values()) == 0 and sum(v[0] for v in rep.values()) <= ec.FRAGILE_MAX, rep
    s64, m64, l64, c = ec.forward_oracle(sd, x, eps, cfg, decisions=dec)
    g64, dx64 = ec.backward_oracle(c, *coefs, kl_scale)
    maps, convs = h.saved_maps(saved, shape), [c["stem"]]
    for st in c["steps"]:
        convs += [st["c1"], st["c2"]] + ([st["cd"]] if st["cd"] is not None else [])
    assert len(maps) == 2 * len(convs)
    raw = max(rel_rows(ec.uncl(maps[(i2v_native.ENC3D_TRAIN_CONV_OUT, ci)]), cv["y"]) for ci, cv in enumerate(convs))
    print(f"  {name}: worst rel-L2 of the {len(convs)} raw conv outputs {raw:.2e}")
    assert raw <= ec.TOL_L2, raw
    worst = max([check(f"{name} sample", outs[0], s64), check(f"{name} mu", outs[1], m64), check(f"{name} logvar", outs[2], l64),
                 check(f"{name} dx", dx, dx64)] + [rel(grads[k], g64[k]) for k in g64])
    for k in g64:
        assert rel(grads[k], g64[k]) <= ec.TOL_L2, (k, rel(grads[k], g64[k]))
    print(f"  {name}: worst rel-L2 over outputs, input gradient and {len(g64)} parameter gradients {worst:.2e}")
    return net, outs


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_on_the_gpus_decisions(tag):
    cfg, clip, seed = FIXTURES[tag]
    x, eps, *coefs = ec.inputs(cfg, clip, seed)
    against_oracle(tag.upper(), cfg, ec.synthetic_state(cfg, seed), x, eps, coefs, ec.KL_WEIGHT)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_saved_layout_is_consistent(tag):
    """The entries of ``saved_maps``: inside ``saved``, on 256-byte offsets, disjoint, two per conv; the workspace holds a forward that
    does not save."""
    cfg, clip, seed = FIXTURES[tag]
    x, eps, *_ = dev(*ec.inputs(cfg, clip, seed))
    h = module(cfg, ec.synthetic_state(cfg, seed))._train_handle()
    n, _, t, hh, w = clip
    saved = h.forward(x, eps, save=True)[3]
    assert saved.numel() == h.saved_bytes(n, t, hh, w) <= h.workspace_bytes(n, t, hh, w)
    maps = h.saved_maps(saved, clip)
    assert len(maps) == 2 * (1 + sum(3 if b["ds"] else 2 for b in ec.blocks(cfg)))
    spans = sorted((m.data_ptr() - saved.data_ptr(), m.data_ptr() - saved.data_ptr() + m.numel() * m.element_size()) for m in maps.values())
    assert all(a % 256 == 0 and 0 <= a < b <= saved.numel() for a, b in spans)
    assert all(p[1] <= q[0] for p, q in zip(spans, spans[1:]))          # sorted by their starts: no two overlap


def test_refusal_names_the_final_map():
    net = module(ec.CFG_B, ec.synthetic_state(ec.CFG_B, ec.SEED_B))
    with pytest.raises(i2v_native.I2VError, match=r"\[1, 8, 8\] map"):
        net(torch.zeros(1, 3, 3, 16, 16, device=DEV))
    h = net._train_handle()
    assert h.out_shape(3, 8, 8) == (1, 4, 4, 32) == h.out_shape(4, 8, 8)       # no power-of-two rule: 8 x 8 frames, two stem frames from T = 3
    x, eps, *coefs = dev(*ec.inputs(ec.CFG_B, ec.CLIP_B, ec.SEED_B))
    _, _, _, saved = h.forward(x, eps, save=True)
    with pytest.raises(i2v_native.I2VError):           # neither an upstream gradient nor kl_scale
        h.backward(None, None, None, saved, tuple(x.shape))
    with pytest.raises(i2v_native.I2VError):           # nothing asked for
        h.backward(*coefs, saved, tuple(x.shape), need_dx=False, param_grads=False)


def test_shipped_widths_against_the_oracle_and_the_inference_handle():
    """[64, 128, 256, 512, 512], strides [1, 2, 2, 2], one clip of 16 frames at 64 x 64: forward and backward against the oracle; then the
    training forward against i2v_encoder3d_forward (split-fp16 convs, other arithmetic: a distance, not bit equality) on the same weights,
    at the project's 1e-4, and the reparameterised sample of one seed on both paths."""
    cfg = ec.CFG_SHIPPED
    sd = ec.synthetic_state(cfg, ec.SEED_SHIPPED)
    x, eps, *coefs = ec.inputs(cfg, ec.CLIP_SHIPPED, ec.SEED_SHIPPED)
    net, (sample, mu, logvar) = against_oracle("shipped", cfg, sd, x, eps, coefs, ec.KL_WEIGHT)
    plain = module(cfg, sd, differentiable=False)
    with torch.no_grad():
        torch.manual_seed(77)
        s_inf, mu_inf, lv_inf = plain(x.to(DEV))
        torch.manual_seed(77)
        s_tr, mu_tr, lv_tr = net(x.to(DEV))
    assert torch.equal(mu_tr, mu) and torch.equal(lv_tr, logvar)
    d = [check("training vs inference handle: mu", mu_tr, mu_inf), check("training vs inference handle: logvar", lv_tr, lv_inf),
         check("training vs inference handle: sample of one seed", s_tr, s_inf)]
    print(f"  shipped widths: distance of the training forward from the inference handle (rel-L2 of mu, logvar, sample): {d}")


# ---------------------------------------------------------------------------------------------------------------- module behaviour

def test_two_runs_give_the_same_bits_and_accumulate_is_write_then_add():
    cfg, clip, seed = FIXTURES["b"]
    sd = ec.synthetic_state(cfg, seed)
    x, eps, *coefs = dev(*ec.inputs(cfg, clip, seed))
    (o0, dx0, g0, saved, h), (o1, dx1, g1, _, _) = (run_entries(module(cfg, sd), x, eps, coefs, 0.3) for _ in range(2))
    assert all(torch.equal(a, b) for a, b in zip(o0, o1)) and torch.equal(dx0, dx1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    prior = {k: ec.randn(63000 + i, tuple(v.shape)).to(DEV) for i, (k, v) in enumerate(g0.items())}
    acc = {k: v.clone() for k, v in prior.items()}
    net = module(cfg, sd)
    _, dx2, _, _, _ = run_entries(net, x, eps, coefs, 0.3, accumulate=True, grads=acc)
    assert torch.equal(dx2, dx0) and all(torch.equal(acc[k], prior[k] + g0[k]) for k in g0)


def test_autograd_path_equals_the_backward_entry_frozen_module_and_second_order_refusal():
    cfg, clip, seed = FIXTURES["b"]
    sd = ec.synthetic_state(cfg, seed)
    x, eps, cs, cm, clv = dev(*ec.inputs(cfg, clip, seed))
    outs, dx, grads, _, _ = run_entries(module(cfg, sd), x, eps, (cs, cm, clv), 0.0)
    twin = module(cfg, sd)
    xa = x.clone().requires_grad_(True)
    sample, mu, logvar = twin(xa, eps=eps)
    assert sample.grad_fn is not None and mu.grad_fn is not None and logvar.grad_fn is not None
    ((sample * cs).sum() + (mu * cm).sum() + (logvar * clv).sum()).backward()
    assert all(torch.equal(a.detach(), b) for a, b in zip((sample, mu, logvar), outs)) and torch.equal(xa.grad, dx)
    assert all(torch.equal(p.grad, grads[k]) for k, p in twin.named_parameters())
    # KL through its own grad_fn next to the fused kl_scale: the same gradient up to the rounding of one more addition
    twin.zero_grad()
    _, mu2, lv2 = twin(x, eps=eps)
    KL(mu2, lv2).backward()
    _, _, gk, _, _ = run_entries(module(cfg, sd), x, eps, (None, None, None), 1.0)
    assert all(rel(p.grad, gk[k]) <= 1e-6 for k, p in twin.named_parameters())
    # a frozen module: no parameter gradient, the same input gradient
    for p in twin.parameters():
        p.requires_grad_(False)
    xb = x.clone().requires_grad_(True)
    sample, mu, logvar = twin(xb, eps=eps)
    ((sample * cs).sum() + (mu * cm).sum() + (logvar * clv).sum()).backward()
    assert torch.equal(xb.grad, dx) and all(p.grad is None or not p.requires_grad for p in twin.parameters())
    assert twin(x, eps=eps)[0].grad_fn is None           # nothing requires grad: the plain forward
    xc = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(twin(xc, eps=eps)[1].sum(), xc, create_graph=True)


def test_optimizer_step_is_seen_and_switching_back_rebuilds_the_inference_handle():
    cfg, clip, seed = ec.CFG_D, ec.CLIP_D, ec.SEED_D       # 64 x 64 frames: the inference handle refuses smaller ones
    sd = ec.synthetic_state(cfg, seed)
    x, eps, cs, cm, clv = dev(*ec.inputs(cfg, clip, seed))
    net = module(cfg, sd, differentiable=False)
    with torch.no_grad():
        before = net(x, eps=eps)                          # builds the packed inference handle on the initial weights
    net.differentiable = True
    opt = i2v_train.FusedAdam(net.parameters(), lr=1e-3)
    sample, mu, logvar = net(x, eps=eps)
    ((sample * cs).sum() + (mu * cm).sum() + (logvar * clv).sum() + KL(mu, logvar)).backward()
    opt.step()
    with torch.no_grad():
        after = net(x, eps=eps)
    assert not torch.equal(after[1], mu.detach())         # the next differentiable forward reads the stepped weights, no refresh
    fresh = module(cfg, net.state_dict())
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(fresh(x, eps=eps), after))
    net.differentiable = False                            # -> refresh_native(): the packed handle is rebuilt from the stepped weights
    new_inference = module(cfg, net.state_dict(), differentiable=False)
    with torch.no_grad():
        back, want = net(x, eps=eps), new_inference(x, eps=eps)
    assert all(torch.equal(a, b) for a, b in zip(back, want)) and not torch.equal(back[1], before[1])
    # the same seed gives the same draw on both paths
    with torch.no_grad():
        torch.manual_seed(5)
        s_inf = net(x)[0]
        net.differentiable = True
        torch.manual_seed(5)
        s_tr = net(x)[0]
    check("sample of one seed, training vs inference path", s_tr, s_inf)


def test_six_sgd_steps_follow_the_references_loss_sequence():
    """Plain SGD on fixture A's loss through the autograd form against the reference's float64 sequence; the bound per step is
    4 x |reference in fp32 - reference in float64| (the rule of the discriminator tests), floor 1e-6."""
    cfg, clip, seed = FIXTURES["a"]
    main = load("encoder_train_a.npz")
    net = module(cfg, ec.synthetic_state(cfg, seed))
    x, eps, cs, cm, clv = dev(*ec.inputs(cfg, clip, seed))
    opt = torch.optim.SGD(net.parameters(), lr=ec.SGD_LR)
    losses = []
    for _ in range(ec.SGD_STEPS):
        opt.zero_grad()
        sample, mu, logvar = net(x, eps=eps)
        loss = (sample.double() * cs).sum() + (mu.double() * cm).sum() + (logvar.double() * clv).sum() + ec.KL_WEIGHT * KL(mu, logvar)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    losses = np.array(losses)
    bound = np.maximum(4 * np.abs(main["sgd_losses_f32"] - main["sgd_losses"]), 1e-6)
    diff = np.abs(losses - main["sgd_losses"])
    print("  losses:", [f"{v:.6f}" for v in losses])
    print("  |gpu - f64|:", [f"{v:.2e}" for v in diff], " bound:", [f"{v:.2e}" for v in bound])
    assert np.all(diff <= bound), (diff, bound)
