"""CPU checks of the temporal discriminator (stage1_VAE/modules/resnet3D.py ``Discriminator`` on csrc/i2v_disc3d.hip): the float64 oracle of
tests/temporal_disc_common.py against the fixtures made from the reference's own module and against torch autograd; every deliberate error
against the gate the GPU tests apply; the C ABI of include/i2v_hip_disc3d.h against i2v_native.DISC3D_SYMBOLS; the refusals; the state
dict and the construction draws; the slice plan; the fragile band of the fp32 restatement."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch
from torch.nn.grad import conv3d_input

import i2v_native
import temporal_disc_common as tc
import test_host_abi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
GOLDEN = os.path.join(REPO, "tests", "golden")
ENCODER_TEXT_SHA256 = "1abf7d78d933222c5077bd0de2cd317c3967736069855cc2a01454512b33c1a5"


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
    """Other modules of the suite switch grad mode off for the process; a test here compares with autograd."""
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


@pytest.fixture(scope="module")
def train_pass(fxa):
    """Fixture A's training step through the oracle: fake first, then real on the updated u, v."""
    _, sd, _ = fxa
    fake, real = tc.clips_a()
    pf, ff, cf = tc.forward_oracle(sd, fake, tc.CFG_A, training=True)
    sd2 = dict(sd, **cf["state"])
    pr, fr, cr = tc.forward_oracle(sd2, real, tc.CFG_A, training=True)
    return sd, fake, real, (pf, ff, cf), (pr, fr, cr)


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def step_grads(cf, cr, pf, pr, mutate=None):
    df, dr = tc.hinge_disc_grads(pf, pr)
    gf, dxf = tc.backward_oracle(cf, df, mutate=mutate)
    gr, dxr = tc.backward_oracle(cr, dr, mutate=mutate)
    return {k: gf[k] + gr[k] for k in gf}, dxf, dxr


def test_every_fixture_file_is_below_the_committed_size_limit():
    files = glob.glob(os.path.join(GOLDEN, "temporal_disc_*.npz"))
    assert len(files) == 16 and all(os.path.getsize(f) < 1 << 20 for f in files)


def test_oracle_reproduces_fixture_a(fxa, train_pass):
    main, _, grads = fxa
    sd, fake, real, (pf, ff, cf), (pr, fr, cr) = train_pass
    assert rel(pf, main["train_pred_fake"]) < 1e-12 and rel(pr, main["train_pred_real"]) < 1e-12
    assert abs(float(tc.hinge_disc(pf, pr)) - float(main["train_loss"])) < 1e-13
    for name, fm in (("fake", ff), ("real", fr)):
        sums = np.array([[float(f.sum()), float(f.pow(2).sum())] for f in fm])
        assert np.allclose(sums, main["train_fmaps_" + name], rtol=1e-11, atol=1e-11)
        assert rel(fm[3], main["train_fmap3_" + name]) < 1e-12
    after = dict(cf["state"], **cr["state"])
    assert {"after." + k for k in after} == {k for k in main if k.startswith("after.")} and len(after) == 24
    for k, v in after.items():
        assert rel(v, main["after." + k]) < 1e-12, k
    g, dxf, dxr = step_grads(cf, cr, pf, pr)
    assert set(g) == set(grads)
    for k in g:
        assert rel(g[k], grads[k]) < 2e-7, k          # the fixture's gradients are rounded to fp32
    assert rel(dxf, load_dx("fake")) < 2e-7 and rel(dxr, load_dx("real")) < 2e-7
    sd_eval = dict(sd, **after)
    for t in (12, 5):
        pred, _, _ = tc.forward_oracle(sd_eval, tc.clips_a_eval(t), tc.CFG_A, training=False)
        assert rel(pred, main[f"eval_t{t}"]) < 1e-12, t


def test_oracle_reproduces_the_generator_loss_and_the_penalty(fxa):
    main, sd, _ = fxa
    fake, real = tc.clips_a()
    (coup, fm, total), dx, _ = tc.generator_loss_oracle(sd, fake, real, tc.CFG_A)
    assert abs(float(coup) - main["gen_coup"]) < 1e-12 and abs(float(fm) - main["gen_fmap"]) < 1e-12 and abs(float(total) - main["gen_loss"]) < 1e-11
    assert rel(dx, load_dx("gen")) < 2e-7
    gp, _ = tc.gradient_penalty_oracle(sd, real, tc.CFG_A)
    assert abs(float(gp) / main["gp_value"] - 1) < 1e-11


def test_oracle_reproduces_fixtures_b_and_c(fxb):
    main, grads = fxb
    sd = tc.synthetic_state(tc.CFG_B, tc.SEED_B)
    d_pred, d_fmaps = tc.upstream_b()
    pred, fmaps, c = tc.forward_oracle(sd, tc.clips_b(), tc.CFG_B, training=True)
    assert rel(pred, main["b_pred"]) < 1e-12 and all(rel(f, main[f"b_fmap{i}"]) < 1e-12 for i, f in enumerate(fmaps))
    assert [tuple(f.shape) for f in fmaps] == [tuple(g.shape) for g in d_fmaps]
    assert fmaps[2].shape[2] == 1 and fmaps[3].shape[2] == 1                      # T = 1 under stride 1
    assert "layer.3.0.downsample.0.weight_orig" not in sd and "layer.1.0.downsample.0.weight_orig" in sd
    g, dx = tc.backward_oracle(c, d_pred, d_fmaps)
    assert set(g) == set(grads) and rel(dx, main["b_dx"]) < 1e-11
    for k in g:
        assert rel(g[k], grads[k]) < 2e-7, k
    pred, fmaps, _ = tc.forward_oracle(tc.synthetic_state(tc.CFG_C, tc.SEED_B), tc.clips_c(), tc.CFG_C, training=True)
    assert rel(pred, main["c_pred"]) < 1e-12 and all(rel(f, main[f"c_fmap{i}"]) < 1e-12 for i, f in enumerate(fmaps))


def test_oracle_sgd_steps_follow_the_fixture(fxa):
    main, sd, _ = fxa
    sd = {k: v.double() for k, v in sd.items()}
    fake, real = tc.clips_a()
    assert np.all(np.abs(main["sgd_losses_f32"] - main["sgd_losses"]) < 1e-4)
    for step in range(tc.SGD_STEPS):
        pf, _, cf = tc.forward_oracle(sd, fake, tc.CFG_A, training=True)
        sd = dict(sd, **cf["state"])
        pr, _, cr = tc.forward_oracle(sd, real, tc.CFG_A, training=True)
        sd = dict(sd, **cr["state"])
        assert abs(float(tc.hinge_disc(pf, pr)) - main["sgd_losses"][step]) < 1e-11
        g, _, _ = step_grads(cf, cr, pf, pr)
        for k in g:
            sd[k] = sd[k] - tc.SGD_LR * g[k].reshape(sd[k].shape)


def test_oracle_equals_autograd_on_a_torch_restatement():
    """The hand-written backward against autograd through the oracle's own forward (float64), with feature-map gradients."""
    sd = {k: v.double().requires_grad_(not k.endswith(("_u", "_v"))) for k, v in tc.synthetic_state(tc.CFG_B, 77).items()}
    x = tc.clips_b()[:2].double().requires_grad_(True)
    d_pred, d_fmaps = tc.upstream_b()
    d_pred, d_fmaps = d_pred[:2].double(), [g[:2].double() for g in d_fmaps]
    with torch.no_grad():
        _, _, c = tc.forward_oracle(sd, x, tc.CFG_B, training=True)
        g, dx = tc.backward_oracle(c, d_pred, d_fmaps)
    # autograd: u and v are constants of the forward, as in torch.nn.utils.spectral_norm
    fixed = {k: v.detach() if k.endswith(("_u", "_v")) else v for k, v in dict(sd, **c["state"]).items()}
    pred, fmaps, _ = tc.forward_oracle(fixed, x, tc.CFG_B, training=False)
    ((pred * d_pred).sum() + sum((f * q).sum() for f, q in zip(fmaps, d_fmaps))).backward()
    assert rel(dx, x.grad) < 1e-12
    for k in g:
        assert rel(g[k], sd[k].grad) < 1e-11, k


def test_dgrad_by_taps_is_the_transposed_convolution():
    for case in tc.conv_cases()[::3] + tc.STEM_CASES:
        _, w, g, _ = tc.conv_case_inputs(case)
        k = w.shape[-1]
        ref = conv3d_input((g.shape[0], w.shape[1]) + tuple(case["thw"]), w.double(), g.double(), stride=(case["st"], case["ss"], case["ss"]),
                           padding=(1, k // 2, k // 2))
        assert rel(tc.dgrad_taps(g.double(), w.double(), case["thw"], (case["st"], case["ss"], case["ss"])), ref) < 1e-14, case["id"]


def test_every_deliberate_error_exceeds_the_gate(fxa, train_pass):
    """The module gate (rel-L2 <= 1e-4 per tensor) rejects each error on fixture A's training step; printed with -s.  Three errors cannot
    show in the module: a GroupNorm follows every conv, so nothing behind it depends on the conv's scale.  <dWn, Wn> vanishes (up to eps) and
    with it the whole projection term -- dropping it, or forming it with the u from before the iteration, changes the module's gradients by
    ~1e-6 relative -- and dividing a block-1 weight by its sigma changes neither an output nor a gradient.  The two projection errors are
    held to the same 1e-4 on the weight-gradient unit, where the upstream gradient is free; the third on the raw conv outputs of the
    module, which the GPU module tests compare with the oracle's."""
    sd, fake, real, (pf, ff, cf), (pr, fr, cr) = train_pass
    ref, dxf, _ = step_grads(cf, cr, pf, pr)
    worst = {}
    for m in tc.MUTATIONS:
        if m in ("projection_dropped", "u_before_iteration"):
            in_module = max(rel(v, ref[k]) for k, v in step_grads(cf, cr, pf, pr, mutate=m)[0].items())
            assert in_module < tc.TOL_L2                                 # (the reason for the unit-level check)
            case = tc.wgrad_cases()[2]
            x, w, g, act = tc.conv_case_inputs(case)
            u0, v0 = tc.randn(1, (w.shape[0],)).double(), tc.randn(2, (w[0].numel(),)).double()
            u0, v0 = u0 / u0.norm(), v0 / v0.norm()
            u, v, sigma = tc.power_iteration(w.double().reshape(w.shape[0], -1), u0, v0)
            good, _ = tc.wgrad_oracle(g, x, w, act, case["st"], case["ss"], u, v, sigma)
            bad, _ = tc.wgrad_oracle(g, x, w, act, case["st"], case["ss"], u, v, sigma, mutate=m, u0=u0)
            worst[m] = rel(bad, good)
            continue
        if m == "block1_spectral":
            # Nothing behind a GroupNorm sees it; the raw conv outputs, which the GPU module tests compare, do.  Measured on fixture B's
            # state: fixture A's block-1 weights are orthogonal as constructed, their sigma is 1 and the error is none there.
            pm, fm, _ = tc.forward_oracle(sd, fake, tc.CFG_A, training=True, mutate=m)
            assert max(rel(pm, pf), max(rel(a, b) for a, b in zip(fm, ff))) < tc.TOL_L2
            sdb = tc.synthetic_state(tc.CFG_B, tc.SEED_B)
            good, bad = (tc.forward_oracle(sdb, tc.clips_b(), tc.CFG_B, training=True, mutate=mm)[2]["steps"] for mm in (None, m))
            assert max(rel(a["c1"]["y"], b["c1"]["y"]) for a, b in zip(bad, good) if not a["block"]["last"]) < tc.TOL_L2
            worst[m] = min(rel(a[k]["y"], b[k]["y"]) for a, b in zip(bad, good) if a["block"]["last"] for k in ("c1", "c2"))
            continue
        if m == "downsample_without_stride_t":     # errors of the forward, seen in its outputs or its gradients
            pm, fm, cm = tc.forward_oracle(sd, fake, tc.CFG_A, training=True, mutate=m)
            d = torch.ones_like(pm) / pm.numel()
            (gm, _), (g0, _) = tc.backward_oracle(cm, d), tc.backward_oracle(cf, d)
            worst[m] = max(rel(pm, pf), max(rel(a, b) for a, b in zip(fm, ff)), max(rel(gm[k], g0[k]) for k in g0 if k in gm))
            continue
        g, dx, _ = step_grads(cf, cr, pf, pr, mutate=m)
        worst[m] = max(max(rel(g[k], ref[k]) for k in ref), rel(dx, dxf))
    print("smallest-gate factors:", {k: f"{v / tc.TOL_L2:.1f}x" for k, v in worst.items()})
    assert set(worst) == set(tc.MUTATIONS)
    for m, v in worst.items():
        assert v > 10 * tc.TOL_L2, (m, v)


def test_unit_gates_reject_the_unit_errors():
    for case in tc.conv_cases()[::5]:
        _, w, g, act = tc.conv_case_inputs(case)
        ref, S, n = tc.dgrad_oracle(g, w, act, case["thw"], case["st"], case["ss"])
        for m in ("taps_not_flipped", "wrong_parity"):
            if m == "wrong_parity" and case["st"] == 1 and case["ss"] == 1:
                continue
            bad, _, _ = tc.dgrad_oracle(g, w, act, case["thw"], case["st"], case["ss"], mutate=m)
            assert not tc.gate(bad.float(), ref, S, n)[0], (case["id"], m)
        assert tc.gate(ref.float(), ref, S, n)[0]
    case = tc.wgrad_cases()[2]
    x, w, g, act = tc.conv_case_inputs(case)
    u, v, sigma = tc.power_iteration(w.double().reshape(w.shape[0], -1), tc.randn(1, (w.shape[0],)).double(), tc.randn(2, (w[0].numel(),)).double())
    ref, bound = tc.wgrad_oracle(g, x, w, act, case["st"], case["ss"], u, v, sigma)
    bad, _ = tc.wgrad_oracle(g, x, w, act, case["st"], case["ss"], u, v, sigma, mutate="projection_dropped")
    assert tc.gate_bound(ref.float(), ref, bound)[0] and not tc.gate_bound(bad.float(), ref, bound)[0]


def test_fp32_restatement_decides_like_float64_up_to_the_fragile_band(fxa, fxb, train_pass):
    """The fp32 CPU restatement on the fixtures: its ReLU masks and pool argmaxes differ from float64's only inside the fragile band
    (margin <= 1e-5 x the layer's rms), in at most FRAGILE_MAX units per case."""
    sd, fake, real, (_, _, cf), (_, _, cr) = train_pass
    sd32 = {k: v.float() for k, v in sd.items()}
    _, _, c32 = tc.forward_oracle(sd32, fake, tc.CFG_A, training=True, dtype=torch.float32)
    cases = [("a-fake", c32, cf)]
    _, _, c32 = tc.forward_oracle(dict(sd32, **c32["state"]), real, tc.CFG_A, training=True, dtype=torch.float32)
    cases.append(("a-real", c32, cr))
    sdb = tc.synthetic_state(tc.CFG_B, tc.SEED_B)
    cases.append(("b", tc.forward_oracle(sdb, tc.clips_b(), tc.CFG_B, True, dtype=torch.float32)[2], tc.forward_oracle(sdb, tc.clips_b(), tc.CFG_B, True)[2]))
    for name, lo, hi in cases:
        assert lo["margins"]["norm1"].dtype == torch.float32
        rep = tc.decision_report(lo["decisions"], hi)
        print(name, "differing decisions:", {k: v for k, v in rep.items() if v[0]})
        assert sum(v[1] for v in rep.values()) == 0, (name, rep)
        assert sum(v[0] for v in rep.values()) <= tc.FRAGILE_MAX, (name, rep)


def parse_header():
    text = open(os.path.join(REPO, "include", "i2v_hip_disc3d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    structs = re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", "", text).replace('extern "C" {', "").replace("}", "")
    funcs = {}
    for decl in (" ".join(d.split()) for d in text.split(";") if d.strip()):
        m = re.match(r"(.*?)\b(i2v_\w+)\s*\((.*)\)$", decl)
        assert m, decl
        args = [re.match(r"(.*?)(\w+)$", a.strip()).groups() for a in m.group(3).split(",") if a.strip() and a.strip() != "void"]
        funcs[m.group(2)] = (m.group(1).strip(), [(t.strip(), n) for t, n in args])
    return funcs, structs


def test_header_matches_the_third_table_and_the_other_two_are_untouched():
    funcs, structs = parse_header()
    assert set(funcs) == set(i2v_native.DISC3D_SYMBOLS) and len(funcs) == 24
    assert abi.compare_functions(funcs, i2v_native.DISC3D_SYMBOLS) == []
    assert all(n.startswith("i2v_disc3d_") for n in funcs)
    (body, name), = structs
    assert name == "i2v_disc3d_cfg"
    fields = [re.sub(r"\[\d+\]", "", f.strip()) for d in body.split(";") if d.strip() for f in d.split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in i2v_native.Disc3DCfg._fields_]
    assert [getattr(t, "_length_", 0) for _, t in i2v_native.Disc3DCfg._fields_] == [0, 5, 4, 4, 0, 0]
    res, args = i2v_native.DISC3D_SYMBOLS["i2v_disc3d_forward"]
    assert abi.compare_functions(funcs, dict(i2v_native.DISC3D_SYMBOLS, i2v_disc3d_forward=(res, args[:-1]))) != []
    main_funcs, _ = abi.parse_header()
    assert len(main_funcs) == 129 and len(i2v_native.DISC_SYMBOLS) == 19
    assert not set(main_funcs) & set(funcs) and not set(i2v_native.DISC_SYMBOLS) & set(funcs)
    assert os.path.exists(i2v_native.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(i2v_native.LIB_PATH)
    assert all(hasattr(lib, n) for n in funcs)


def test_source_is_built_and_reads_no_environment():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_disc3d.hip" in mk.split("SRCS =")[1].splitlines()[0]
    assert "../../include/i2v_hip_disc3d.h" in mk.split("HDRS =")[1].splitlines()[0].split()
    src = open(os.path.join(PKG, "csrc", "i2v_disc3d.hip")).read() + open(os.path.join(PKG, "csrc", "i2v_power_iter.h")).read()
    assert "getenv" not in src and "atomic" not in src.lower()
    assert "mfma_f32_16x16x4f32" in src


def _create(**over):
    cfg = dict(res_type=18, channels=[64, 64, 128, 256, 512], stride_s=[1, 1, 2, 2], stride_t=[2, 2, 2, 2], use_max_pool=1, spectral_norm=1)
    cfg.update(over)
    c = i2v_native.Disc3DCfg(cfg["res_type"], (ctypes.c_int32 * 5)(*cfg["channels"]), (ctypes.c_int32 * 4)(*cfg["stride_s"]),
                             (ctypes.c_int32 * 4)(*cfg["stride_t"]), cfg["use_max_pool"], cfg["spectral_norm"])
    h = ctypes.c_void_p()
    lib = i2v_native.lib()
    return lib.i2v_disc3d_create(ctypes.byref(c), ctypes.byref(h)), h, lib.i2v_last_error().decode()


def test_refusals_and_the_slice_plan_need_no_gpu():
    """Every refusal of i2v_disc3d_create comes before the device is looked for; the slice plan is a pure function of the shape."""
    for bad, word in ((dict(channels=[64, 64, 120, 256, 512]), "multiple of 16"), (dict(stride_s=[1, 3, 2, 2]), "outside {1, 2}"),
                      (dict(stride_t=[0, 2, 2, 2]), "outside {1, 2}"), (dict(res_type=34), "resnet18")):
        rc, h, msg = _create(**bad)
        assert rc == -1 and not h and word in msg, (bad, msg)
    with pytest.raises(i2v_native.I2VError):
        i2v_native.disc3d_wgrad_plan(24, 16, 100)
    with pytest.raises(i2v_native.I2VError):
        i2v_native.disc3d_wgrad_plan(16, 16, 100, taps=64)
    for case in tc.wgrad_cases():
        _, _, g, _ = tc.conv_case_inputs(case)
        p = g.shape[0] * int(np.prod(g.shape[2:]))
        s, l = i2v_native.disc3d_wgrad_plan(case["cout"], case["cin"], p, taps=3 * case.get("k", 3) ** 2)
        assert s == case["slices"] and l % 16 == 0 and (s - 1) * l < p <= s * l, (case["id"], p, s, l)
        assert (s, l) == i2v_native.disc3d_wgrad_plan(case["cout"], case["cin"], p, taps=3 * case.get("k", 3) ** 2)
    for cout, cin, p in ((64, 3, 122880), (512, 256, 160), (16, 16, 1), (48, 32, 72)):
        s, l = i2v_native.disc3d_wgrad_plan(cout, cin, p, taps=147 if cin == 3 else 27)
        assert l % 16 == 0 and (s - 1) * l < p <= s * l
    assert i2v_native.lib().i2v_disc3d_unit_workspace_bytes(0, 1, 4, 4, 16, 16, 0) == 0
    assert i2v_native.lib().i2v_disc3d_unit_workspace_bytes(1, 1, 4, 4, 16, 16, 0) > 0
    assert i2v_native.lib().i2v_disc3d_saved_bytes(None, 1, 12, 64, 64) == 0
    from stage1_VAE.modules.resnet3D import Discriminator
    with pytest.raises(NotImplementedError, match="not built"):
        Discriminator(dict(tc.CFG_A, res_type_encoder="resnet34"))
    with pytest.raises(i2v_native.I2VError):
        Discriminator(dict(tc.CFG_A, channels=[16, 16, 24, 32, 32]))
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        Discriminator(dict(tc.CFG_A))(torch.zeros(1, 3, 12, 64, 64))
    import i2v_train
    with pytest.raises(NotImplementedError, match="double backward"):
        i2v_train.TemporalDiscTrainer(Discriminator(dict(tc.CFG_A)), w_GP=10)


def test_state_dict_is_the_reference_layout_and_the_init_is_the_reference_draw(fxa):
    from stage1_VAE.modules.resnet3D import Discriminator
    net = Discriminator(dict(tc.CFG_SHIPPED))
    want = tc.state_keys(tc.CFG_SHIPPED)
    assert {k: (tuple(v.shape), v.dtype) for k, v in net.state_dict().items()} == want and list(net.state_dict()) == list(want)
    assert sum(k.endswith("weight_orig") for k in want) == 12
    assert {k for k, _ in net.named_parameters()} == {k for k in want if not k.endswith(("weight_u", "weight_v"))}
    plain = Discriminator(dict(tc.CFG_SHIPPED, spectral_norm=False))
    assert sum(k.endswith("weight_orig") for k in plain.state_dict()) == 4 and "layer.0.0.conv1.weight" in plain.state_dict()
    _, ref, _ = fxa
    torch.manual_seed(tc.SEED_A)
    small = Discriminator(dict(tc.CFG_A))
    assert list(small.state_dict()) == list(tc.state_keys(tc.CFG_A)) and set(small.state_dict()) == set(ref)
    for k, v in small.state_dict().items():
        if v.dim() == 5:          # every conv: the orthogonal draw (a QR, compared to 1e-6).  It reaches weight_orig too: on a wrapped
            assert rel(v, ref[k]) < 1e-6, k          # conv the reference's m.weight is weight_orig.data, initialised in place
        else:                     # u, v, norms, fc (nn.Linear's default init): bit for bit
            assert torch.equal(v, ref[k]), k
    small.load_state_dict(ref)


def test_module_copies_and_pickles_without_its_handle():
    import copy
    import pickle
    from stage1_VAE.modules.resnet3D import Discriminator
    net = Discriminator(dict(tc.CFG_A))
    object.__setattr__(net, "_native", object())
    twin = copy.deepcopy(net)
    assert twin._native is None
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(twin.state_dict().values(), net.state_dict().values()))
    object.__setattr__(net, "_native", None)
    back = pickle.loads(pickle.dumps(net))
    assert back._native is None and list(back.state_dict()) == list(net.state_dict())


def test_encoder_classes_are_untouched():
    """BasicBlock and Encoder, from ``class BasicBlock`` to the end of ``Encoder.forward``, are the text they were before the Discriminator
    was added below them (its SHA-256), and the Discriminator's block class is its own."""
    import hashlib
    from stage1_VAE.modules import resnet3D
    src = open(resnet3D.__file__).read()
    part = src[src.index("class BasicBlock(_NoForward)"):src.index("# ------", src.index("class Encoder(NativeBacked)"))]
    assert part.rstrip().endswith("return self.native().forward(x, eps)")
    assert hashlib.sha256(part.rstrip().encode()).hexdigest() == ENCODER_TEXT_SHA256
    assert resnet3D.DiscBasicBlock is not resnet3D.BasicBlock
