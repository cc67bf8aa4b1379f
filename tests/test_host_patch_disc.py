"""CPU checks of the patch discriminator (stage1_VAE/modules/patch_disc.py on csrc/i2v_patchdisc.hip): the float64 oracle of
tests/patch_disc_common.py against the fixture made from the reference's own module and against torch autograd; every deliberate error
against the gate the GPU tests apply; the C ABI of include/i2v_hip_disc.h against i2v_native.DISC_SYMBOLS; the refusals; the state dict."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i2v_native
import patch_disc_common as pc
import test_host_abi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
GOLDEN = os.path.join(REPO, "tests", "golden")
LAYERS = pc.spec(16, 3)


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
    """Other modules of the suite switch grad mode off for the process; two tests here compare with autograd."""
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


@pytest.fixture(scope="module")
def train_pass(fx):
    """The fixture's training step through the oracle: fake first (it initialises ActNorm), then real on the updated state."""
    main, _ = fx
    sd = params_of(main)
    fake, real = pc.train_inputs()
    pf, cf = pc.forward_oracle(sd, fake, LAYERS, training=True, init=True)
    sd2 = dict(sd, **cf["state"])
    pr, cr = pc.forward_oracle(sd2, real, LAYERS, training=True)
    return sd, fake, real, pf, cf, pr, cr


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def step_grads(cf, cr, pf, pr, mutate=None):
    df, dr = pc.hinge_disc_grads(pf, pr)
    gf, dxf = pc.backward_oracle(cf, df, mutate)
    gr, dxr = pc.backward_oracle(cr, dr, mutate)
    return {k: gf[k] + gr[k] for k in gf}, dxf, dxr


def test_oracle_reproduces_the_reference_fixture(fx, train_pass):
    main, grads = fx
    sd, fake, real, pf, cf, pr, cr = train_pass
    assert rel(pf, main["train_pred_fake"]) < 1e-12 and rel(pr, main["train_pred_real"]) < 1e-12
    assert abs(float(pc.hinge_disc(pf, pr)) - float(main["train_loss"])) < 1e-13
    after = dict(cf["state"], **cr["state"])
    for k, v in after.items():
        assert rel(v, main["after." + k]) < 1e-12, k
    g, dxf, dxr = step_grads(cf, cr, pf, pr)
    assert set(g) == set(grads)
    for k in g:
        assert rel(g[k], grads[k]) < 2e-7, k          # the fixture's gradients are rounded to fp32
    assert rel(dxf, main["train_dx_fake"]) < 1e-11 and rel(dxr, main["train_dx_real"]) < 1e-11
    sd_eval = dict(sd, **after)
    for tag in pc.EVAL_SHAPES:
        pred, _ = pc.forward_oracle(sd_eval, pc.eval_inputs(tag), LAYERS, training=False)
        assert rel(pred, main["eval_" + tag]) < 1e-12, tag


def test_loss_sequence_of_the_fixture_is_the_recorded_one(fx):
    main, _ = fx
    assert np.allclose(main["sgd_losses"], pc.ISSUE_LOSSES, rtol=0, atol=1.5e-6)
    assert np.allclose(main["sgd_losses_f32"], main["sgd_losses"], rtol=0, atol=1.5e-6)
    assert all(b < a for a, b in zip(main["sgd_losses"], main["sgd_losses"][1:]))


def test_oracle_sgd_steps_follow_the_fixture(fx):
    main, _ = fx
    sd = {k: v.double() for k, v in params_of(main).items()}
    fake, real = pc.train_inputs()
    for step in range(pc.SGD_STEPS):
        pf, cf = pc.forward_oracle(sd, fake, LAYERS, training=True, init=step == 0)
        sd = dict(sd, **cf["state"])
        pr, cr = pc.forward_oracle(sd, real, LAYERS, training=True)
        sd = dict(sd, **cr["state"])
        assert abs(float(pc.hinge_disc(pf, pr)) - main["sgd_losses"][step]) < 1e-12
        g, _, _ = step_grads(cf, cr, pf, pr)
        for k in g:
            sd[k] = sd[k] - pc.SGD_LR * g[k].reshape(sd[k].shape)


def test_spectral_norm_gradient_formula_against_autograd():
    """One conv under torch.nn.utils.spectral_norm in float64: the hand formula equals autograd to 1e-13, and differs visibly without the projection."""
    torch.manual_seed(5)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(16, 32, 4, 2, 1)).double().train()
    x = torch.randn(2, 16, 9, 13, dtype=torch.float64)
    W, u0, v0 = conv.weight_orig.detach().clone(), conv.weight_u.clone(), conv.weight_v.clone()
    y = conv(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    u, v, sigma = pc.power_iteration(W.reshape(32, -1), u0, v0)
    assert rel(u, conv.weight_u) < 1e-14 and rel(v, conv.weight_v) < 1e-14
    dW, _, _, _ = pc.wgrad_oracle(gy, x, W, None, None, 2, u, v, sigma)
    assert rel(dW, conv.weight_orig.grad) < 1e-13
    dropped, _, _, _ = pc.wgrad_oracle(gy, x, W, None, None, 2, u, v, sigma, mutate="projection_dropped")
    assert rel(dropped, conv.weight_orig.grad) > 1e-3


def test_dgrad_by_taps_is_the_transposed_convolution():
    from torch.nn.grad import conv2d_input
    for stride, hw in ((2, (9, 13)), (2, (8, 8)), (1, (6, 7))):
        g, w, _, _ = pc.dgrad_inputs({"cin": 16, "cout": 48, "hw": hw, "batch": 2, "stride": stride, "seed": 7})
        ref = conv2d_input((2, 16) + hw, w.double(), g.double(), stride=stride, padding=1)
        assert rel(pc.dgrad_taps(g.double(), w.double(), hw, stride), ref) < 1e-14


def test_actnorm_init_is_the_reference_rule():
    y = pc.randn(3, (4, 8, 5, 6)).double() * 2 + 1
    loc, scale = pc.actnorm_init(y)
    flat = y.permute(1, 0, 2, 3).reshape(8, -1)
    assert torch.allclose(loc, -flat.mean(1)) and torch.allclose(scale, 1 / (flat.std(1) + 1e-6))
    h = scale.view(1, -1, 1, 1) * (y + loc.view(1, -1, 1, 1))
    assert h.mean((0, 2, 3)).abs().max() < 1e-12 and (h.permute(1, 0, 2, 3).reshape(8, -1).std(1) - 1).abs().max() < 1e-5


def test_every_deliberate_error_exceeds_the_gate(fx, train_pass):
    """The module gate (rel-L2 <= 1e-4 per tensor) rejects each error on the fixture's training step; printed with -s."""
    main, _ = fx
    sd, fake, real, pf, cf, pr, cr = train_pass
    ref, dxf, _ = step_grads(cf, cr, pf, pr)
    worst = {}
    for m in pc.MUTATIONS:
        if m == "biased_std":
            _, cm = pc.forward_oracle(sd, fake, LAYERS, training=True, init=True, mutate=m)
            worst[m] = max(rel(cm["state"][k], cf["state"][k]) for k in cf["state"] if k.endswith("scale"))
            continue
        if m == "mask_wrong_side_of_scale":   # needs a negative scale: flip one channel of every ActNorm behind the init
            state = dict(sd, **cf["state"])
            for k in [k for k in state if k.endswith("scale")]:
                state[k] = state[k] * (1.0 - 2.0 * (torch.arange(state[k].numel()) == 0)).view_as(state[k])
            pn, cn = pc.forward_oracle(state, real, LAYERS, training=True)
            d = torch.ones_like(pn) / pn.numel()
            (g0, x0), (g1, x1) = pc.backward_oracle(cn, d), pc.backward_oracle(cn, d, mutate=m)
            worst[m] = max(max(rel(g1[k], g0[k]) for k in g0), rel(x1, x0))
            continue
        g, dx, _ = step_grads(cf, cr, pf, pr, mutate=m)
        worst[m] = max(max(rel(g[k], ref[k]) for k in ref), rel(dx, dxf))
    print("smallest-gate factors:", {k: f"{v / pc.TOL_L2:.1f}x" for k, v in worst.items()})
    assert set(worst) == set(pc.MUTATIONS)
    for m, v in worst.items():
        assert v > 10 * pc.TOL_L2, (m, v)


def test_unit_gates_reject_the_unit_errors():
    """The element-wise gates of the dgrad and wgrad units reject their deliberate errors on the cases the GPU test runs."""
    for case in pc.conv_cases()[::7]:
        g, w, act, scale = pc.dgrad_inputs(case)
        ref, S, n = pc.dgrad_oracle(g, w, act, scale, case["hw"], case["stride"])
        for m in ("dgrad_not_flipped", "dgrad_wrong_parity"):
            if m == "dgrad_wrong_parity" and case["stride"] == 1:
                continue
            bad, _, _ = pc.dgrad_oracle(g, w, act, scale, case["hw"], case["stride"], mutate=m)
            assert not pc.gate(bad.float(), ref, S, n)[0], (case["id"], m)
        assert pc.gate(ref.float(), ref, S, n)[0]
    case = pc.wgrad_cases()[0]
    x, w, _, _, _ = pc.conv_inputs(case)
    g, _, act, scale = pc.dgrad_inputs(case)
    u, v, sigma = pc.power_iteration(w.double().reshape(w.shape[0], -1), pc.randn(1, (w.shape[0],)).double(), pc.randn(2, (w[0].numel(),)).double())
    ref, _, bound, _ = pc.wgrad_oracle(g, x, w, act, scale, case["stride"], u, v, sigma)
    bad, _, _, _ = pc.wgrad_oracle(g, x, w, act, scale, case["stride"], u, v, sigma, mutate="projection_dropped")
    assert pc.gate_bound(ref.float(), ref, bound)[0] and not pc.gate_bound(bad.float(), ref, bound)[0]


def test_fp32_masks_equal_float64_masks_on_the_committed_seeds(fx, train_pass):
    """Plain fp32 torch against float64 on the fixture's inputs: no LeakyReLU mask differs (the seeds were kept because none does)."""
    main, _ = fx
    sd, fake, real, _, cf, _, cr = train_pass
    sd32 = {k: v.float() for k, v in sd.items()}
    x, init = {"fake": fake, "real": real}, {"fake": True, "real": False}
    state32 = dict(sd32)
    for name, c64 in (("fake", cf), ("real", cr)):
        h = x[name]
        for st in c64["steps"][:-1]:
            l = st["layer"]
            m = f"main.{l['key']}."
            W = state32[m + "weight_orig"]
            u, v, sigma = pc.power_iteration(W.reshape(W.shape[0], -1), state32[m + "weight_u"], state32[m + "weight_v"])
            state32[m + "weight_u"], state32[m + "weight_v"] = u, v
            y = F.conv2d(h, W / sigma, state32[m + "bias"], stride=l["stride"], padding=1)
            if l["norm"] is not None:
                a = f"main.{l['norm']}."
                if init[name]:
                    loc, scale = pc.actnorm_init(y)
                    state32[a + "loc"], state32[a + "scale"] = loc, scale
                y = state32[a + "scale"].view(1, -1, 1, 1) * (y + state32[a + "loc"].view(1, -1, 1, 1))
            assert y.dtype == torch.float32
            assert pc.fragile_units(y > 0, st["h"]) == (0, 0), (name, l["key"])
            h = torch.where(y > 0, y, 0.2 * y)


def parse_disc_header():
    text = open(os.path.join(REPO, "include", "i2v_hip_disc.h")).read()
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


def test_disc_header_matches_the_second_table_and_the_first_is_untouched():
    funcs, structs = parse_disc_header()
    assert set(funcs) == set(i2v_native.DISC_SYMBOLS) and len(funcs) == 19
    assert abi.compare_functions(funcs, i2v_native.DISC_SYMBOLS) == []
    assert all(n.startswith("i2v_patchdisc_") for n in funcs)
    (body, name), = structs
    assert name == "i2v_patchdisc_cfg"
    fields = [f.strip() for d in body.split(";") if d.strip() for f in d.split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in i2v_native.PatchDiscCfg._fields_] and all(t is ctypes.c_int32 for _, t in i2v_native.PatchDiscCfg._fields_)
    res, args = i2v_native.DISC_SYMBOLS["i2v_patchdisc_forward"]
    assert abi.compare_functions(funcs, dict(i2v_native.DISC_SYMBOLS, i2v_patchdisc_forward=(res, args[:-1]))) != []
    main_funcs, main_structs = abi.parse_header()
    assert set(main_funcs) == set(i2v_native.SYMBOLS) and len(main_funcs) == 129 and len(main_structs) == 8
    assert not set(main_funcs) & set(funcs)
    if os.path.exists(i2v_native.LIB_PATH):
        lib = ctypes.CDLL(i2v_native.LIB_PATH)
        assert all(hasattr(lib, n) for n in funcs)


def test_source_is_built_and_reads_no_environment():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_patchdisc.hip" in mk.split("SRCS =")[1].splitlines()[0]
    hdrs = mk.split("HDRS =")[1].splitlines()[0].split()
    assert "../../include/i2v_hip_disc.h" in hdrs and "i2v_train_conv.h" in hdrs
    src = open(os.path.join(PKG, "csrc", "i2v_patchdisc.hip")).read()
    conv = open(os.path.join(PKG, "csrc", "i2v_train_conv.h")).read()
    for text in (src, conv):
        assert "getenv" not in text and "atomic" not in text.lower()
    assert '#include "i2v_train_conv.h"' in src and "mfma_f32_16x16x4f32" in conv
    assert "a_lds" not in src and "a_lds" in conv      # the staged-GEMM loop is the shared header's


def test_refusals_need_no_gpu():
    """Every refusal of i2v_patchdisc_create comes before the device is looked for; the plan refuses what the kernels do not take."""
    if not os.path.exists(i2v_native.LIB_PATH):
        pytest.skip("library not built")
    lib = i2v_native.lib()
    for bad, word in ((dict(ndf=24), "multiple of 16"), (dict(in_channels=1), "in_channels"), (dict(use_actnorm=0), "not built"), (dict(n_layers=0), "n_layers")):
        cfg = i2v_native.PatchDiscCfg(**dict(dict(in_channels=3, ndf=64, n_layers=3, use_actnorm=1, spectral_norm=1), **bad))
        h = ctypes.c_void_p()
        assert lib.i2v_patchdisc_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h
        assert word in lib.i2v_last_error().decode()
    with pytest.raises(i2v_native.I2VError):
        i2v_native.patchdisc_wgrad_plan(24, 16, 100)
    assert i2v_native.patchdisc_wgrad_plan(512, 256, 980) == (2, 496)
    for cout, cin, p in ((64, 3, 20480), (128, 64, 5120), (16, 16, 1), (1, 512, 720), (48, 16, 72)):
        s, l = i2v_native.patchdisc_wgrad_plan(cout, cin, p)
        assert l % 16 == 0 and (s - 1) * l < p <= s * l
    from stage1_VAE.modules.patch_disc import NLayerDiscriminator
    with pytest.raises(NotImplementedError, match="not built"):
        NLayerDiscriminator(dict(pc.FIXTURE_CFG, use_actnorm=False))
    with pytest.raises(i2v_native.I2VError):
        NLayerDiscriminator(dict(pc.FIXTURE_CFG, ndf=24))
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        NLayerDiscriminator(dict(pc.FIXTURE_CFG))(torch.zeros(1, 3, 32, 32))


def test_state_dict_is_the_reference_layout_and_the_init_is_the_reference_draw(fx):
    from stage1_VAE.modules.patch_disc import ActNorm, NLayerDiscriminator, weights_init  # noqa: F401
    net = NLayerDiscriminator({"in_channels": 3, "ndf": 64, "n_layers": 3, "use_actnorm": True, "spectral_norm": True})
    want = pc.state_keys(64, 3)
    got = {k: (tuple(v.shape), v.dtype) for k, v in net.state_dict().items()}
    assert got == want
    assert sorted(k.split(".")[1] for k in want if k.endswith("bias")) == sorted(["0", "2", "5", "8", "11"], key=str)
    assert {k for k, _ in net.named_parameters()} == {k for k in want if k.endswith(("bias", "weight_orig", "loc", "scale"))}
    main, _ = fx
    torch.manual_seed(pc.SEED_MODULE)
    small = NLayerDiscriminator(dict(pc.FIXTURE_CFG))
    ref = params_of(main)
    assert list(small.state_dict()) == list(ref)
    for k, v in small.state_dict().items():
        assert torch.equal(v, ref[k]), k
    small.load_state_dict(ref)
    plain = NLayerDiscriminator(dict(pc.FIXTURE_CFG, spectral_norm=False))
    assert "main.0.weight" in plain.state_dict() and "main.0.weight_u" not in plain.state_dict()


def test_module_copies_and_pickles_without_its_host_state():
    """The native handle and the remembered ActNorm answer are host-side state: deepcopy and pickle drop them, load_state_dict forgets the answer."""
    import copy
    import pickle
    from stage1_VAE.modules.patch_disc import NLayerDiscriminator
    net = NLayerDiscriminator(dict(pc.FIXTURE_CFG))
    object.__setattr__(net, "_native", object())      # stands for a handle: copying it would be an error
    object.__setattr__(net, "_init_done", True)
    twin = copy.deepcopy(net)
    assert twin._native is None and twin._init_done is None and net._init_done is True
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(twin.state_dict().values(), net.state_dict().values()))
    object.__setattr__(net, "_native", None)
    back = pickle.loads(pickle.dumps(net))
    assert back._native is None and back._init_done is None and list(back.state_dict()) == list(net.state_dict())
    net.load_state_dict(back.state_dict())
    assert net._init_done is None


def test_backward_forward_still_raises():
    from stage1_VAE.modules.loss import Backward
    with pytest.raises(NotImplementedError) as e:
        Backward(None).forward(None, None, None, None, None, None, 0, None)
    for word in ("discriminators", "backward passes", "decoder", "encoder", "PatchDiscTrainer"):
        assert word in str(e.value)
