"""CPU checks of the motion encoder's training path (stage1_VAE/modules/resnet3D.py ``Encoder.differentiable`` on
csrc/i2v_encoder_train.hip): the float64 oracle of tests/encoder_train_common.py, with its backward written out by hand, against the
fixtures made from the reference's own module; every deliberate error against the gate the GPU tests apply; the C ABI of
include/i2v_hip_enc3d_train.h against i2v_native.ENC3D_TRAIN_SYMBOLS; the state dict; the refusals; the fragile band of the fp32
restatement."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

import encoder_train_common as ec
import i2v_native
import test_host_abi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = {"a": (ec.CFG_A, ec.CLIP_A, ec.SEED_A), "b": (ec.CFG_B, ec.CLIP_B, ec.SEED_B)}


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
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


def rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((torch.as_tensor(got).double() - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def oracle():
    """Per fixture: (state dict, inputs, the float64 oracle's full-loss result), computed once and shared."""
    out = {}
    for tag, (cfg, clip, seed) in FIXTURES.items():
        sd = ec.synthetic_state(cfg, seed)
        x, eps, *coefs = ec.inputs(cfg, clip, seed)
        out[tag] = (sd, (x, eps, coefs), ec.loss_and_grads(sd, x, eps, coefs, cfg))
    return out


@pytest.mark.parametrize("tag", ["a", "b"])
def test_hand_written_backward_matches_the_reference_fixture(oracle, tag):
    cfg, clip, seed = FIXTURES[tag]
    main, ref_grads = load(f"encoder_train_{tag}.npz"), load(f"encoder_train_{tag}_grads*.npz")
    sd, (x, eps, coefs), (loss, outs, grads, dx, _) = oracle[tag]
    assert set(ref_grads) == set(grads) == set(sd)
    for name, got in zip(("sample", "mu", "logvar"), outs):
        assert rel(got, main[name]) < 1e-12, name
    assert abs(float(loss) - float(main["loss"])) <= 1e-10 * abs(float(main["loss"]))
    assert abs(float(ec.kl_value(outs[1], outs[2])) - float(main["kl"])) <= 1e-10 * abs(float(main["kl"]))
    assert rel(dx, main["dx"]) < 1e-6                     # (the fixtures' gradients are rounded to fp32)
    worst = max((rel(grads[k], v), k) for k, v in ref_grads.items())
    print(f"fixture {tag}: worst parameter gradient {worst[1]} rel {worst[0]:.2e}")
    assert worst[0] < 1e-6, worst
    _, _, kgrads, kdx, _ = ec.loss_and_grads(sd, x, eps, coefs, cfg, kl_only=True)
    assert rel(kdx, main["kl.dx"]) < 1e-6
    kl_keys = [k[3:] for k in main if k.startswith("kl.") and k != "kl.dx"]
    assert "conv_mu.weight" in kl_keys and "conv_var.bias" in kl_keys and "conv1.weight" in kl_keys and "norm1.weight" in kl_keys
    for k in kl_keys:
        assert rel(kgrads[k], main["kl." + k]) < 1e-6, k


def test_sgd_sequence_of_the_oracle_is_the_reference_s(oracle):
    main = load("encoder_train_a.npz")
    sd, (x, eps, coefs), _ = oracle["a"]
    seq = ec.sgd_losses(sd, x, eps, coefs, ec.CFG_A, torch.float64)
    assert len(seq) == ec.SGD_STEPS == len(main["sgd_losses"])
    assert np.allclose(seq, main["sgd_losses"], rtol=1e-10, atol=0)
    assert len(set(np.round(main["sgd_losses"], 6))) == ec.SGD_STEPS          # the loss moves from step to step
    band = 4 * np.abs(main["sgd_losses_f32"] - main["sgd_losses"])
    print("SGD band 4 |fp32 - float64|:", band)


def parse_header(name):
    text = open(os.path.join(REPO, "include", name)).read()
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


def test_header_matches_the_fourth_table_and_the_other_three_are_untouched():
    funcs, structs = parse_header("i2v_hip_enc3d_train.h")
    assert set(funcs) == set(i2v_native.ENC3D_TRAIN_SYMBOLS) and len(funcs) == 14
    assert abi.compare_functions(funcs, i2v_native.ENC3D_TRAIN_SYMBOLS) == []
    assert all(n.startswith("i2v_enc3d_") for n in funcs)
    (body, name), = structs
    assert name == "i2v_enc3d_train_cfg"
    fields = [re.sub(r"\[\d+\]", "", f.strip()) for d in body.split(";") if d.strip() for f in d.split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in i2v_native.Enc3dTrainCfg._fields_]
    assert [getattr(t, "_length_", 0) for _, t in i2v_native.Enc3dTrainCfg._fields_] == [0, 5, 4, 4, 0]
    res, args = i2v_native.ENC3D_TRAIN_SYMBOLS["i2v_enc3d_train_backward"]
    assert abi.compare_functions(funcs, dict(i2v_native.ENC3D_TRAIN_SYMBOLS, i2v_enc3d_train_backward=(res, args[:-1]))) != []
    main_funcs, _ = abi.parse_header()
    disc3d_funcs, _ = parse_header("i2v_hip_disc3d.h")
    assert len(main_funcs) == 129 and len(i2v_native.DISC_SYMBOLS) == 19 and len(disc3d_funcs) == len(i2v_native.DISC3D_SYMBOLS) == 24
    for other in (main_funcs, i2v_native.SYMBOLS, i2v_native.DISC_SYMBOLS, i2v_native.DISC3D_SYMBOLS):
        assert not set(other) & set(funcs)
    assert os.path.exists(i2v_native.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(i2v_native.LIB_PATH)
    assert all(hasattr(lib, n) for n in funcs)


def test_sources_are_built_share_the_trunk_and_read_no_environment():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_encoder_train.hip" in mk.split("SRCS =")[1].splitlines()[0]
    hdrs = mk.split("HDRS =")[1].splitlines()[0].split()
    assert "../../include/i2v_hip_enc3d_train.h" in hdrs and "i2v_res3d_trunk.h" in hdrs and "i2v_train_conv.h" in hdrs
    enc = open(os.path.join(PKG, "csrc", "i2v_encoder_train.hip")).read()
    disc = open(os.path.join(PKG, "csrc", "i2v_disc3d.hip")).read()
    trunk = open(os.path.join(PKG, "csrc", "i2v_res3d_trunk.h")).read()
    conv = open(os.path.join(PKG, "csrc", "i2v_train_conv.h")).read()
    patch = open(os.path.join(PKG, "csrc", "i2v_patchdisc.hip")).read()
    for src in (enc, trunk, conv):
        assert "getenv" not in src and "atomic" not in src.lower()
    assert '#include "i2v_res3d_trunk.h"' in enc and '#include "i2v_res3d_trunk.h"' in disc and '#include "i2v_train_conv.h"' in trunk
    for kernel in ("conv_kernel", "dgrad_kernel", "wgrad_kernel"):      # one definition, in the header shared with the patch discriminator
        assert conv.count(f"void tc_{kernel}(") == 1
        for src in (patch, trunk, disc, enc):
            assert not any(f"void {family}_{kernel}(" in src for family in ("tc", "d3", "pd")) and "a_lds" not in src
    for kernel in ("d3_gn_bwd_dx_kernel",):                             # one definition, in the trunk's header
        assert f"void {kernel}(" in trunk and f"void {kernel}(" not in disc and f"void {kernel}(" not in enc
    assert "mfma_f32_16x16x4f32" in enc
    # the plan, the layout and the two walks exist once, in i2v_res3d_net.h
    assert "i2v_res3d_net.h" in hdrs
    net = open(os.path.join(PKG, "csrc", "i2v_res3d_net.h")).read()
    assert "getenv" not in net and "atomic" not in net.lower()
    assert '#include "i2v_res3d_net.h"' in enc and '#include "i2v_res3d_net.h"' in disc
    for src in (enc, disc):
        for gone in ("struct D3Block", "struct E3Block", "D3Layout", "E3Layout", "e3_bound", "e3_refuse"):
            assert gone not in src, gone
    for launcher in ("launch_conv<Trunk3d>(", "launch_dgrad<Trunk3d>(", "launch_gn_bwd(", "launch_wgrad<Trunk3d>("):     # the discriminator's: its unit entry
        assert disc.count(launcher) == 1 and enc.count(launcher) == 0 and net.count(launcher) >= 1, launcher
    assert conv.count("hipLaunchKernelGGL((tc_pack_kernel<") == 1 and conv.count("void tc_pack_kernel(") == 1
    assert net.count("launch_pack<") == 1 and "launch_pack<" not in enc and "pack_kernel" not in enc + net + disc + patch
    assert disc.count("launch_pack<") == 1 and patch.count("launch_pack<") == 2      # (the patch discriminator's forward packs its own network)
    for src in (disc, patch):
        assert "launch_pack<" in src[src.index("int pack_unit("):src.index("}  // namespace", src.index("int pack_unit("))]
    assert "void d3_maxpool_kernel(" in trunk and "void d3_maxpool_kernel(" not in disc and "void d3_maxpool_kernel(" not in enc


def test_state_dict_keys_are_the_existing_encoder_s_and_the_reference_s():
    from stage1_VAE.modules.resnet3D import Encoder
    for cfg in (ec.CFG_A, ec.CFG_B, ec.CFG_SHIPPED):
        net = Encoder(dict(cfg))
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == ec.state_keys(cfg)
        assert list(net.state_dict()) == list(ec.state_keys(cfg))
        assert net.differentiable is False
    assert set(ec.synthetic_state(ec.CFG_A, ec.SEED_A)) == set(load("encoder_train_a_grads*.npz"))
    ref_keys = [str(k) for k in load("encoder_train_keys.npz")["halfrate_keys"]]
    assert ref_keys == list(ec.state_keys(ec.CFG_HALFRATE))


def test_module_copies_without_its_handles():
    import copy
    from stage1_VAE.modules.resnet3D import Encoder
    net = Encoder(dict(ec.CFG_B))
    net.differentiable = True
    object.__setattr__(net, "_native", object())
    object.__setattr__(net, "_train_native", object())
    twin = copy.deepcopy(net)
    assert twin._native is None and twin._train_native is None and twin.differentiable is True and type(twin) is Encoder
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(twin.state_dict().values(), net.state_dict().values()))
    net.differentiable = False                       # drops both handles (refresh_native)
    assert net._native is None and net._train_native is None and net.differentiable is False


def _create(**over):
    cfg = dict(z_dim=64, channels=[64, 128, 256, 512, 512], stride_s=[1, 2, 2, 2], stride_t=[1, 2, 2, 2], use_max_pool=0)
    cfg.update(over)
    c = i2v_native.Enc3dTrainCfg(cfg["z_dim"], (ctypes.c_int32 * 5)(*cfg["channels"]), (ctypes.c_int32 * 4)(*cfg["stride_s"]),
                                 (ctypes.c_int32 * 4)(*cfg["stride_t"]), cfg["use_max_pool"])
    h = ctypes.c_void_p()
    lib = i2v_native.lib()
    return lib.i2v_enc3d_train_create(ctypes.byref(c), ctypes.byref(h)), h, lib.i2v_last_error().decode()


def test_refusals_need_no_gpu():
    """Every refusal of i2v_enc3d_train_create comes before the device is looked for."""
    for bad, word in ((dict(channels=[64, 128, 250, 512, 512]), "multiple of 16"), (dict(stride_s=[1, 3, 2, 2]), "outside {1, 2}"),
                      (dict(stride_t=[0, 2, 2, 2]), "outside {1, 2}"), (dict(use_max_pool=1), "use_max_pool"), (dict(z_dim=0), "z_dim"),
                      (dict(channels=[64, 64, 128, 256, 512], stride_s=[1, 2, 2, 2], stride_t=[2, 2, 2, 2]),
                       "layer 0 has stride_t 2 with stride_s 1 and equal widths (64): no downsample branch exists for its half-rate residual")):
        rc, h, msg = _create(**bad)
        assert rc == -1 and not h and word in msg, (bad, msg)
    lib = i2v_native.lib()
    assert lib.i2v_enc3d_train_saved_bytes(None, 1, 16, 64, 64) == 0 and lib.i2v_enc3d_train_workspace_bytes(None, 1, 16, 64, 64) == 0
    assert lib.i2v_enc3d_head_workspace_bytes(0, 16, 8) == 0 and lib.i2v_enc3d_head_workspace_bytes(1, 24, 8) == 0
    assert lib.i2v_enc3d_head_workspace_bytes(3, 48, 5) > 0
    with pytest.raises(i2v_native.I2VError):
        i2v_native.NativeEnc3DTrain(8, [16, 16, 16, 16], [1, 1, 1, 1], [1, 1, 1, 1])
    from stage1_VAE.modules.resnet3D import Encoder
    with pytest.raises(ValueError, match="half-rate residual"):
        Encoder(dict(ec.CFG_HALFRATE))
    with pytest.raises(NotImplementedError):
        Encoder(dict(ec.CFG_A, use_max_pool=True))
    net = Encoder(dict(ec.CFG_B))
    net.differentiable = True
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        net(torch.zeros(*ec.CLIP_B))
    from stage1_VAE.modules.loss import Backward
    with pytest.raises(NotImplementedError, match="decoder") as info:
        Backward(None).forward(None, None, None, None, None, None, 0, None)
    assert "motion-encoder backward" in str(info.value) and "double backward" in str(info.value)


def _all_tensors(result):
    loss, outs, grads, dx, _ = result
    out = {"sample": outs[0], "mu": outs[1], "logvar": outs[2], "dx": dx}
    out.update({"grad." + k: v for k, v in grads.items()})
    return out


@pytest.mark.parametrize("mutation", ec.MUTATIONS)
def test_each_deliberate_error_exceeds_the_gate(oracle, mutation):
    """Fixture B's network; the stem's temporal stride on a two-frame clip, on which both strides end on the [1, 4, 4] map.  The
    downsample rule with the discriminator's stride_t term differs from the encoder's only on configurations that the encoder refuses
    (stride_t 2, stride_s 1, equal widths), so no run can show it: it shows in the list of keys, against the reference's own."""
    if mutation == "downsample_with_stride_t_term":
        ref_keys = [str(k) for k in load("encoder_train_keys.npz")["halfrate_keys"]]
        wrong = list(ec.state_keys(ec.CFG_HALFRATE, mutate=mutation))
        extra = sorted(set(wrong) - set(ref_keys))
        print(f"{mutation}: {len(extra)} keys the reference does not have: {extra}")
        assert extra == ["layer.0.0.downsample.0.weight", "layer.0.0.downsample.1.bias", "layer.0.0.downsample.1.weight"]
        for cfg in (ec.CFG_A, ec.CFG_B, ec.CFG_SHIPPED):
            assert ec.state_keys(cfg, mutate=mutation) == ec.state_keys(cfg)
        return
    cfg = ec.CFG_B
    sd = oracle["b"][0]
    if mutation == "stem_stride_t_1":
        x, eps, *coefs = ec.inputs(cfg, ec.CLIP_B2, ec.SEED_B + 50)
        good = _all_tensors(ec.loss_and_grads(sd, x, eps, coefs, cfg))
    else:
        x, eps, coefs = oracle["b"][1]
        good = _all_tensors(oracle["b"][2])
    bad = _all_tensors(ec.loss_and_grads(sd, x, eps, coefs, cfg, mutate=mutation))
    worst = max((rel(bad[k], good[k]), k) for k in good)
    print(f"{mutation}: {worst[1]} is off by rel-L2 {worst[0]:.2e} = {worst[0] / ec.TOL_L2:.0f} x the gate")
    assert worst[0] > 10 * ec.TOL_L2, worst


def test_mutated_head_oracles_exceed_the_unit_gate():
    """The head's unit oracles with the three head errors switched on, against the unit gate itself."""
    case = ec.head_cases()[4]
    emb, w_mu, b_mu, w_var, b_var, eps, d_s, d_m, d_l = ec.head_inputs(case)
    (mu, S, n), (lv, _, _) = ec.head_forward_oracle(emb, w_mu, b_mu, w_var, b_var)
    C = emb.shape[-1]
    swapped = emb.reshape(emb.shape[0], C, 16).permute(0, 2, 1).contiguous()
    (mu_bad, _, _), _ = ec.head_forward_oracle(swapped, w_mu, b_mu, w_var, b_var)
    ok, ratio, l2 = ec.gate(mu_bad, mu, S, n)
    print(f"head_layout_swapped: {ratio:.0f} x the bound, rel-L2 {l2:.2e}")
    assert not ok and ratio > 100
    good = ec.fold_oracle(mu, lv, eps, d_s, d_m, d_l, 0.7)
    for mutation in ("kl_half_dropped", "eps_missing_in_dlogvar"):
        bad = ec.fold_oracle(mu, lv, eps, d_s, d_m, d_l, 0.7, mutate=mutation)
        ok, ratio, l2 = ec.gate(bad[1], good[1], good[3], 1)
        print(f"{mutation}: {ratio:.0f} x the bound, rel-L2 {l2:.2e}")
        assert not ok and ratio > 100


def test_fp32_restatement_decides_as_float64_within_the_cap(oracle):
    """The condition on the fixtures' inputs: the fp32 restatement's ReLU decisions differ from float64's only inside the fragile band
    (FRAGILE_REL of the layer's rms), and in at most FRAGILE_MAX units per case."""
    for tag, (cfg, clip, seed) in FIXTURES.items():
        sd, (x, eps, coefs), (_, _, _, _, hi) = oracle[tag]
        _, _, _, lo = ec.forward_oracle(sd, x, eps, cfg, dtype=torch.float32)
        assert lo["margins"]["norm1"].dtype == torch.float32
        rep = ec.decision_report(lo["decisions"], hi)
        print(tag, "differing decisions:", {k: v for k, v in rep.items() if v[0]})
        assert sum(v[1] for v in rep.values()) == 0, (tag, rep)
        assert sum(v[0] for v in rep.values()) <= ec.FRAGILE_MAX, (tag, rep)
