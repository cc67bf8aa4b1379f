"""CPU checks of the Generator's training path (stage1_VAE/modules/decoder.py ``Generator.differentiable`` on csrc/i2v_gen_train.hip): the
float64 oracle of tests/gen_train_common.py, with the backwards of fc, the up-samplings and the image head written out by hand, against the
fixtures made from the reference's own Generator; every deliberate error against the gate the GPU tests apply; the C ABI of
include/i2v_hip_gen_train.h against i2v_native.GEN_TRAIN_SYMBOLS; the Makefile's lists; the state dict; the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gen_train_common as gt
import i2v_native
import test_host_abi as abi
from test_host_encoder_train import parse_header

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")


@pytest.fixture(scope="module")
def golden():
    return gt.load_golden()


@pytest.fixture(scope="module")
def oracle():
    """Per fixture the float64 oracle's result, computed once and shared."""
    out = {}
    for tag in gt.FIXTURES:
        case = gt.CASES[tag]
        img, z, c = gt.inputs(case)
        out[tag] = gt.generator(gt.synthetic_state(case), img, z, case, c)
    return out


@pytest.mark.parametrize("tag", gt.FIXTURES)
def test_hand_written_backward_matches_the_reference_fixture(golden, oracle, tag):
    r, case = oracle[tag], gt.CASES[tag]
    assert tuple(r["out"].shape) == gt.out_shape(case) == golden[f"{tag}.out"].shape
    assert gt.rel(r["out"], golden[f"{tag}.out"]) < 1e-9 and gt.rel(r["dz"], golden[f"{tag}.dz"]) < 1e-9
    keys = {k for k in gt.param_shapes(case) if not gt.gc.is_buffer(k)}
    assert set(r["grads"]) == keys
    full = {k for k in keys if k in gt.FULL_GRADS or gt.is_zero_grad(k)}
    assert {k[len(tag) + 3:] for k in golden if k.startswith(tag + ".g.")} == full
    assert {k[len(tag) + 3:] for k in golden if k.startswith(tag + ".n.")} == keys - full == {k[len(tag) + 3:] for k in golden if k.startswith(tag + ".p.")}
    worst = 0.0
    for k in sorted(keys):
        if k in full:
            d = gt.rel(r["grads"][k], golden[f"{tag}.g.{k}"], r["scale"].get(k))
        else:
            d = gt.check_summary(k, r["grads"][k], golden, tag, 1e-9)
        worst = max(worst, d)
    print(f"fixture {tag}: worst parameter gradient against the reference's float64 run {worst:.2e}")
    assert worst < 1e-9


def test_the_gradients_of_conv_0_bias_are_zero_and_held_on_their_own_scale(golden, oracle):
    for tag in gt.FIXTURES:
        zero = [k for k in oracle[tag]["grads"] if gt.is_zero_grad(k)]
        assert len(zero) == 6
        for k in zero:
            assert np.abs(golden[f"{tag}.g.{k}"]).max() < 1e-10 * float(oracle[tag]["scale"][k].max())


def test_gates_come_from_the_reference_s_own_fp32_run(golden):
    """1e-4 where the reference's fp32 run stays a factor four inside it (the frames do), else four times its distance; the recorded worst
    figures are those written next to TOL_L2."""
    for tag, (worst, key) in gt.REF_FP32.items():
        d32 = {k[len(tag) + 5:]: float(v) for k, v in golden.items() if k.startswith(tag + ".d32.")}
        assert len(d32) == 2 + len([k for k in gt.param_shapes(gt.CASES[tag]) if not gt.gc.is_buffer(k)])
        assert d32["out"] <= gt.TOL_L2 / 4 and gt.gate_of(golden, tag, "out") == gt.TOL_L2
        top = max(d32.items(), key=lambda kv: kv[1])
        assert top[0] == "g." + key and abs(top[1] - worst) <= 0.01 * worst
        assert gt.gate_of(golden, tag, top[0]) == 4 * top[1]
        assert all(gt.gate_of(golden, tag, k) == gt.TOL_L2 for k, v in d32.items() if v <= gt.TOL_L2 / 4)
    dist = np.abs(golden["a.sgd_losses_f32"] - golden["a.sgd_losses"]) / golden["a.sgd_scale"]
    print("the reference's fp32 SGD losses against float64, on the scale sum |c frames|:", dist)
    assert len(golden["a.sgd_losses"]) == gt.SGD_STEPS == len(set(np.round(golden["a.sgd_losses"], 6))) and dist.max() <= gt.TOL_L2 / 4


def test_header_matches_the_sixth_table():
    funcs, structs = parse_header("i2v_hip_gen_train.h")
    assert set(funcs) == set(i2v_native.GEN_TRAIN_SYMBOLS) and len(funcs) == 18 and structs == []
    assert abi.compare_functions(funcs, i2v_native.GEN_TRAIN_SYMBOLS) == []
    assert all(n.startswith("i2v_gen_train_") for n in funcs)
    res, args = i2v_native.GEN_TRAIN_SYMBOLS["i2v_gen_train_head_backward"]
    assert abi.compare_functions(funcs, dict(i2v_native.GEN_TRAIN_SYMBOLS, i2v_gen_train_head_backward=(res, args[:-1]))) != []
    other = (set(i2v_native.SYMBOLS) | set(i2v_native.DISC_SYMBOLS) | set(i2v_native.DISC3D_SYMBOLS) | set(i2v_native.ENC3D_TRAIN_SYMBOLS)
             | set(i2v_native.GBLOCK_TRAIN_SYMBOLS))
    assert not other & set(funcs)
    lib = i2v_native.lib()
    assert all(hasattr(lib, n) for n in funcs)


def test_makefile_lists_the_source_and_the_header():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_gen_train.hip" in mk.split("SRCS =")[1].splitlines()[0].split()
    hdrs = mk.split("HDRS =")[1].splitlines()[0].split()
    assert "../../include/i2v_hip_gen_train.h" in hdrs and "i2v_res3d_trunk.h" in hdrs and "i2v_train_conv.h" in hdrs


@pytest.mark.parametrize("tag", sorted(gt.CASES))
def test_keys_are_those_of_the_module_s_state_dict(tag):
    from stage1_VAE.modules.decoder import Generator
    case = gt.CASES[tag]
    net = Generator(gt.dic_of(case))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == gt.param_shapes(case)
    assert net.differentiable is False and not any(b.differentiable for b in net._blocks())
    assert set(net._glue_params()) == set(net._GLUE_KEYS) == {"fc.weight", "fc.bias", "conv_img.weight", "conv_img.bias"}
    header = open(os.path.join(REPO, "include", "i2v_hip_gen_train.h")).read()
    assert "fc.{weight,bias}" in header and "conv_img.{weight,bias}" in header
    net.differentiable = True
    assert all(b.differentiable for b in net._blocks())
    with pytest.raises(i2v_native.I2VError, match="HIP device"):
        net(torch.zeros(1, 3, 8, 8), torch.zeros(1, case["z_dim"]))
    net.differentiable = False
    assert not any(b.differentiable for b in net._blocks()) and net.__dict__["_native"] is None


def test_module_copies_and_pickles_without_its_handles():
    import copy
    import pickle
    from stage1_VAE.modules.decoder import Generator
    net = Generator(gt.dic_of(gt.CASES["a"]))
    net.differentiable = True
    for m in (net, net.g_0):                                  # stand-ins for live handles
        object.__setattr__(m, "_train_native", object())
        object.__setattr__(m, "_native", object())
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert twin.differentiable and all(b.differentiable for b in twin._blocks())
        for m in (twin, twin.g_0):
            assert m.__dict__["_train_native"] is None and m.__dict__["_native"] is None
        assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), net.state_dict().values()))
        twin.load_state_dict(net.state_dict())               # the load hook came along


@pytest.mark.parametrize("args, word", [((8, 8), "multiple of 16"), ((24, 8), "multiple of 16"), ((80, 8), "16 nf <= 1024"), ((0, 8), "multiple of 16"),
                                        ((16, 0), "z_dim"), ((64, -2), "z_dim")])
def test_create_refuses_before_a_device_is_looked_for(args, word):
    lib = i2v_native.lib()
    h = ctypes.c_void_p()
    assert lib.i2v_gen_train_create(*args, ctypes.byref(h)) == -1 and not h.value
    assert word in lib.i2v_last_error().decode()


def test_sizes_of_a_bad_shape_are_zero():
    lib = i2v_native.lib()
    assert lib.i2v_gen_train_head_saved_bytes(16, 1, 1, 4, 4) > 0 and lib.i2v_gen_train_head_workspace_bytes(16, 1, 1, 4, 4) > 0
    for bad in ((24, 1, 1, 4, 4), (16, 0, 1, 4, 4), (16, 1, 1, 0, 4), (2048, 1, 1, 4, 4)):
        assert lib.i2v_gen_train_head_saved_bytes(*bad) == 0 and lib.i2v_gen_train_head_workspace_bytes(*bad) == 0
    assert lib.i2v_gen_train_fc_workspace_bytes(3, 4096, 8) >= 3 * 16 * 8 * 8 and lib.i2v_gen_train_fc_workspace_bytes(0, 4096, 8) == 0
    assert lib.i2v_gen_train_fc_workspace_bytes(3, 0, 8) == 0 and lib.i2v_gen_train_fc_slices(4096) == 16 and lib.i2v_gen_train_fc_slices(0) == 0
    assert lib.i2v_gen_train_fc_slices(257) == 2


# ---------------------------------------------------------------------------------------------------------------- what the gates catch

def _head_case():
    rng = np.random.default_rng(61)
    nf, B, thw = 16, 2, (3, 5, 6)
    x = torch.from_numpy(rng.standard_normal((B, nf) + thw).astype(np.float32))
    x[torch.from_numpy(rng.uniform(size=tuple(x.shape)) < 0.1)] = 0.0
    w = torch.from_numpy((rng.standard_normal((3, nf, 3, 3, 3)) * 0.5 / np.sqrt(27 * nf)).astype(np.float32))
    b = torch.from_numpy((0.2 * rng.standard_normal(3)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B, thw[0], 3) + thw[1:]).astype(np.float32))
    return x, w, b, g, 27 * nf + 4


@pytest.mark.parametrize("error", ["no_tanh_grad", "slope_at_zero", "no_flip"])
def test_deliberate_errors_in_the_head_land_above_the_gate(error):
    x, w, b, g, n = _head_case()
    y = gt.head_forward_ref(x, w, b)[0].float()
    r = gt.head_backward_ref(x, w, g, y)
    ok, ratio, _ = gt.gate(r["dx"].float(), r["dx"], r["S_dx"], n)
    assert ok and ratio <= 1.0, "the float64 result rounded to fp32 passes its own gate"
    bad = gt.head_backward_ref(x, w, g, y, **{error: 1.0 if error == "slope_at_zero" else True})
    ok, ratio, l2 = gt.gate(bad["dx"].float(), r["dx"], r["S_dx"], n)
    print(f"head {error}: |err| / bound {ratio:.1f}, rel-L2 {l2:.2e}")
    assert not ok and ratio > 10


def test_the_adjoint_as_a_mean_lands_above_the_gate():
    rng = np.random.default_rng(62)
    for ut, us in ((2, 2), (1, 2), (2, 1), (4, 4)):
        g = torch.from_numpy(rng.standard_normal((2, 16, 3 * ut, 5 * us, 6 * us)))
        ref, S, n = gt.upsample_backward(g, ut, us), gt.upsample_backward(g.abs(), ut, us), ut * us * us - 1
        assert gt.gate(ref.float(), ref, S, n)[0]
        ok, ratio, l2 = gt.gate(gt.upsample_backward(g, ut, us, mean=True).float(), ref, S, n)
        print(f"adjoint as a mean ({ut}, {us}, {us}): |err| / bound {ratio:.1f}, rel-L2 {l2:.2e}")
        assert not ok and ratio > 10
    x = torch.from_numpy(rng.standard_normal((1, 2, 2, 3, 3)))
    assert torch.equal(gt.upsample(x, 2, 4), torch.nn.functional.interpolate(x, scale_factor=(2, 4, 4)))
    assert float((gt.upsample(x, 2, 4) * g[:1, :2, :4, :12, :12]).sum() - (x * gt.upsample_backward(g[:1, :2, :4, :12, :12], 2, 4)).sum()) < 1e-9


def test_fc_s_term_missing_from_motion_grad_lands_above_the_gate(golden, oracle):
    for tag in gt.FIXTURES:
        r = oracle[tag]
        gate = gt.gate_of(golden, tag, "dz")
        d = gt.rel(r["dz_blocks"], r["dz"])
        print(f"fixture {tag}: motion.grad without fc's term: rel-L2 {d:.2e} against the gate {gate:.1e}")
        assert gt.rel(r["dz"].float(), r["dz"]) <= gate and d > 10 * gate
