"""CPU checks of the GeneratorBlock's training path (stage1_VAE/modules/decoder.py ``GeneratorBlock.differentiable`` on
csrc/i2v_gblock_train.hip): the float64 oracle of tests/gblock_train_common.py, with its backward written out by hand, against the fixtures
made from the reference's own module; every deliberate error against the gate the GPU tests apply; the C ABI of
include/i2v_hip_gblock_train.h against i2v_native.GBLOCK_TRAIN_SYMBOLS; the Makefile's lists; the state dict; the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gblock_train_common as gc
import i2v_native
import test_host_abi as abi
from test_host_encoder_train import parse_header

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")


@pytest.fixture(scope="module")
def golden():
    return gc.load_golden()


@pytest.fixture(scope="module")
def oracle():
    """Per fixture the float64 oracle's result, computed once and shared."""
    out = {}
    for tag, cfg in gc.FIXTURES.items():
        x, z, img, c = gc.inputs(cfg)
        out[tag] = gc.block(gc.synthetic_state(cfg), x, z, img, cfg, c)
    return out


@pytest.mark.parametrize("tag", sorted(gc.FIXTURES))
def test_hand_written_backward_matches_the_reference_fixture(golden, oracle, tag):
    r = oracle[tag]
    assert gc.rel(r["out"], golden[f"{tag}.out"]) < 1e-12
    assert gc.rel(r["dx"], golden[f"{tag}.dx"]) < 1e-6 and gc.rel(r["dz"], golden[f"{tag}.dz"]) < 1e-6   # (the fixtures' gradients are rounded to fp32)
    want = {k[len(tag) + 3:]: v for k, v in golden.items() if k.startswith(tag + ".g.")}
    assert set(want) == set(r["grads"]) == {k for k in gc.param_shapes(gc.FIXTURES[tag]) if not gc.is_buffer(k)}
    worst = max((gc.rel(r["grads"][k], v, r["scale"].get(k)), k) for k, v in want.items())
    print(f"fixture {tag}: worst parameter gradient {worst[1]} rel {worst[0]:.2e}")
    assert worst[0] < 1e-6, worst
    for k in r:
        if gc.is_buffer(k):
            assert gc.rel(r[k], golden[f"{tag}.{'u' if k.endswith('_u') else 'v'}.{k.rsplit('.', 1)[0]}"]) < 1e-12, k


def test_the_gradient_of_conv_0_bias_is_zero_and_is_held_on_its_own_scale(golden, oracle):
    for tag in gc.FIXTURES:
        g, scale = golden[f"{tag}.g.conv_0.bias"], oracle[tag]["scale"]["conv_0.bias"]
        assert np.abs(g).max() < 1e-10 * float(scale.max())
    assert gc.ZERO_GRADS == ("conv_0.bias",)


def test_sgd_sequence_of_the_oracle_is_the_reference_s(golden):
    cfg = gc.FIXTURES["a"]
    x, z, img, c = gc.inputs(cfg)
    seq = gc.sgd_outputs(gc.synthetic_state(cfg), x, z, img, c, cfg, torch.float64)
    assert len(seq) == gc.SGD_STEPS == len(golden["a.sgd_losses"])
    assert np.allclose(seq, golden["a.sgd_losses"], rtol=1e-9, atol=0)
    assert len(set(np.round(golden["a.sgd_losses"], 6))) == gc.SGD_STEPS          # the loss moves from step to step
    dist = np.abs(golden["a.sgd_losses_f32"] - golden["a.sgd_losses"]) / golden["a.sgd_scale"]
    print("the reference's fp32 SGD losses against float64, on the scale sum |c out|:", dist)
    assert dist.max() <= gc.TOL_L2 / 4


def test_header_matches_the_fifth_table():
    funcs, structs = parse_header("i2v_hip_gblock_train.h")
    assert set(funcs) == set(i2v_native.GBLOCK_TRAIN_SYMBOLS) and len(funcs) == 15 and structs == []
    assert abi.compare_functions(funcs, i2v_native.GBLOCK_TRAIN_SYMBOLS) == []
    assert all(n.startswith("i2v_gblock_train_") for n in funcs)
    res, args = i2v_native.GBLOCK_TRAIN_SYMBOLS["i2v_gblock_train_backward"]
    assert abi.compare_functions(funcs, dict(i2v_native.GBLOCK_TRAIN_SYMBOLS, i2v_gblock_train_backward=(res, args[:-1]))) != []
    other = set(i2v_native.SYMBOLS) | set(i2v_native.DISC_SYMBOLS) | set(i2v_native.DISC3D_SYMBOLS) | set(i2v_native.ENC3D_TRAIN_SYMBOLS)
    assert not other & set(funcs)


def test_makefile_lists_the_source_and_the_header():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_gblock_train.hip" in mk.split("SRCS =")[1].splitlines()[0].split()
    hdrs = mk.split("HDRS =")[1].splitlines()[0].split()
    assert "../../include/i2v_hip_gblock_train.h" in hdrs and "i2v_res3d_trunk.h" in hdrs and "i2v_train_conv.h" in hdrs and "i2v_power_iter.h" in hdrs


@pytest.mark.parametrize("tag", sorted(gc.FIXTURES))
def test_keys_are_those_of_the_module_s_state_dict(tag):
    from stage1_VAE.modules.decoder import GeneratorBlock
    cfg = gc.FIXTURES[tag]
    net = GeneratorBlock(cfg["n_in"], cfg["n_out"], cfg["spectral"], cfg["z_dim"])
    sd = net.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == gc.param_shapes(cfg)
    assert {k for k, _ in net.named_buffers()} == {k for k in sd if gc.is_buffer(k)}
    assert net.differentiable is False
    header = open(os.path.join(REPO, "include", "i2v_hip_gblock_train.h")).read()
    for k in ("conv_{0,1}.{weight_orig,weight_u,weight_v,bias}", "norm_0.{conv,conv_gamma,conv_beta}.{weight,bias}", "norm_1.linear.{weight,bias}",
              "norm_s.bn.{weight,bias}", "conv_s.{weight_orig,weight_u,weight_v}"):
        assert k in header


@pytest.mark.parametrize("args, word", [((8, 16, 4, 1), "multiples of 16"), ((16, 24, 4, 1), "multiples of 16"), ((16, 2048, 4, 0), "multiples of 16"),
                                        ((0, 16, 4, 1), "multiples of 16"), ((32, 16, 0, 1), "z_dim"), ((32, 16, -3, 0), "z_dim")])
def test_create_refuses_before_a_device_is_looked_for(args, word):
    lib = i2v_native.lib()
    h = ctypes.c_void_p()
    assert lib.i2v_gblock_train_create(*args, ctypes.byref(h)) == -1 and not h.value
    assert word in lib.i2v_last_error().decode()


def test_sizes_of_a_null_handle_or_a_bad_shape_are_zero():
    lib = i2v_native.lib()
    assert lib.i2v_gblock_train_saved_bytes(None, 1, 1, 4, 4, 4, 4) == 0 and lib.i2v_gblock_train_workspace_bytes(None, 1, 1, 4, 4, 4, 4) == 0
    assert lib.i2v_gblock_train_unit_workspace_bytes(1, 16, 24) == 0 and lib.i2v_gblock_train_unit_workspace_bytes(1, 64, 16) > 0


# ---------------------------------------------------------------------------------------------------------------- what the gate catches

def _modnorm_case(mode):
    C, B, thw = gc.UNIT_CASES[1]
    g, act, x = gc.unit_inputs(7, C, B, thw)
    rng = np.random.default_rng(8)
    mod = torch.from_numpy(rng.standard_normal((B, thw[1], thw[2], C) if mode == 0 else (B, 2 * C)).astype(np.float32))
    return g, act, x, mod


@pytest.mark.parametrize("mode, error, which", [(0, "slope_at_zero", "dx"), (1, "slope_at_zero", "dx"), (0, "plain_gamma", "dx"), (0, "unbiased", "dx"),
                                                (1, "unbiased", "dx"), (0, "t_mean", "dgamma")])
def test_deliberate_errors_in_the_modulated_norm_land_above_the_gate(mode, error, which):
    g, act, x, mod = _modnorm_case(mode)
    dx, dg, _, S, (Sg, _) = gc.modnorm_ref(mode, g, act, x, mod)
    bad = gc.modnorm_ref(mode, g, act, x, mod, **{error: 1.0 if error == "slope_at_zero" else True})
    ref, wrong, S_, n = (dx, bad[0], S, 4) if which == "dx" else (dg, bad[1], Sg, 2)
    ok, ratio, l2 = gc.gate(ref.float(), ref, S_, n)
    assert ok and ratio <= 1.0, "the float64 result rounded to fp32 passes its own gate"
    ok, ratio, l2 = gc.gate(wrong.float(), ref, S_, n)
    print(f"mode {mode} {error}: |err| / bound {ratio:.1f}, rel-L2 {l2:.2e}")
    assert not ok and ratio > 10


def test_the_missing_projection_lands_above_the_gate():
    rng = np.random.default_rng(9)
    cout, cin, rows = 48, 32, 180
    g, x = torch.from_numpy(rng.standard_normal((rows, cout))), torch.from_numpy(rng.standard_normal((rows, cin)))
    w = torch.from_numpy(rng.standard_normal((cout, cin)) / np.sqrt(cin))
    u, v = gc._unit(torch.from_numpy(rng.standard_normal(cout))), gc._unit(torch.from_numpy(rng.standard_normal(cin)))
    wn, u, v, sigma = gc.spectral(w, u, v, True)
    dwn, S = g.t() @ x, g.abs().t() @ x.abs()
    n = sum(gc.wgrad1_plan(cout, cin, rows))
    ref, bound = gc.sn_finish_ref(dwn, S, n, w, u, v, sigma)
    assert gc.rel(ref, gc.sn_project(dwn, wn, u, v, sigma)) < 1e-12
    assert gc.gate_bound(ref.float(), ref, bound)[0]
    wrong, _ = gc.sn_finish_ref(dwn, S, n, w, u, v, sigma, drop_projection=True)
    ok, ratio, l2 = gc.gate_bound(wrong.float(), ref, bound)
    print(f"missing projection: |err| / bound {ratio:.1f}, rel-L2 {l2:.2e}")
    assert not ok and ratio > 10


def test_unit_cases_are_a_latin_square():
    cs, bs, ms = sorted({c[0] for c in gc.UNIT_CASES}), sorted({c[1] for c in gc.UNIT_CASES}), sorted({c[2] for c in gc.UNIT_CASES})
    assert cs == [16, 48, 64, 128] and bs == [1, 2, 3] and ms == [(1, 4, 4), (2, 8, 8), (3, 5, 6)]
    assert {(c[0], c[1]) for c in gc.UNIT_CASES} == {(c, b) for c in cs for b in bs}      # every channel count with every batch
    assert {(c[0], c[2]) for c in gc.UNIT_CASES} == {(c, m) for c in cs for m in ms}      # ... and with every map
    assert gc.BIG_CASE == (16, 4, (16, 32, 32))
