"""CPU checks of the gradient penalty's gradient on the temporal discriminator (csrc/i2v_res3d_gp.h, include/i2v_hip_disc3d_gp.h,
i2v_train.TemporalDiscPenaltyTrainer, resnet3D.Discriminator.forward_with_penalty): the hand-written float64 oracle of
tests/temporal_disc_gp_common.py against torch's float64 double backward and against the fixtures made from the reference's own module
(tests/golden/disc3d_gp_*.npz); every deliberate error against the gate the GPU tests apply; the C ABI of the seventh header against
i2v_native.DISC3D_GP_SYMBOLS; the Makefile's lists; the refusals."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import i2v_native
import temporal_disc_common as tc
import temporal_disc_gp_common as gp
import test_host_abi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURE_ROUNDING = 2e-7      # the fixtures' gradients are rounded to fp32: relative L2 of that rounding <= 2^-24, with room for tiny tensors


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


def case(name):
    """-> (cfg, state dict, clips) of fixture ``name``"""
    if name == "a":
        return tc.CFG_A, {k: torch.from_numpy(v) for k, v in load("temporal_disc_a_params*.npz").items()}, tc.clips_a()[1]
    cfg = tc.CFG_B if name == "b" else tc.CFG_C
    return cfg, tc.synthetic_state(cfg, tc.SEED_B), (tc.clips_b if name == "b" else tc.clips_c)()


@pytest.fixture(scope="module")
def oracles():
    """The hand-written oracle on the three fixtures, own decisions, scale 1: computed once"""
    return {n: gp.penalty_oracle(case(n)[1], case(n)[2], case(n)[0]) for n in "abc"}


def test_every_fixture_file_is_below_the_committed_size_limit():
    files = glob.glob(os.path.join(GOLDEN, "disc3d_gp_*.npz"))
    assert len(files) == 13 and all(os.path.getsize(f) < 1 << 20 for f in files)


@pytest.mark.parametrize("name", ("b", "c"))
def test_hand_written_oracle_equals_torchs_double_backward(name, oracles):
    """Own decisions, and the decisions of an fp32 pass given to both (they differ from float64's own or not: both sides take them)."""
    cfg, sd, x = case(name)
    for given, scale in ((None, 1.0), (tc.forward_oracle(sd, x, cfg, training=True, dtype=torch.float32)[2]["decisions"], gp.W_GP)):
        hand = oracles[name] if given is None else gp.penalty_oracle(sd, x, cfg, scale=scale, decisions=given)
        l_gp, auto = gp.penalty_autograd(sd, x, cfg, scale=scale, decisions=given)
        assert abs(float(hand["l_gp"]) / float(l_gp) - 1) < 1e-12
        assert set(auto) == set(hand["grads"])
        for k, v in auto.items():
            if v is None:
                assert k == "layer.3.1.bn2.bias" and float(hand["grads"][k].abs().max()) == 0.0
            else:
                assert gp.rel(hand["grads"][k], v) <= 1e-10, (name, k, gp.rel(hand["grads"][k], v))


@pytest.mark.parametrize("name", ("a", "b", "c"))
def test_hand_written_oracle_equals_the_reference_fixtures(name, oracles):
    main, grads = load(f"disc3d_gp_{name}.npz"), load(f"disc3d_gp_{name}_grads*.npz")
    o = oracles[name]
    assert abs(float(o["l_gp"]) / float(main["l_gp"]) - 1) < 1e-10
    assert set(grads) == set(o["grads"]) == {k for k in case(name)[1] if not k.endswith(("weight_u", "weight_v"))}
    assert json.loads(bytes(main["none"]).decode()) in ([], ["layer.3.1.bn2.bias"])     # (.backward() leaves an exact zero there, grad() a None)
    for k, v in grads.items():
        if k == "layer.3.1.bn2.bias":      # the one structurally zero gradient: g does not depend on the last bias
            assert float(np.abs(v).max()) == 0.0 and float(o["grads"][k].abs().max()) == 0.0
        else:
            assert gp.rel(o["grads"][k], v) <= FIXTURE_ROUNDING, (name, k, gp.rel(o["grads"][k], v))
            assert float(np.abs(v).max()) > 0.0


def test_every_deliberate_error_exceeds_the_gate(oracles):
    """On fixture B every mutation moves at least one parameter gradient past the 1e-4 gate of the GPU tests; none needs its unit's gate.
    The unmutated oracle stays seven orders of magnitude inside it."""
    cfg, sd, x = case("b")
    good = oracles["b"]["grads"]
    for m in gp.MUTATIONS:
        bad = gp.penalty_oracle(sd, x, cfg, mutate=m)["grads"]
        worst = max((gp.rel(bad[k], good[k]), k) for k in good if k != "layer.3.1.bn2.bias")
        print(f"  {m}: worst rel-L2 {worst[0]:.2e} at {worst[1]}")
        assert worst[0] > tc.TOL_L2, (m, worst)
    assert len(gp.MUTATIONS) == 7


def test_unit_gates_reject_the_unit_errors():
    """The two GroupNorm unit oracles: the mutated value lies outside the bound of the right one."""
    c = gp.GN_CASES[1]
    x, xd, resd, act, g, gd, w, _ = gp.gn_case_inputs(c)
    mask = act > 0
    ref, bound, _, _ = gp.gn_tangent_oracle(x, xd, w, resd, mask)
    bad, _, _, _ = gp.gn_tangent_oracle(x, xd, w, resd, mask, mutate="tangent_relu_mask_dropped")
    assert not tc.gate_bound(bad, ref, bound)[0] and tc.gate_bound(ref.float(), ref, bound)[0]
    good = gp.gn_dual_oracle(g, gd, x, xd, w, mask)
    for m, name in (("second_order_dropped", "dx"), ("gamma_without_tangent", "dweight")):
        bad = gp.gn_dual_oracle(g, gd, x, xd, w, mask, mutate=m)
        assert not tc.gate_bound(bad[name][0], *good[name])[0], m
    for name, (ref, bound) in good.items():
        assert tc.gate_bound(ref.float(), ref, bound)[0], name      # an fp32 rounding of the right value passes
    slices = [(gp.gn_slices(int(np.prod(c["thw"])), c["c"] // 16), gp.gn_slices(int(np.prod(c["thw"])), 16)) for c in gp.GN_CASES]
    assert (1, 1) in slices and (32, 32) in slices and any(1 < a < 32 and 1 < b < 32 for a, b in slices), slices


def parse_header(name):
    text = open(os.path.join(REPO, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = text.replace('extern "C" {', "").replace("}", "")
    funcs = {}
    for decl in (" ".join(d.split()) for d in text.split(";") if d.strip()):
        m = re.match(r"(.*?)\b(i2v_\w+)\s*\((.*)\)$", decl)
        assert m, decl
        args = [re.match(r"(.*?)(\w+)$", a.strip()).groups() for a in m.group(3).split(",") if a.strip() and a.strip() != "void"]
        funcs[m.group(2)] = (m.group(1).strip(), [(t.strip(), n) for t, n in args])
    return funcs


def test_header_matches_the_seventh_table():
    funcs = parse_header("i2v_hip_disc3d_gp.h")
    assert set(funcs) == set(i2v_native.DISC3D_GP_SYMBOLS) and len(funcs) == 10
    assert abi.compare_functions(funcs, i2v_native.DISC3D_GP_SYMBOLS) == []
    assert all(n.startswith("i2v_disc3d_gp_") for n in funcs)
    res, args = i2v_native.DISC3D_GP_SYMBOLS["i2v_disc3d_gp_backward"]
    assert abi.compare_functions(funcs, dict(i2v_native.DISC3D_GP_SYMBOLS, i2v_disc3d_gp_backward=(res, args[:-1]))) != []
    others = (i2v_native.SYMBOLS, i2v_native.DISC_SYMBOLS, i2v_native.DISC3D_SYMBOLS, i2v_native.ENC3D_TRAIN_SYMBOLS, i2v_native.GBLOCK_TRAIN_SYMBOLS,
              i2v_native.GEN_TRAIN_SYMBOLS)
    assert all(not set(t) & set(funcs) for t in others) and len(i2v_native.DISC3D_SYMBOLS) == 24
    assert os.path.exists(i2v_native.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(i2v_native.LIB_PATH)
    assert all(hasattr(lib, n) for n in funcs)
    assert all(hasattr(i2v_native.lib(), n) for n in funcs)


def test_makefile_lists_the_new_files_and_the_encoder_path_does_not_include_them():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    hdrs = mk.split("HDRS =")[1].splitlines()[0].split()
    assert "i2v_res3d_gp.h" in hdrs and "../../include/i2v_hip_disc3d_gp.h" in hdrs
    assert "i2v_disc3d.hip" in mk.split("SRCS =")[1].splitlines()[0].split()
    assert "i2v_res3d_gp.h" in open(os.path.join(PKG, "csrc", "i2v_disc3d.hip")).read()
    assert "i2v_res3d_gp" not in open(os.path.join(PKG, "csrc", "i2v_encoder_train.hip")).read()
    src = open(os.path.join(PKG, "csrc", "i2v_res3d_gp.h")).read()
    assert "getenv" not in src and "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src


def test_refusals_need_no_gpu():
    lib = i2v_native.lib()
    assert lib.i2v_disc3d_gp_saved_bytes(None, 2, 12, 64, 64) == 0 and lib.i2v_disc3d_gp_workspace_bytes(None, 2, 12, 64, 64) == 0
    assert lib.i2v_disc3d_gp_groupnorm_workspace_bytes(0, 16) == 0 and lib.i2v_disc3d_gp_groupnorm_workspace_bytes(2, 48) > 0
    assert lib.i2v_disc3d_gp_backward(None, None, 0, 2, 12, 64, 64, 10.0, None, 0, None, 0, None, 0, None) != 0
    assert lib.i2v_disc3d_gp_head_dual_unit(None, None, 1.0, 2, 16, None, None, None, None, None) != 0
    assert "null argument" in lib.i2v_last_error().decode()
    cpu = torch.zeros(2, 4, 4, 4, 16)
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        i2v_native.disc3d_gp_groupnorm_tangent_unit(cpu, cpu, torch.zeros(2, 16, 2, dtype=torch.float64), torch.ones(16))
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        i2v_native.disc3d_gp_maxpool_tangent_unit(cpu, torch.zeros(2, 4, 2, 2, 16, dtype=torch.int32))
    from stage1_VAE.modules.resnet3D import Discriminator
    from stage1_VAE.modules import loss
    net = Discriminator(dict(tc.CFG_A))
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        net.forward_with_penalty(torch.zeros(1, 3, 12, 64, 64))
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        loss.gradient_penalty(net, torch.zeros(1, 3, 12, 64, 64))
    import i2v_train
    with pytest.raises(NotImplementedError, match="double backward") as e:
        i2v_train.TemporalDiscTrainer(net, w_GP=10)
    assert "TemporalDiscPenaltyTrainer" in str(e.value)
    assert issubclass(i2v_train.TemporalDiscPenaltyTrainer, i2v_train.TemporalDiscTrainer)
    with pytest.raises(NotImplementedError, match="composition") as e:
        loss.Backward(None).forward(None, None, None, None, None, None, 0, None)
    assert "forward_with_penalty" in str(e.value) and "TemporalDiscPenaltyTrainer" in str(e.value)
