"""CPU-side checks of the FID surface: the float64 oracle of tests/fid_common.py against the fixtures written from the reference's own
modules, the deliberate errors the gates have to catch, the new native symbols, the holder's key list, the reductions and the CLI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_common as fc
import i2v_native
from conftest import PKG, REPO
from metrics.FID import FID_Score
from metrics.FID import inception as inc_mod
from metrics.PyTorch_FVD import FVD_logging

NEW_SYMBOLS = ["i2v_inception_create", "i2v_inception_destroy", "i2v_inception_load", "i2v_inception_block_shape", "i2v_inception_workspace_bytes",
               "i2v_inception_input_stage", "i2v_inception_features", "i2v_inception_conv_unit", "i2v_inception_pool", "i2v_inception_global_avg",
               "i2v_inception_mixed_shape", "i2v_inception_mixed_workspace_bytes", "i2v_inception_mixed_forward"]


def fixture_frames(f):
    return torch.from_numpy(fc.clips(f["seed"], f["n"], 1, f["h"], f["w"]))[:, 0].contiguous()


# ---------------------------------------------------------------------------------------------------------------- oracle vs fixtures

def test_oracle_reproduces_the_reference_at_299():
    arr, meta = fc.load_fixture("fid_feats_299")
    _, bmeta = fc.load_fixture("fid_blocks")
    sd = fc.fid_state_dict(meta["weights"]["seed"])
    for tag, f in meta["frames"].items():
        x = fixture_frames(f)
        blocks = fc.trunk_oracle(sd, fc.input_oracle(x))
        assert tuple(arr[f"block3_{tag}"].shape) == (f["n"], 2048)
        assert max(fc.rel_l2_rows(torch.from_numpy(arr[f"block3_{tag}"]), blocks[3].flatten(1))) <= 1e-5      # the reference ran in fp32
        assert np.count_nonzero(arr[f"block3_{tag}"], axis=1).min() >= 1024 and np.isfinite(arr[f"block3_{tag}"]).all()
        if tag == "64x48":
            assert bmeta["frame"] == f
            for b in range(3):
                st = bmeta["blocks"][str(b)]
                assert list(blocks[b].shape) == st["shape"] and abs(float(blocks[b].norm()) - st["l2"]) <= 1e-5 * st["l2"]
            assert [bmeta["blocks"][str(b)]["shape"][1:] for b in range(3)] == [[64, 73, 73], [192, 35, 35], [768, 17, 17]]
            # align_corners=True is another network input: rejected at the project gate
            bad = fc.trunk_oracle(sd, fc.input_oracle(x, align_corners=True))[3]
            assert max(fc.rel_l2_rows(bad.flatten(1), blocks[3].flatten(1))) > fc.TOL_L2
    assert bmeta["dims"] == {str(k): v for k, v in inc_mod.InceptionV3.BLOCK_INDEX_BY_DIM.items()} and inc_mod.InceptionV3.DEFAULT_BLOCK_INDEX == 3


def test_frechet_value_and_gate_of_the_score_fixture():
    arr, meta = fc.load_fixture("fid_score")
    im = meta["images"]
    assert arr["act64"].shape == (2, im["used"], 2048) and im["used"] == (im["n"] // im["batch_size"]) * im["batch_size"] == 16
    assert np.isfinite(arr["act64"]).all() and min(np.count_nonzero(np.abs(a).sum(0)) for a in arr["act64"]) >= 1024
    (m1, s1), (m2, s2) = fc.frechet_stats(arr["act64"][0]), fc.frechet_stats(arr["act64"][1])
    got = FID_Score.calculate_frechet_distance(m1, s1, m2, s2)
    assert FID_Score.calculate_frechet_distance is FVD_logging.calculate_frechet_distance                 # imported, not copied
    assert abs(got - meta["fid_fp64_eigh"]) <= 1e-9 * abs(got)
    assert abs(meta["fid_fp32_sqrtm"] - got) <= 10 * meta["eigh_vs_sqrtm_rel"] * abs(got)                 # the reference's sqrtm formulation
    r = meta["ref_fp32_vs_fp64_rel"]
    assert meta["gate"]["gate_rel"] == (1e-6 if r < 1e-7 else 10 * r)
    assert abs(meta["fid_all_fp64_eigh"] - got) > meta["gate"]["gate_rel"] * got                           # all 20 images: another value


# ---------------------------------------------------------------------------------------------------------------- what the gates catch

SEED = 91


def test_unit_gate_accepts_fp32_and_rejects_bn_eps_and_a_swapped_window():
    for case in (fc.conv_cases()[0], next(c for c in fc.conv_cases() if c["kernel"] == (1, 7)), next(c for c in fc.conv_cases() if c["kernel"] == (7, 1))):
        x, (w, bn) = fc.conv_input(case), fc.conv_params(case)
        ref, S, n = fc.conv_oracle(x, w, bn, case["stride"], case["padding"])
        g, b, m, v = (torch.from_numpy(t) for t in bn)
        scale = (g.double() / torch.sqrt(v.double() + fc.BN_EPS)).float()
        shift = (b.double() - m.double() * scale.double()).float()
        fp32 = torch.relu(F.conv2d(x, w, stride=case["stride"], padding=case["padding"]) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
        ok, ratio, l2 = fc.gate(fp32, ref, S, n)
        assert ok, (case["id"], ratio, l2)
        assert not fc.gate(fc.conv_oracle(x, w, bn, case["stride"], case["padding"], mutate="bn_eps")[0].float(), ref, S, n)[0], case["id"]
        if case["kernel"][0] != case["kernel"][1]:
            hw = (9, 9)                                   # a square map: the swapped window gives the same shape and other values
            x = fc.randn(case["seed"] + 7, (1, case["cin"], *hw))
            ref, S, n = fc.conv_oracle(x, w, bn, case["stride"], case["padding"])
            assert not fc.gate(fc.conv_oracle(x, w, bn, case["stride"], case["padding"], mutate="swap_kernel")[0].float(), ref, S, n)[0], case["id"]


def test_pool_errors_are_rejected():
    x = fc.randn(9300, (2, 8, 6, 7), negative=True)
    good = fc.pool_oracle(x, fc.POOL_MAX_S1)[0]
    assert torch.equal(good, F.max_pool2d(x, 3, 1, 1)) and (good < 0).all()
    assert not torch.equal(fc.pool_oracle(x, fc.POOL_MAX_S1, "zero_pad_max")[0], good)                     # zeros win on an all-negative map
    assert tuple(fc.pool_oracle(x, fc.POOL_MAX_S2)[0].shape[2:]) == (2, 3) != tuple(fc.pool_oracle(x, fc.POOL_MAX_S2, "ceil_mode")[0].shape[2:])
    x = fc.randn(9301, (1, 4, 5, 6))
    ref, S, n = fc.pool_oracle(x, fc.POOL_AVG)
    assert fc.gate(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), ref, S, n)[0]
    assert not fc.gate(fc.pool_oracle(x, fc.POOL_AVG, "count_pad")[0].float(), ref, S, n)[0]
    one = fc.randn(9302, (1, 4, 1, 1))
    assert torch.equal(fc.pool_oracle(one, fc.POOL_AVG)[0].float(), one)                                  # divisor 1 on a 1 x 1 map


@pytest.mark.parametrize("block,mutations", [("Mixed_5b", ("bn_eps", "avg_count_pad", "cat_order")), ("Mixed_6b", ("swap_1x7_7x1", "avg_count_pad", "cat_order")),
                                             ("Mixed_7c", ("e2_avg", "zero_pad_max", "cat_order"))])
def test_block_mutations_fail_the_project_gate(block, mutations):
    sd = fc.fid_state_dict(SEED)
    name, kind, cin, par = fc.MIXED[fc.BLOCK_NAMES.index(block)]
    x = fc.randn(9400 + cin, (1, cin, 5, 5))
    if block == "Mixed_7c":
        x = -x.abs()                                        # an all-negative input: zero padding wins the max pool
    ref = fc.mixed_cat(fc.mixed_oracle(sd, block, x))
    assert ref.shape[1] == {"Mixed_5b": 256, "Mixed_6b": 768, "Mixed_7c": 2048}[block]
    for m in mutations:
        bad = fc.mixed_cat(fc.mixed_oracle(sd, block, x, mutate=m))
        assert max(fc.rel_l2_rows(bad, ref)) > fc.TOL_L2, m


def test_input_stage_oracle_tells_align_corners_and_normalisation_apart():
    x = torch.from_numpy(fc.clips(9500, 1, 1, 16, 16))[:, 0]
    a = fc.input_oracle(x)
    assert tuple(a.shape) == (1, 3, 299, 299) and fc.rel_l2(fc.input_oracle(x, align_corners=True), a) > 1e-4
    assert torch.equal(fc.input_oracle(x, normalize=True), 2 * a - 1) and torch.equal(fc.input_oracle(x, resize=False), x.double())


# ---------------------------------------------------------------------------------------------------------------- surface

def test_header_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    declared = set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    lib = i2v_native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in i2v_native.SYMBOLS and hasattr(lib, name), name
    for ref in ("metrics/FID/inception.py", "metrics/FID/FID_Score.py", "FIDInceptionE_2", "count_include_pad=False"):
        assert ref in header, ref
    assert "i2v_inception.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    for name in ("inception.py", "FID_Score.py", "__init__.py"):
        text = open(os.path.join(PKG, "metrics", "FID", name)).read()
        assert not re.search(r"^\s*(import|from) (torchvision|scipy|imageio)", text, flags=re.M), name


def test_holder_keeps_the_reference_keys_and_loads_files(tmp_path):
    _, meta = fc.load_fixture("fid_blocks")
    m = inc_mod.InceptionV3()
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"] == fc.holder_keys()
    assert [k for k, _ in meta["ignored"]] == ["fc.weight", "fc.bias"]
    assert not any(p.requires_grad for p in m.parameters()) and not m.training
    with pytest.raises(FileNotFoundError, match=fc.FID_FILE):
        m.native()                                          # no path, nothing loaded: refused on first use, nothing is downloaded
    path = str(tmp_path / fc.FID_FILE)
    fc.save_fid_file(path, 5)                               # with fc.* and num_batches_tracked, as the checkpoint has them
    sd = fc.torch_state_dict(5)
    m = inc_mod.InceptionV3(path=path)
    assert torch.equal(m.Mixed_7c.branch_pool.conv.weight, sd["Mixed_7c.branch_pool.conv.weight"])
    assert torch.equal(m.Conv2d_1a_3x3.bn.running_var, sd["Conv2d_1a_3x3.bn.running_var"]) and m.Mixed_6b.branch7x7_2.conv.weight.shape[2:] == (1, 7)
    assert not hasattr(m, "fc")
    m.load_state_dict({**sd, "AuxLogits.fc.weight": torch.zeros(2, 2)})                                    # accepted and ignored
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        inc_mod.InceptionV3(path=str(tmp_path / "nowhere.pth"))
    missing = {k: v for k, v in sd.items() if k != "Mixed_6a.branch3x3.bn.running_mean"}
    with pytest.raises(RuntimeError, match="Mixed_6a.branch3x3.bn.running_mean"):
        inc_mod.InceptionV3().load_state_dict(missing)
    bad = dict(sd)
    bad["Mixed_5c.branch5x5_2.conv.weight"] = torch.zeros(64, 48, 3, 3)
    with pytest.raises(RuntimeError, match="Mixed_5c.branch5x5_2.conv.weight"):
        inc_mod.InceptionV3().load_state_dict(bad)
    with pytest.raises(NotImplementedError):
        inc_mod.InceptionV3(requires_grad=True)
    with pytest.raises(NotImplementedError):
        inc_mod.InceptionV3(use_fid_inception=False)
    assert [(u[0], u[1], u[2], tuple(u[3]), u[4], tuple(u[5])) for u in inc_mod.UNITS] == fc.units()


def test_refusals_without_a_gpu():
    m = inc_mod.InceptionV3()
    m.load_state_dict(fc.torch_state_dict(5))
    with pytest.raises(i2v_native.I2VError):
        m(torch.zeros(1, 3, 16, 16))
    with pytest.raises(i2v_native.I2VError):
        i2v_native.inception_input_stage(torch.zeros(1, 3, 16, 16))
    with pytest.raises(i2v_native.I2VError):
        FID_Score.FIDAccumulator(m).update(torch.zeros(2, 3, 16, 16), "gen")
    with pytest.raises(ValueError, match="which"):
        FID_Score.FIDAccumulator(m).update(torch.zeros(2, 3, 16, 16), "fake")
    if not torch.cuda.is_available():
        with pytest.raises(i2v_native.I2VError):
            FID_Score.calculate_FID(m, torch.zeros(4, 3, 16, 16), torch.zeros(4, 3, 16, 16), 2, 2048)


class FakeModel(torch.nn.Module):
    """[B, 3, H, W] -> [[B, 4, 1, 1]]: the per-channel mean and the first pixel."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x):
        self.calls.append(x.shape[0])
        return [torch.cat([x.mean((2, 3)), x[:, :1, 0, 0]], 1)[:, :, None, None]]


def test_get_activations_drops_the_ragged_batch_and_clips_the_batch_size():
    data = torch.arange(23.0).view(23, 1, 1, 1).expand(23, 3, 2, 2).contiguous()
    model = FakeModel()
    act = FID_Score.get_activations(data, model, batch_size=5, dims=4)
    assert act.dtype == np.float64 and act.shape == (20, 4) and model.calls == [5] * 4 and np.array_equal(act[:, 0], np.arange(20.0))
    model = FakeModel()
    act = FID_Score.get_activations(data[:7], model, batch_size=50, dims=4)
    assert act.shape == (7, 4) and model.calls == [7]                                                     # batch_size > n: clipped to n
    mu, sigma = FID_Score.calculate_activation_statistics(data, FakeModel(), batch_size=5, dims=4, cuda=False)
    assert mu.shape == (4,) and sigma.shape == (4, 4) and mu[0] == pytest.approx(9.5)                      # the mean of 0..19
    wide = FakeModel()
    wide.forward = lambda x: [x[:, :, :2, :2] + 0]                                                        # a spatial block: averaged to [B, C]
    assert FID_Score.get_activations(data, wide, batch_size=23, dims=3).shape == (23, 3)


def test_fid_accumulator_state_round_trip_and_refusals():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((9, 6)), rng.standard_normal((7, 6)) + 0.5
    acc = FID_Score.FIDAccumulator(FakeModel(), dims=6)
    assert isinstance(acc, FVD_logging.StatsAccumulator) and issubclass(FVD_logging.FVDAccumulator, FVD_logging.StatsAccumulator)
    acc.load_state({"gen": {"n": 9, "sum": a.sum(0), "gram": a.T @ a}, "orig": {"n": 7, "sum": b.sum(0), "gram": b.T @ b}}, device="cpu")
    want = FID_Score.calculate_frechet_distance(*fc.frechet_stats(a), *fc.frechet_stats(b))
    assert acc.compute() == pytest.approx(want, rel=1e-9)
    acc2 = FID_Score.FIDAccumulator(FakeModel(), dims=6)
    acc2.load_state(acc.state(), device="cpu")
    assert acc2.compute() == acc.compute()
    acc2.reset("orig")
    with pytest.raises(ValueError, match="both sets"):
        acc2.compute()
    with pytest.raises(ValueError, match="shapes"):
        FID_Score.FIDAccumulator(FakeModel(), dims=5).load_state(acc.state(), device="cpu")
    with pytest.raises(ValueError, match="unknown set"):
        acc2.load_state({"real": acc.state()["gen"]}, device="cpu")


@pytest.mark.parametrize("argv,word", [
    (["-FID", "True"], "-FID is not built: "),
    (["-FID", "True"], "-inception_path"),
    (["-FID", "True", "-inception_path", "a.pth"], "-clips_npy"),
    (["-FID", "True", "-inception_path", "a.pth", "-LPIPS", "True"], "-LPIPS is not built: "),
    ([], "-FID True -inception_path FILE"),
    (["-FVD", "True", "-FID", "True", "-inception_path", "a.pth"], "-FVD is not built"),
])
def test_cli_refusals(argv, word):
    r = subprocess.run([sys.executable, os.path.join(PKG, "eval_synthesis_quality.py"), "-gpu", "0"] + argv, capture_output=True, text=True, cwd=PKG)
    assert r.returncode != 0 and word in r.stderr, (r.returncode, r.stderr)


def test_cli_help_lists_the_new_flag():
    r = subprocess.run([sys.executable, os.path.join(PKG, "eval_synthesis_quality.py"), "--help"], capture_output=True, text=True, cwd=PKG)
    assert r.returncode == 0, r.stderr
    for f in ("-inception_path", "-FID"):
        assert re.search(rf"(^|\s){f}\b", r.stdout), f
