"""CPU-side checks of the DTFVD / diversity surface: the mirrors keep the reference's state_dict layout, the shape arithmetic equals the
shapes the reference produced, the eigh Frechet route vs the reference's sqrtm value on rank-deficient 1024-d statistics, the
accumulator's state round trip, the refusals, the new native symbols and both evaluation CLIs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtfvd_common as dc
import i2v_native
from conftest import PKG, REPO
from metrics.Diversity import I3D as diversity
from metrics.Diversity.VGG import compute_vgg_diversity
from metrics.DTFVD import DTFVD_Score as score
from metrics.DTFVD import ID3, ID3_32
from metrics.PyTorch_FVD.I3D import I3D as KineticsI3D

NEW_SYMBOLS = ["i2v_dti3d_create", "i2v_i3d_features_workspace_bytes", "i2v_i3d_feature_steps", "i2v_i3d_features", "i2v_diversity_update"]
I3D_FIXTURES = ["dtfvd_i3d16_t16", "dtfvd_i3d16_t9", "dtfvd_i3d16_t24", "dtfvd_i3d32_t32", "dtfvd_i3d32_t40"]


@pytest.mark.parametrize("fixture", I3D_FIXTURES)
def test_mirror_state_dict_equals_reference_list(fixture):
    _, meta = dc.load_fixture(fixture)
    nc = meta["weights"]["num_classes"]
    for mod in (ID3, ID3_32):
        got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in mod.InceptionI3D(nc, 1).state_dict().items()]
        assert got == meta["state_dict"]
        assert got == [[k, list(s), d] for k, s, d in dc.dti3d_state_dict_spec(nc)]
        mod.InceptionI3D(nc, 1).load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in dc.dti3d_state_dict(1, nc).items()}, strict=True)
    assert ID3.InceptionI3D.feature_dim == 1024 and (ID3.InceptionI3D.LENGTH, ID3_32.InceptionI3D.LENGTH) == (16, 32)


@pytest.mark.parametrize("T", [16, 9, 24, 32, 40])
def test_shape_arithmetic_vs_reference_shapes(T):
    _, meta = dc.load_fixture("dtfvd_shapes")
    assert meta["H"] == 224
    assert ID3.endpoint_shapes(T) == meta["shapes"]["16"][str(T)]
    assert ID3_32.endpoint_shapes(T) == meta["shapes"]["32"][str(T)]
    assert (meta["shapes"]["32"][str(T)]["AvgPool_5"] is None) == (T < 25)


def test_endpoint_shapes_of_the_i3d_fixtures():
    for name in I3D_FIXTURES:
        _, meta = dc.load_fixture(name)
        want = {k: v["shape"] for k, v in meta["endpoints"].items()}
        shapes = (ID3_32 if meta["length"] == 32 else ID3).endpoint_shapes(meta["clips"]["t"], batch=meta["clips"]["n"])
        assert shapes == want, name


def test_frechet_eigh_route_vs_reference_sqrtm_on_rank_deficient_statistics():
    """24 clips, 1024 features: rank-23 covariances.  Gate: 10 x the distance between the two float64 formulations measured when the
    fixture was made (meta eigh_vs_sqrtm_rel = 1.71e-8 -> 1.71e-7 relative)."""
    arr, meta = dc.load_fixture("dtfvd_end2end")
    g, o = arr["act_gen"].astype(np.float64), arr["act_orig"].astype(np.float64)
    got = score.calculate_frechet_distance(g.mean(0), np.cov(g, rowvar=False), o.mean(0), np.cov(o, rowvar=False))
    ref = meta["fvd_fp32_sqrtm"]
    dev = abs(got - ref) / abs(ref)
    print(f"DTFVD eigh {got!r}, reference sqrtm {ref!r}, relative deviation {dev:.3e} (at fixture time {meta['eigh_vs_sqrtm_rel']:.3e})")
    assert meta["eigh_vs_sqrtm_rel"] > 0 and dev <= 10 * meta["eigh_vs_sqrtm_rel"]
    assert float(arr["fvd"][2]) == ref and float(arr["fvd"][0]) == meta["fvd_fp32_eigh"]
    # the gate of the GPU tests is the one the issue sets: 10 x the reference's own fp32-vs-fp64 deviation, floored at 1e-6 below 1e-7
    r = meta["ref_fp32_vs_fp64_rel"]
    assert r == abs(meta["fvd_fp32_eigh"] - meta["fvd_fp64_eigh"]) / abs(meta["fvd_fp64_eigh"])
    assert meta["gate"]["gate_rel"] == (1e-6 if r < 1e-7 else 10 * r) and meta["gate"]["floored"] == (r < 1e-7)
    g64, o64 = arr["act_gen64"], arr["act_orig64"]
    v64 = score.calculate_frechet_distance(g64.mean(0), np.cov(g64, rowvar=False), o64.mean(0), np.cov(o64, rowvar=False))
    assert abs(v64 - meta["fvd_fp64_eigh"]) <= 10 * meta["eigh_vs_sqrtm_rel"] * abs(v64)


def test_diversity_fixture_pair_formula():
    arr, meta = dc.load_fixture("dtfvd_diversity")
    assert dc.pair_diversity(arr["embed"]) == meta["diversity_fp32"] and dc.pair_diversity(arr["embed64"]) == meta["diversity_fp64"]
    r = meta["ref_fp32_vs_fp64_rel"]
    assert meta["gate"]["gate_rel"] == (1e-6 if r < 1e-7 else 10 * r)
    assert arr["embed"].shape == (meta["clips"]["n"], meta["clips"]["r"], 1024)


def test_accumulator_state_round_trip_with_1024_features():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((30, 1024)).astype(np.float32), (rng.standard_normal((25, 1024)) * 1.5 + 0.3).astype(np.float32)
    model = ID3.InceptionI3D(18, 1)
    acc = score.DTFVDAccumulator(model)
    assert acc.dim == 1024
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    acc.load_state({"gen": {"n": 30, "sum": a64.sum(0), "gram": a64.T @ a64}, "orig": {"n": 25, "sum": b64.sum(0), "gram": b64.T @ b64}}, device="cpu")
    st = acc.state()
    assert st["gen"]["n"] == 30 and np.array_equal(st["gen"]["sum"], a64.sum(0)) and np.array_equal(st["orig"]["gram"], b64.T @ b64)
    acc2 = score.DTFVDAccumulator(model)
    acc2.load_state(st, device="cpu")
    assert acc2.compute() == acc.compute() and np.isfinite(acc.compute()) and acc.compute() > 0
    with pytest.raises(ValueError):
        acc2.load_state({"orig": {"n": 3, "sum": np.zeros(18), "gram": np.zeros((18, 18))}}, device="cpu")
    with pytest.raises(i2v_native.I2VError):     # update_features feeds the device kernel: host features are refused
        score.DTFVDAccumulator(model).update_features(torch.from_numpy(a), "gen")
    with pytest.raises(TypeError):
        score.DTFVDAccumulator(KineticsI3D(16))


def test_refusals_without_a_gpu():
    model = ID3.InceptionI3D(18, 1).eval()
    clips = torch.zeros(2, 16, 3, 32, 32)
    with pytest.raises(i2v_native.I2VError):
        model.forward_frames(clips)
    with pytest.raises(i2v_native.I2VError):
        model.get_representation(torch.zeros(1, 3, 16, 224, 224))
    with pytest.raises(ValueError, match="224"):
        model.get_representation(torch.zeros(1, 3, 16, 112, 112))
    with pytest.raises(i2v_native.I2VError):
        score.DTFVDAccumulator(model).update(clips, "gen")
    with pytest.raises(i2v_native.I2VError):
        score.calculate_FVD(model, clips, clips, 2, cuda=False)
    with pytest.raises(i2v_native.I2VError):
        diversity.DiversityAccumulator(model).update(clips[None])
    with pytest.raises(i2v_native.I2VError):
        diversity.compute_DTI3D_diversity(clips[None], model)
    with pytest.raises(NotImplementedError):
        model(clips.permute(0, 2, 1, 3, 4))
    with pytest.raises(NotImplementedError):
        model.replace_logits(5)
    with pytest.raises(NotImplementedError):
        ID3.InceptionI3D(18, 1, final_endpoint='Mixed_4f')
    with pytest.raises(ValueError):
        ID3.InceptionI3D(18, 1, final_endpoint='nope')
    m32 = ID3_32.InceptionI3D(18, 1).eval()
    for t in (16, 31, 33):
        with pytest.raises(ValueError, match="32"):
            score.calculate_FVD32(m32, torch.zeros(2, t, 3, 32, 32), torch.zeros(2, 32, 3, 32, 32), 2)
        with pytest.raises(ValueError, match="32"):     # the reference's assert lets this one through (operator precedence)
            score.calculate_FVD32(m32, torch.zeros(2, 32, 3, 32, 32), torch.zeros(2, t, 3, 32, 32), 2)
    with pytest.raises(ValueError, match="32"):
        score.embedding_I3D_32(m32, torch.zeros(2, 16, 3, 32, 32), 2)
    with pytest.raises(NotImplementedError, match="TensorFlow"):
        diversity.compute_I3D_diversity(clips[None], 5)
    with pytest.raises(NotImplementedError, match="torchvision"):
        compute_vgg_diversity(clips[None])


def test_dtfvd_mode_of_the_hooks_needs_the_dt_network():
    from utils import auxiliaries as aux
    with pytest.raises(NotImplementedError, match="DTFVD"):
        aux.evaluate_FVD_prior([], None, None, KineticsI3D(16).eval(), 64, None, 0, "DTFVD", False)
    with pytest.raises(NotImplementedError, match="DTFVD"):
        aux.evaluate_FVD_posterior([], None, None, KineticsI3D(16).eval(), "DTFVD")
    assert isinstance(aux._fvd_accumulator(ID3.InceptionI3D(18, 1), "DTFVD", "test"), score.DTFVDAccumulator)
    assert isinstance(aux._fvd_accumulator(ID3_32.InceptionI3D(18, 1), "DTFVD", "test"), score.DTFVDAccumulator)
    with pytest.raises(ValueError):     # an empty loader: both sets need at least one update
        aux.evaluate_FVD_posterior([], None, None, ID3.InceptionI3D(18, 1), "DTFVD")


def test_header_symbols_and_sources():
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    declared = set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    lib = i2v_native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in i2v_native.SYMBOLS and hasattr(lib, name), name
    for ref in ("metrics/DTFVD/ID3.py", "ID3_32.py", "get_representation", "DTFVD_Score.calculate_FVD", "metrics/Diversity/I3D.py"):
        assert ref in header, ref
    for name in ("DTFVD_Score.py", "ID3.py", "ID3_32.py"):
        text = open(os.path.join(PKG, "metrics", "DTFVD", name)).read()
        assert not re.search(r"^\s*(import|from) (scipy|kornia)", text, flags=re.M), name


@pytest.mark.parametrize("script,argv,word", [
    ("eval_synthesis_quality.py", ["-FID", "True"], "-FID is not built"),
    ("eval_synthesis_quality.py", ["-LPIPS", "True"], "-LPIPS is not built"),
    ("eval_synthesis_quality.py", ["-FVD", "True", "-DTFVD", "True"], "-FVD is not built"),
    ("eval_diversity.py", ["-dataset", "DTDB", "-I3D", "True"], "-I3D is not built"),
    ("eval_diversity.py", ["-dataset", "DTDB", "-VGG", "True", "-DTI3D", "True"], "-VGG is not built"),
])
def test_cli_not_built_exits(script, argv, word):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "-gpu", "0"] + argv, capture_output=True, text=True, cwd=PKG)
    assert r.returncode != 0 and word in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("script,flags", [
    ("eval_synthesis_quality.py", ["-gpu", "-dataset", "-texture", "-ckpt_path", "-data_path", "-seq_length", "-bs", "-FID", "-FVD", "-DTFVD", "-LPIPS",
                                   "-clips_npy", "-i3d_path", "-seed"]),
    ("eval_diversity.py", ["-gpu", "-dataset", "-texture", "-ckpt_path", "-data_path", "-seq_length", "-n_realiz", "-bs", "-I3D", "-VGG", "-DTI3D",
                           "-clips_npy", "-i3d_path", "-seed"]),
])
def test_cli_help(script, flags):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True, cwd=PKG)
    assert r.returncode == 0, r.stderr
    for f in flags:
        assert re.search(rf"(^|\s){f}\b", r.stdout), f


def test_compared_frames_rule():
    sys.path.insert(0, PKG)
    import eval_synthesis_quality as esq
    seq, gen = torch.arange(17.0).view(1, 17, 1, 1, 1), -torch.arange(1.0, 17.0).view(1, 16, 1, 1, 1)
    f, r = esq.compared_frames("bair", seq, gen)
    assert f.flatten().tolist() == [0.0] + [-float(i) for i in range(1, 16)] and r.flatten().tolist() == [float(i) for i in range(16)]
    f, r = esq.compared_frames("iPER", seq, gen)
    assert f.shape[1] == 17 and f[0, 0] == 0 and torch.equal(r, seq)
    f, r = esq.compared_frames("DTDB", seq, gen)
    assert torch.equal(f, gen) and torch.equal(r, seq[:, :-1])
