"""CPU-side checks of the FVD surface: the I3D mirror keeps the reference's state_dict layout, the package's padding / shape arithmetic
equals the shapes the reference produced, the host Frechet distance vs the reference's values, the accumulator's state round trip,
and the product path refuses to run without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import fvd_common as fc
import i2v_native
from conftest import PKG, REPO
from metrics.PyTorch_FVD import FVD_logging as fvd
from metrics.PyTorch_FVD.I3D import I3D, endpoint_shapes

FVD_SYMBOLS = ["i2v_i3d_create", "i2v_i3d_load", "i2v_i3d_workspace_bytes", "i2v_i3d_forward", "i2v_i3d_destroy", "i2v_i3d_input_stage",
               "i2v_fvd_stats_update"]


@pytest.mark.parametrize("fixture", ["fvd_i3d_t16", "fvd_i3d_t9", "fvd_i3d_128", "fvd_end2end"])
def test_mirror_state_dict_equals_reference_list(fixture):
    _, meta = fc.load_fixture(fixture)
    nc = meta["weights"]["num_classes"]
    got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in I3D(nc).state_dict().items()]
    if "state_dict" in meta:
        assert got == meta["state_dict"]
    # the synthesiser writes the same names and shapes (so the weights it makes load with strict=True)
    assert got == [[k, list(s), d] for k, s, d in fc.i3d_state_dict_spec(nc)]
    I3D(nc).load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fc.i3d_state_dict(1, nc).items()}, strict=True)


def test_other_modalities_are_not_built():
    with pytest.raises(NotImplementedError):
        I3D(400, "flow")


@pytest.mark.parametrize("T", [16, 9, 10, 17])
def test_same_padding_and_shape_arithmetic_vs_reference_shapes(T):
    _, meta = fc.load_fixture("fvd_shapes")
    assert meta["H"] == 224 and endpoint_shapes(T, 224, 224) == meta["shapes"][str(T)]


def test_endpoint_shapes_of_the_i3d_fixtures():
    for name in ("fvd_i3d_t16", "fvd_i3d_t9", "fvd_i3d_128"):
        _, meta = fc.load_fixture(name)
        want = {k: v["shape"] for k, v in meta["endpoints"].items()}
        assert endpoint_shapes(meta["clips"]["t"], batch=meta["clips"]["n"]) == want, name


def test_frechet_distance_vs_reference():
    """Gate: 10 x the distance between the eigenvalue formulation and the reference's sqrtm formulation measured on the CPU when the fixture
    was made (meta eigh_vs_sqrtm_rel = 1.14e-13 -> 1.14e-12 relative); both are float64 evaluations of the same quantity."""
    arr, meta = fc.load_fixture("fvd_frechet")
    a1, a2 = fc.frechet_sets(meta["sets"]["seed"], meta["sets"]["n"], meta["sets"]["d"])
    got = fvd.calculate_frechet_distance(a1.mean(0), np.cov(a1, rowvar=False), a2.mean(0), np.cov(a2, rowvar=False))
    ref = float(arr["reference"][0])
    dev = abs(got - ref) / abs(ref)
    print(f"frechet: got {got!r}, reference {ref!r}, relative deviation {dev:.3e} (measured at fixture time {meta['eigh_vs_sqrtm_rel']:.3e})")
    assert meta["eigh_vs_sqrtm_rel"] > 0
    assert dev <= 10 * meta["eigh_vs_sqrtm_rel"]
    # through (n, sum, gram), the accumulator's route: the gram subtraction costs digits (|mu|^2 / var ~ 1 here), float64 leaves ~1e-12
    mu, sig = fvd.stats_from_sums(a1.shape[0], a1.sum(0), a1.T @ a1)
    mu2, sig2 = fvd.stats_from_sums(a2.shape[0], a2.sum(0), a2.T @ a2)
    assert abs(fvd.calculate_frechet_distance(mu, sig, mu2, sig2) - ref) / abs(ref) < 1e-10


def test_frechet_closed_form():
    """Equal covariances: the distance is ||mu1 - mu2||^2 exactly; gate = the same 10 x figure relative to tr(S1) + tr(S2), the size of
    the terms that cancel."""
    arr, meta = fc.load_fixture("fvd_frechet")
    m1, sig, m2, exact = fc.frechet_closed_form(meta["closed_form"]["seed"])
    got = fvd.calculate_frechet_distance(m1, sig, m2, sig)
    print(f"closed form: got {got!r}, exact {exact!r}, reference {float(arr['reference'][1])!r}")
    assert abs(exact - float(arr["reference"][2])) == 0
    assert abs(got - exact) <= 10 * meta["eigh_vs_sqrtm_rel"] * (2 * np.trace(sig) + exact)


def test_frechet_rank_deficient_and_identical_sets():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((20, 64)), rng.standard_normal((20, 64)) + 0.5     # N < D: singular covariances
    v = fvd.calculate_frechet_distance(a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False))
    assert np.isfinite(v) and v >= 0
    same = fvd.calculate_frechet_distance(a.mean(0), np.cov(a, rowvar=False), a.mean(0), np.cov(a, rowvar=False))
    # identical singular sets: every null direction of S carries an eigenvalue error ~ eps * lambda_max^2 in S^(1/2) S S^(1/2), whose square
    # root is sqrt(eps) * lambda_max -- not eps: the bound is 2 D sqrt(eps) lambda_max
    lam = np.linalg.eigvalsh(np.cov(a, rowvar=False)).max()
    assert abs(same) < 2 * 64 * np.sqrt(np.finfo(np.float64).eps) * lam
    c = rng.standard_normal((200, 16))
    assert abs(fvd.calculate_frechet_distance(c.mean(0), np.cov(c, rowvar=False), c.mean(0), np.cov(c, rowvar=False))) < 1e-10


def test_accumulator_state_round_trip_and_compute_on_host_state():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((30, 16)), rng.standard_normal((25, 16)) * 1.5 + 0.3
    model = I3D(16)
    acc = fvd.FVDAccumulator(model)
    acc.load_state({"gen": {"n": 30, "sum": a.sum(0), "gram": a.T @ a}, "orig": {"n": 25, "sum": b.sum(0), "gram": b.T @ b}}, device="cpu")
    st = acc.state()
    assert st["gen"]["n"] == 30 and np.array_equal(st["gen"]["sum"], a.sum(0)) and np.array_equal(st["orig"]["gram"], b.T @ b)
    acc2 = fvd.FVDAccumulator(model)
    acc2.load_state(st, device="cpu")
    want = fvd.calculate_frechet_distance(a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False))
    assert acc2.compute() == acc.compute() and abs(acc.compute() - want) < 1e-10 * abs(want)
    # the real set's statistics alone can be carried across epochs
    acc3 = fvd.FVDAccumulator(model)
    acc3.load_state(acc.state("orig"), device="cpu")
    with pytest.raises(ValueError):
        acc3.compute()
    with pytest.raises(ValueError):
        acc3.load_state({"orig": {"n": 3, "sum": np.zeros(4), "gram": np.zeros((4, 4))}}, device="cpu")


def test_product_path_refuses_to_run_without_a_gpu():
    model = I3D(16).eval()
    clips = torch.zeros(2, 16, 3, 32, 32)
    with pytest.raises(i2v_native.I2VError):
        model(clips.permute(0, 2, 1, 3, 4))
    with pytest.raises(i2v_native.I2VError):
        fvd.FVDAccumulator(model).update(clips, "gen")
    with pytest.raises(i2v_native.I2VError):
        fvd.calculate_FVD(model, clips, clips, 2, cuda=False)
    from utils import auxiliaries as aux
    with pytest.raises(NotImplementedError, match="DTFVD"):
        aux.evaluate_FVD_prior([], None, None, model, 64, None, 0, "DTFVD", False)
    with pytest.raises(NotImplementedError, match="DTFVD"):
        aux.evaluate_FVD_posterior([], None, None, model, "DTFVD")


def test_header_symbols_and_sources():
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    declared = set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    lib = i2v_native.lib()
    for name in FVD_SYMBOLS:
        assert name in declared and name in i2v_native.SYMBOLS and hasattr(lib, name), name
    assert "metrics/PyTorch_FVD/I3D.py" in header and "FVD_logging" in header
    i3d = open(os.path.join(PKG, "csrc", "i2v_i3d.hip")).read()
    assert '#include "i2v_flatconv.h"' in i3d                       # its conv kernel and the packing: checked with it
    src = i3d + "".join(open(os.path.join(PKG, "csrc", f)).read() for f in ("i2v_flatconv.h", "i2v_flatconv_pack.h"))
    assert "getenv" not in src and "atomic" not in src.replace("no atomics", "")
    assert "mfma_f32_16x16x4f32" in src
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_i3d.hip" in mk.split("SRCS =")[1].splitlines()[0]
    assert {"i2v_flatconv.h", "i2v_flatconv_pack.h"} <= set(mk.split("HDRS =")[1].splitlines()[0].split())
    pkg_fvd = open(os.path.join(PKG, "metrics", "PyTorch_FVD", "FVD_logging.py")).read()
    assert not re.search(r"^\s*(import|from) scipy", pkg_fvd, flags=re.M)


def test_i3d_code_object_uses_no_scratch(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    asm = tmp_path / "i3d.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(PKG, "csrc", "i2v_i3d.hip"),
                    "-o", str(asm)], check=True)
    text = asm.read_text()
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text)]
    assert len(sizes) >= 8 and all(v == 0 for v in sizes) and all(v == 0 for v in spills), (sizes, spills)
    assert "v_mfma_f32_16x16x4_f32" in text or "v_mfma_f32_16x16x4f32" in text
