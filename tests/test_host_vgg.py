"""CPU-side checks of the VGG / LPIPS surface: the float64 oracle of tests/vgg_common.py against the fixtures written from the reference's
own modules, the deliberate errors the gates have to catch, the new native symbols, the holders' key lists, the refusals and the CLIs."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import i2v_native
import vgg_common as vc
from conftest import PKG, REPO
from metrics.Diversity.VGG import compute_vgg_diversity
from stage2_cINN.AE.modules import LPIPS as lpips_mod
from stage2_cINN.AE.modules import vgg16 as vgg_mod

NEW_SYMBOLS = ["i2v_vgg_create", "i2v_vgg_destroy", "i2v_vgg_load", "i2v_vgg_lin", "i2v_vgg_workspace_bytes", "i2v_vgg_input_stage", "i2v_vgg_features",
               "i2v_vgg_conv_unit", "i2v_vgg_maxpool2", "i2v_vgg_reduce_workspace_bytes", "i2v_lpips_layer", "i2v_vgg_pairdiff_update", "i2v_vgg_saved_layout"]


# ---------------------------------------------------------------------------------------------------------------- oracle vs fixtures

@pytest.mark.parametrize("fixture", ["vgg_taps_16", "vgg_taps_odd"])
def test_oracle_taps_match_the_reference(fixture):
    arr, meta = vc.load_fixture(fixture)
    x = vc.randn(meta["input"]["seed"], tuple(meta["input"]["shape"]))
    taps = vc.trunk_oracle(vc.vgg_state_dict(meta["weights"]["seed"]), x)
    for name, t in zip(vc.TAPS, taps):
        assert list(t.shape) == meta["taps"][name]["shape"] == list(arr[name].shape)
        assert vc.rel_l2(arr[name], t) <= 1e-5, name          # the reference ran in fp32
    if fixture == "vgg_taps_odd":
        assert [meta["taps"][n]["shape"][2:] for n in vc.TAPS] == [[35, 29], [17, 14], [8, 7], [4, 3], [2, 1]]
    assert [k for k, _ in meta["state_dict"]] == vc.holder_keys()


def test_oracle_at_224_matches_the_reference_and_tells_align_corners_apart():
    arr, meta = vc.load_fixture("vgg_224")
    f = meta["frame"]
    frame = torch.from_numpy(vc.clips(f["seed"], 1, 1, f["h"], f["w"]))[0]
    sd = vc.vgg_state_dict(meta["weights"]["seed"])
    got = {ac: vc.trunk_oracle(sd, vc.input_oracle(frame, "diversity", (224, 224), bool(ac))) for ac in (0, 1)}
    for ac in (0, 1):
        assert vc.rel_l2(arr[f"relu5_3_ac{ac}"], got[ac][4]) <= 1e-5
        for name, t in zip(vc.TAPS, got[ac]):
            st = meta["taps"][f"ac{ac}"][name]
            assert list(t.shape) == st["shape"] and abs(float(t.norm()) - st["l2"]) <= 1e-5 * st["l2"]
        assert vc.rel_l2(arr[f"relu5_3_ac{1 - ac}"], got[ac][4]) > vc.TOL_L2        # align_corners flipped: rejected at the 1e-4 gate
    x = torch.from_numpy(vc.clips(3, 1, 1, 16, 16))[0]
    a, b = vc.input_oracle(x, "diversity", (224, 224), False), vc.input_oracle(x, "diversity", (224, 224), True)
    assert vc.rel_l2(a, b) > 1e-4                                                   # ... and at the input stage's 1e-6 gate


def test_oracle_lpips_and_diversity_match_the_reference():
    arr, meta = vc.load_fixture("vgg_lpips")
    sd, lin = vc.vgg_state_dict(meta["weights"]["seed"]), vc.lin_state_dict(meta["weights"]["lin_seed"])
    assert [k for k, _ in meta["state_dict"]] == vc.lpips_keys()
    for tag, seed in (("32x32", meta["first_seed"]), ("24x40", meta["first_seed"] + 2)):
        sz, n = meta["sizes"][tag], meta["n"]
        a = torch.from_numpy(vc.clips(seed, n, 1, sz["h"], sz["w"]))[:, 0]
        b = (0.7 * a + 0.3 * torch.from_numpy(vc.clips(seed + 1, n, 1, sz["h"], sz["w"]))[:, 0]).contiguous()
        got = vc.lpips_oracle(sd, lin, a, b).numpy()
        assert np.max(np.abs(got - arr[f"lpips64_{tag}"]) / arr[f"lpips64_{tag}"]) <= 1e-9
        assert np.max(np.abs(got - arr[f"lpips32_{tag}"]) / got) <= sz["per_image_gate"]["gate_rel"]
        assert vc.lpips_score_rule(arr[f"lpips32_{tag}"]) == sz["score_fp32"] and vc.lpips_score_rule(arr[f"lpips64_{tag}"]) == sz["score_fp64"]
        assert vc.lpips_score_rule(arr[f"lpips64_{tag}"]) == float(arr[f"lpips64_{tag}"][:10].mean())      # 12 images: the last two are dropped
        for g in (sz["gate"], sz["per_image_gate"]):
            assert g["gate_rel"] == (1e-6 if g["measured"] < 1e-7 else 10 * g["measured"])
    arr, meta = vc.load_fixture("vgg_diversity")
    c = meta["clips"]
    videos = torch.from_numpy(vc.clips(c["seed"], c["n"] * c["r"], c["t"], c["h"], c["w"])).reshape(c["n"], c["r"], c["t"], 3, c["h"], c["w"])
    got = vc.diversity_oracle(vc.vgg_state_dict(meta["weights"]["seed"]), videos)
    assert abs(got - meta["diversity_fp64"]) <= 1e-9 * got and abs(got - meta["diversity_fp32"]) <= meta["gate"]["gate_rel"] * got
    assert arr["terms64"].shape == (c["n"] * c["r"] * (c["r"] - 1) * 5,) and float(arr["terms64"].mean()) == meta["diversity_fp64"]
    r = meta["ref_fp32_vs_fp64_rel"]
    assert meta["gate"]["gate_rel"] == (1e-6 if r < 1e-7 else 10 * r)
    assert abs(vc.diversity_oracle(vc.vgg_state_dict(meta["weights"]["seed"]), videos, align_corners=True) - got) > meta["gate"]["gate_rel"] * got


# ---------------------------------------------------------------------------------------------------------------- what the gates catch

def _fp32_conv(x, w, b):
    return torch.relu(torch.nn.functional.conv2d(x, w, b, padding=1))


@pytest.mark.parametrize("cin,cout,hw", [(3, 64, (9, 17)), (16, 64, (5, 7)), (64, 64, (13, 21))])
def test_unit_gate_accepts_fp32_and_rejects_deliberate_errors(cin, cout, hw):
    case = {"cin": cin, "cout": cout, "hw": hw, "batch": 2, "seed": 9100 + cin}
    x, (w, b) = vc.conv_input(case), vc.conv_params(case)
    ref, S, n = vc.conv_oracle(x, w, b)
    assert n == 9 * (4 if cin == 3 else cin) + 1
    ok, ratio, l2 = vc.gate(_fp32_conv(x, w, b), ref, S, n)
    assert ok, (ratio, l2)
    for m in vc.MUTATIONS:
        if m == "transposed_kernel" and cin != cout:
            continue
        bad = vc.conv_oracle(x, w, b, mutate=m)[0]
        ok, ratio, l2 = vc.gate(bad.float(), ref, S, n)
        assert not ok, m


def test_pool_input_and_normalisation_errors_are_rejected():
    x = vc.randn(9200, (1, 8, 7, 9))
    assert torch.equal(vc.maxpool_oracle(x), torch.nn.functional.max_pool2d(x, 2, 2)) and tuple(vc.maxpool_oracle(x).shape) == (1, 8, 3, 4)
    bad = vc.maxpool_oracle(x, "pool_stride1")
    assert tuple(bad.shape) != tuple(vc.maxpool_oracle(x).shape)                     # a pool at stride 1: the shape already differs
    assert not vc.gate_bound(bad, vc.maxpool_oracle(x).double(), torch.zeros(1))[0]
    f0, f1 = torch.relu(vc.randn(9201, (2, 64, 3, 3))), torch.relu(vc.randn(9202, (2, 64, 3, 3)))
    f0[0, :, 0, 0] = 0
    lin = torch.from_numpy(vc.lin_state_dict(1)["lin0.model.1.weight"]).flatten()
    assert torch.isfinite(vc.lpips_layer_oracle(f0, f1, lin)).all()
    assert not torch.isfinite(vc.lpips_layer_oracle(f0, f1, lin, eps=0.0)).all()     # no eps: 0 / 0 at the all-zero feature vector
    ref = vc.lpips_layer_oracle(f0, f1, lin)
    fp32 = (((vgg_mod.normalize_tensor(f0) - vgg_mod.normalize_tensor(f1)) ** 2) * lin.view(1, -1, 1, 1)).sum(1, keepdim=True)
    assert float(((vgg_mod.spatial_average(fp32).flatten().double() - ref).abs() / ref).max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- surface

def test_header_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    declared = set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    lib = i2v_native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in i2v_native.SYMBOLS and hasattr(lib, name), name
    for ref in ("stage2_cINN/AE/modules/vgg16.py", "stage2_cINN/AE/modules/LPIPS.py", "metrics/Diversity/VGG.py", "ScalingLayer", "normalize_tensor"):
        assert ref in header, ref
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_vgg.hip" in makefile and "i2v_lpips.hip" in makefile and "i2v_vgg_plan.h" in makefile
    for name in ("vgg16.py", "LPIPS.py"):
        text = open(os.path.join(PKG, "stage2_cINN", "AE", "modules", name)).read()
        assert not re.search(r"^\s*(import|from) (torchvision|requests|kornia|lpips)", text, flags=re.M), name
    assert not os.path.exists(os.path.join(PKG, "stage2_cINN", "AE", "modules", "ckpt_util.py"))


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_layer_plan_equals_the_rules_the_entries_spelled_out(tmp_path, san):
    """tests/vgg_plan_host_check.cpp: vgg_plan of csrc/i2v_vgg_plan.h at 4 batch sizes x 10 x 10 maps against the slot-sizing loop, the
    saved-offset loop, the forward's pointer comparison and the backward's two halves, written out independently -- the three byte
    totals, every offset, every layer's map and the destination of every conv and pool with and without saved state.  A stand-alone
    host program; with the sanitizers it is built with them and run directly.  `--perturb` (slots a and b of one layer swapped) has
    to be counted: the check is not blind."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path / "vgg_plan_host_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if san else ["-O1"]
    r = subprocess.run([hipcc, "-std=c++17", "-Wall", "-Werror", "--offload-arch=gfx950"] + flags + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(REPO, "include"),
                        "-x", "hip", os.path.join(REPO, "tests", "vgg_plan_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    if san and r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libclang_rt\.\w+san", r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    m = re.search(r"(\d+) shapes, (\d+) checks, 0 mismatches: ok", out.stdout)
    assert m and int(m.group(1)) == 4 * 10 * 10 and int(m.group(2)) > 200 * int(m.group(1)), out.stdout
    bad = subprocess.run([str(exe), "--perturb"], capture_output=True, text=True, timeout=300)
    m = re.search(r"(\d+) shapes, \d+ checks, (\d+) mismatches: FAILED", bad.stdout)
    assert bad.returncode != 0 and m and int(m.group(2)) >= int(m.group(1)), bad.stdout + bad.stderr


@pytest.mark.parametrize("n,h,w", [(3, 16, 16), (2, 35, 29), (1, 24, 40)])
def test_saved_layout_query_equals_the_rule_the_binding_used_to_carry(n, h, w):
    """i2v_vgg_saved_layout (a host function: no device) against the table and the 256-byte rule VGGSaved.activations spelled out
    before it asked the library, and against tap_shapes."""
    if not os.path.exists(i2v_native.LIB_PATH):
        pytest.skip("library not built")
    lay = (i2v_native.VGGLayer * 13)()
    assert i2v_native.lib().i2v_vgg_saved_layout(n, h, w, lay) == 0
    layers = ((64, -1, 0), (64, 0, 1), (128, -1, 0), (128, 1, 1), (256, -1, 0), (256, -1, 0), (256, 2, 1), (512, -1, 0), (512, -1, 0), (512, 3, 1),
              (512, -1, 0), (512, -1, 0), (512, 4, 0))
    shapes, off, hh, ww = i2v_native.NativeVGG.tap_shapes(n, h, w), 0, h, w
    for l, (cout, tap, pool) in enumerate(layers):
        assert (lay[l].h, lay[l].w, lay[l].cout, lay[l].tap, lay[l].offset) == (hh, ww, cout, tap, off), l
        if tap >= 0:
            assert shapes[tap] == (n, hh, ww, cout)
        else:
            off += (n * hh * ww * cout * 4 + 255) // 256 * 256
        if pool:
            hh, ww = hh // 2, ww // 2
    assert i2v_native.lib().i2v_vgg_saved_layout(n, 15, w, lay) != 0 and i2v_native.lib().i2v_vgg_saved_layout(0, h, w, lay) != 0
    assert i2v_native.lib().i2v_vgg_saved_layout(n, h, w, None) != 0


def test_holders_keep_the_reference_keys_and_load_files(tmp_path):
    _, meta = vc.load_fixture("vgg_taps_16")
    m = vgg_mod.vgg16(pretrained=False)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    path = str(tmp_path / "vgg16.pth")
    sd = {k: torch.from_numpy(v) for k, v in vc.vgg_state_dict(5).items()}
    sd["classifier.0.weight"] = torch.zeros(2, 2)                                   # ignored
    torch.save(sd, path)
    m = vgg_mod.vgg16(path=path)
    assert torch.equal(getattr(m.slice5, "28").bias, sd["features.28.bias"]) and torch.equal(getattr(m.slice1, "0").weight, sd["features.0.weight"])
    assert set(m.torchvision_state_dict()) == set(vc.vgg_state_dict(5)) and not any(p.requires_grad for p in m.parameters())
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        vgg_mod.vgg16(path=str(tmp_path / "nowhere.pth"))
    with pytest.raises(FileNotFoundError, match="vgg16-397923af.pth"):
        vgg_mod.vgg16()
    with pytest.raises(NotImplementedError):
        vgg_mod.vgg16(requires_grad=True, pretrained=False)
    _, lmeta = vc.load_fixture("vgg_lpips")
    lin_path = str(tmp_path / "vgg.pth")
    vc.save_lin_file(lin_path, 6)
    lp = lpips_mod.LPIPS(vgg_path=path, lin_path=lin_path)
    assert [[k, list(v.shape)] for k, v in lp.state_dict().items()] == lmeta["state_dict"]
    assert torch.equal(lp.lin3.model[1].weight, torch.from_numpy(vc.lin_state_dict(6)["lin3.model.1.weight"]))
    assert torch.equal(lp.scaling_layer.shift.flatten(), torch.Tensor(vc.LPIPS_SHIFT))
    with pytest.raises(FileNotFoundError, match="missing.pth"):
        lpips_mod.LPIPS(vgg_path=path, lin_path=str(tmp_path / "missing.pth"))


def test_refusals_without_a_gpu():
    x = torch.zeros(1, 2, 2, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="torchvision"):
        compute_vgg_diversity(x)
    m = vgg_mod.vgg16(pretrained=False)
    with pytest.raises(i2v_native.I2VError):
        compute_vgg_diversity(x, m)
    with pytest.raises(i2v_native.I2VError):
        m(torch.zeros(1, 3, 16, 16))
    with pytest.raises(i2v_native.I2VError):
        lpips_mod.LPIPS()(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    with pytest.raises(i2v_native.I2VError):
        i2v_native.vgg_input_stage(torch.zeros(1, 3, 16, 16), i2v_native.VGG_INPUT_LPIPS)


def test_lpips_score_drops_the_tail_and_refuses_fewer_than_one_batch():
    calls = []

    def fake(pd, gt):
        calls.append(pd.shape[0])
        return (pd - gt).abs().mean((1, 2, 3), keepdim=True)
    pd, gt = torch.arange(25.0).view(25, 1, 1, 1).expand(25, 3, 2, 2), torch.zeros(25, 3, 2, 2)
    assert lpips_mod.lpips_score(fake, pd, gt) == pytest.approx((4.5 + 14.5) / 2) and calls == [10, 10]
    assert lpips_mod.lpips_score(fake, pd[:12], gt[:12]) == pytest.approx(4.5)
    with pytest.raises(ValueError, match="fewer"):
        lpips_mod.lpips_score(fake, pd[:9], gt[:9])
    with pytest.raises(ValueError):
        lpips_mod.lpips_score(fake, pd, gt[:20])


@pytest.mark.parametrize("script,argv,word", [
    ("eval_synthesis_quality.py", ["-LPIPS", "True"], "-LPIPS is not built: "),
    ("eval_synthesis_quality.py", ["-LPIPS", "True", "-vgg_path", "a.pth"], "-lpips_path"),
    ("eval_synthesis_quality.py", ["-LPIPS", "True", "-vgg_path", "a.pth", "-lpips_path", "b.pth"], "-clips_npy"),
    ("eval_synthesis_quality.py", ["-FID", "True", "-LPIPS", "True", "-vgg_path", "a.pth", "-lpips_path", "b.pth"], "-FID is not built"),
    ("eval_synthesis_quality.py", [], "-LPIPS True -vgg_path FILE -lpips_path FILE"),
    ("eval_diversity.py", ["-dataset", "DTDB", "-VGG", "True"], "-VGG is not built: "),
    ("eval_diversity.py", ["-dataset", "DTDB", "-VGG", "True"], "-vgg_path"),
    ("eval_diversity.py", ["-dataset", "DTDB", "-VGG", "True", "-vgg_path", "a.pth"], "-clips_npy"),
    ("eval_diversity.py", ["-dataset", "DTDB", "-I3D", "True", "-VGG", "True", "-vgg_path", "a.pth"], "-I3D is not built"),
    ("eval_diversity.py", ["-dataset", "DTDB"], "-VGG True -vgg_path FILE"),
])
def test_cli_refusals(script, argv, word):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "-gpu", "0"] + argv, capture_output=True, text=True, cwd=PKG)
    assert r.returncode != 0 and word in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("script,flags", [("eval_synthesis_quality.py", ["-vgg_path", "-lpips_path", "-LPIPS"]), ("eval_diversity.py", ["-vgg_path", "-VGG"])])
def test_cli_help_lists_the_new_flags(script, flags):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True, cwd=PKG)
    assert r.returncode == 0, r.stderr
    for f in flags:
        assert re.search(rf"(^|\s){f}\b", r.stdout), f
