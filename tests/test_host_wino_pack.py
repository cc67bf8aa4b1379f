"""CPU checks of the conv kernels' host code after it was folded into one packer (csrc/i2v_wino_pack.h) and one F(4,3) launch plan
(wino4_plan, csrc/i2v_conv16w4.hip): tests/wino_host_check.hip, compiled for the host, must reproduce the packed bytes and the
launch plans recorded in tests/golden/wino_pack_digests.json from the code BEFORE the fold (its header says how)."""
import json
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("wino_host_check") / "wino_host_check"
    csrc = os.path.join(PKG, "csrc")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-DW4_HOST_ONLY", "-I" + csrc, "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "wino_host_check.hip"), os.path.join(csrc, "i2v_conv16w4.hip"), os.path.join(csrc, "i2v_common.hip"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=900)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {"pack": {}, "plan": {}}
    for line in out.stdout.splitlines():
        kind, name, rest = line.split(" ", 2)
        assert name not in got[kind], name
        got[kind][name] = rest
    return got


def golden():
    return json.load(open(os.path.join(REPO, "tests", "golden", "wino_pack_digests.json")))


def test_packed_bytes_are_the_parents(host_check):
    """Every packer (split F(2,3), split F(4,3), one-term F(4,3), the direct split-fp16 kernel's, the fp32 F(4,3) planes), plain and
    temporal-duplication, both signs of the scale, an all-zero tensor and one with a 1e20 entry: the same bytes and metadata."""
    want = golden()["pack"]
    assert len(want) == 120 and set(host_check["pack"]) == set(want)
    bad = {k: (host_check["pack"][k], v) for k, v in want.items() if host_check["pack"][k] != v}
    assert not bad, bad


def test_launch_plans_are_the_parents(host_check):
    """Every F(4,3) layer of the BAIR nf = 64 decoder (64 x 64, T = 16) and of the 128 x 128 nf = 32 decoder from g_1 on, SPADE's 1x3x3
    gamma | beta convs included, at B = 1, 8, 32, 64 on 256 CUs with default switches, in the split and the one-term form: the same
    argument block and kernel instantiation as the two forwards computed separately."""
    want = golden()["plan"]
    assert len(want) == 160 and set(host_check["plan"]) == set(want)
    bad = {k: (host_check["plan"][k], v) for k, v in want.items() if host_check["plan"][k] != v}
    assert not bad, bad


def test_split_and_one_term_plans_agree(host_check):
    """The one-term forward promised "the production geometry of wino4_forward": per layer and batch the two forms must agree in the
    tile width, the workgroup size, the brick and the grid (they differ in the chunk count and the weight-set stride only)."""
    plans = host_check["plan"]
    pairs = 0
    for name, split in plans.items():
        if "_split_" not in name or "_spade_" in name:   # (SPADE's 1x3x3 convs exist in the split form only)
            continue
        one = plans[name.replace("_split_", "_one_")]
        assert split != "error" and one != "error", name
        fs, fo = (dict(kv.split("=") for kv in p.split()) for p in (split, one))
        for key in ("BN", "NTH", "NT", "TT", "TH", "TJ", "nbT", "nbH", "nbJ", "grid", "nvirt", "lds", "tofs", "th_shift", "hh_magic"):
            assert fs[key] == fo[key], (name, key, fs[key], fo[key])
        cin = int(fs["Cin"])   # chunks of 16 channels against chunks of 32 over Cin padded to 64
        assert int(fs["nchunk"]) == cin // 16 and int(fo["nchunk"]) == (cin + 63) // 64 * 2, name
        pairs += 1
    assert pairs == 2 * 4 * 2 * 4   # decoders x blocks x convs x batches
    # the table crosses both decisions: 64 -> 32 channel narrowing and the 256-thread form
    assert {re.search(r"BN=(\d+) NTH=(\d+)", p).groups() for p in plans.values() if p != "error"} == {("64", "512"), ("32", "512"), ("32", "256")}
