"""CPU checks of the packing that the I3D and the Inception-v3 trunks share (csrc/i2v_flatconv_pack.h): tests/flatconv_host_check.cpp,
plain C++, must reproduce the packed weights, the (scale, shift) pairs and the metadata recorded in
tests/golden/flatconv_pack_digests.json from the two Unit::pack bodies the networks had BEFORE they shared it (its header says how)."""
import json
import os
import shutil
import subprocess

import pytest

import fid_common
import fvd_common
import i3d_units_common as uc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "image2video-synthesis-using-cinns_amd", "csrc")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("flatconv_host_check") / "flatconv_host_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + CSRC, os.path.join(REPO, "tests", "flatconv_host_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {"pack": {}, "tile": {}}
    for line in out.stdout.splitlines():
        kind, name, rest = line.split(" ", 2)
        assert name not in got[kind], name
        got[kind][name] = rest
    return got


def test_packed_units_are_the_parents(host_check):
    """cin 3, 16, 24, 48, 80 x cout 32, 48, 112, 192, 400 x the windows 1x1x1, 3x3x3, 7x7x7 (3 channels) with a BatchNorm at eps 1e-3 and
    1e-5, a bias and the identity, and 1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1 with a BatchNorm at eps 1e-3; LCG weights, an all-zero unit and
    one with 1e20 entries: the same bytes and metadata as the code of either network gave."""
    want = json.load(open(os.path.join(REPO, "tests", "golden", "flatconv_pack_digests.json")))["pack"]
    assert len(want) == 3 * 5 * (19 + 4 * 15) and set(host_check["pack"]) == set(want)
    bad = {k: (host_check["pack"][k], v) for k, v in want.items() if host_check["pack"][k] != v}
    assert not bad, bad


def test_both_networks_pack_a_1x1_window_alike(host_check):
    """The one case both networks had: a 1x1x1 unit of the I3D and a 1x1 unit of Inception with the same BatchNorm are the same bytes."""
    pack = host_check["pack"]
    pairs = [(k, k.replace("k1x1_", "k1x1x1_")) for k in pack if k.startswith("k1x1_")]
    assert len(pairs) == 3 * 5 * 5
    assert all(pack[a] == pack[b] for a, b in pairs)


def network_couts():
    couts = {64, 192, *uc.CLASSES.values()}                        # the I3D stem, 2b, 2c and the two heads
    couts.update(o for _, _, outs in fvd_common.MIXED for o in outs)
    couts.update(u[2] for u in fid_common.units())
    return sorted(couts)


def test_column_tile_of_every_network_width(host_check):
    """The tile of 128, 64, 32 that pads Cout least, the wider on a tie, for every Cout of the I3D networks and of Inception-v3."""
    couts = network_couts()
    assert {16, 18, 24, 48, 80, 96, 112, 144, 208, 288, 320, 400, 448} <= set(couts)
    for cout in couts:
        padded = {bn: (cout + bn - 1) // bn * bn for bn in (128, 64, 32)}
        want = max(bn for bn in padded if padded[bn] == min(padded.values()))
        assert int(host_check["tile"][str(cout)]) == want, (cout, want)
    tile = {c: int(host_check["tile"][str(c)]) for c in couts}
    assert (tile[16], tile[48], tile[64], tile[96], tile[112], tile[128], tile[192], tile[208], tile[384], tile[400]) == \
        (32, 64, 64, 32, 128, 128, 64, 32, 128, 32)
