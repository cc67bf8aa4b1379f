"""Static checks of the F(4,3) operand writer (modulate_wino4_kernel, csrc/i2v_dec_writers.hip) as the production library compiles it: 16-byte
stores behind a DPP pair exchange; no scratch, and registers for the occupancy the writer had
with 8-byte stores: 3 waves per SIMD where SPADE's maps are held per position (<= 168 VGPRs), 4 where they are not (<= 128)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG


@pytest.fixture(scope="module")
def writer_kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("asm") / "i2v_dec_writers.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(PKG, "csrc"), "-S", "--cuda-device-only",
                    os.path.join(PKG, "csrc", "i2v_dec_writers.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    bodies = dict(re.findall(r"^(\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel", out.read_text(), flags=re.S | re.M))
    return {n: b for n, b in bodies.items() if "modulate_wino4_kernelILb" in n}


def test_writer_occupancy_and_no_scratch(writer_kernels):
    found = set()
    for name, body in writer_kernels.items():
        gb, one, sh = re.search(r"modulate_wino4_kernelILb([01])ELb([01])ELb([01])E", name).groups()
        found.add((gb, one, sh))
        assert "scratch_" not in body and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert [int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", body) if int(v)] == [], name
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        assert vgpr <= (168 if gb == "1" else 128), (name, vgpr)   # 512 registers per SIMD lane: 3 / 4 waves
    assert found == {("1", "0", "1"), ("1", "0", "0"), ("0", "0", "0"), ("1", "1", "1"), ("1", "1", "0"), ("0", "1", "0")}, found
    assert len(writer_kernels) == 6                               # one form per instantiation in the production library


def test_writer_store_shape(writer_kernels):
    """Every store of the frame loop is 16 bytes wide -- six per frame in the split form, three in the one-term form -- and the pair
    exchange is DPP (quad_perm [1, 0, 3, 2]), not LDS."""
    for name, body in writer_kernels.items():
        one = re.search(r"modulate_wino4_kernelILb[01]ELb([01])E", name).group(1) == "1"
        stores = re.findall(r"\bglobal_store_(\w+)", body)
        assert stores.count("dwordx4") == (3 if one else 6), (name, stores)
        assert "dwordx2" not in stores, (name, stores)
        assert len(re.findall(r"_dpp [^\n]*quad_perm:\[1,0,3,2\]", body)) >= (6 if one else 12), name


def test_form_switch_only_in_the_measurement_build():
    import i2v_native
    src = open(os.path.join(PKG, "csrc", "i2v_dec_writers.hip")).read()
    at = src.index('getenv("I2V_MOD4_FORM")')
    assert src.rfind("#ifdef I2V_MEASURE", 0, at) > src.rfind("#endif", 0, at)
    if os.path.exists(i2v_native.LIB_PATH):
        assert b"I2V_MOD4_FORM" not in open(i2v_native.LIB_PATH, "rb").read()
    if os.path.exists(i2v_native.MEASURE_LIB_PATH):
        assert b"I2V_MOD4_FORM" in open(i2v_native.MEASURE_LIB_PATH, "rb").read()
