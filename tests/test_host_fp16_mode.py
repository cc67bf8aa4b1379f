"""CPU checks of the opt-in half-precision decoder mode (mma = 3, "fp16"): its spelling in the Python surface, the header and the
integration notes, the kernel symbol in the production library, and static checks of the one-term F(4,3) kernel's compiled loops
(csrc/i2v_conv16w4h.hip) with the same replay of the hand-counted waits as the split kernel's."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

KERNEL = "conv_wino4_f16_kernel"


def test_fp16_mode_spelling():
    import i2v_native
    assert i2v_native.parse_mma("fp16") == 3 and i2v_native.parse_mma(" FP16 ") == 3 and i2v_native.parse_mma(3) == 3
    assert i2v_native.parse_mma("auto") == 2 and i2v_native.parse_mma("1") == 1
    assert i2v_native.NativeDecoder.KERNEL_NAMES[6] == "conv_wino4_f16"
    hdr = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    assert '"fp16"' in hdr and "3 = " in hdr
    integ = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "fp16" in integ and "mma = 3" in integ
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "i2v_conv16w4h.hip" in mk.split("SRCS =")[1].splitlines()[0]


def test_fp16_mode_default_unchanged(monkeypatch):
    import i2v_native
    monkeypatch.delenv("I2V_DEC_MMA", raising=False)
    assert i2v_native.default_mma() == 1
    monkeypatch.setenv("I2V_DEC_MMA", "fp16")
    assert i2v_native.default_mma() == 3


def test_fp16_kernel_symbol_in_production_library():
    lib = os.path.join(PKG, "lib", "libi2v_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    data = open(lib, "rb").read()
    assert b"_ZN3i2v21conv_wino4_f16_kernelILi9ELi64ELi512EEEvNS_6W4ArgsE" in data
    assert data.count(b"_ZN3i2v21conv_wino4_f16_kernel") >= 6


def _waits(loop):
    return [int(w) for w in re.findall(r"s_waitcnt vmcnt\((\d+)\)", loop)]


def _loops(whole):
    return [mm.group(2) for mm in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n((?:(?!^\.LBB).)*?)s_cbranch_\w+ \1\n", whole, flags=re.S | re.M)
            if "v_mfma" in mm.group(2)]


def _asm(tmp_path, name):
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / (name + ".s")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(PKG, "csrc"), "-S", "--cuda-device-only",
                    os.path.join(PKG, "csrc", name + ".hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    return out.read_text()


def test_fp16_kernel_static_checks(tmp_path):
    """Every instantiation of the one-term kernel: no scratch, two tap loops (pass A: planes 0..3, pass B: planes 4, 5) with exactly
    the loads of the split kernel's loops (the same V bricks, two weight fragments per tap) and 2 WM MFMAs per tap, hand-counted waits
    that replay clean and tight (a wait relaxed by one is caught), loops entered with nothing in flight, no asm load reading a freshly
    VALU-written SGPR -- and per input channel one third of the split kernel's v_mfma_f32_32x32x16_f16."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_asm_waits as caw
    text = _asm(tmp_path, "i2v_conv16w4h")
    kernels = re.findall(r"^(_ZN3i2v21conv_wino4_f16_kernelILi(\d)ELi(\d+)ELi(\d+)EEEvNS_6W4ArgsE):[^\n]*\n(.*?)\.end_amdhsa_kernel",
                         text, flags=re.S | re.M)
    assert sorted((k[1], k[2], k[3]) for k in kernels) == sorted(
        [("9", "64", "512"), ("6", "64", "512"), ("9", "32", "512"), ("6", "32", "512"), ("9", "32", "256"), ("6", "32", "256")])
    assert "getenv" not in open(os.path.join(PKG, "csrc", "i2v_conv16w4h.hip")).read()
    mfma_per_chunk = {}
    for name, nt, bn, nth, whole in kernels:
        nt = int(nt)
        assert "scratch_" not in whole and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", whole), name
        loops = _loops(whole)
        assert len(loops) == 2, (name, len(loops))
        for loop, wm, vh2 in zip(loops, (4, 2) if bn == "64" else (2, 1), (9, 5) if nth == "256" else (8, 4)):
            taps = 2 * nt
            assert loop.count("v_mfma_f32_32x32x16_f16") == taps * 2 * wm, name
            mfma_per_chunk.setdefault((nt, bn, nth), []).append(loop.count("v_mfma_f32_32x32x16_f16"))
            assert len(re.findall(r"buffer_load_dwordx4 [^\n]* lds", loop)) == 2 * vh2, name
            assert len(re.findall(r"global_load_dwordx4", loop)) == taps * 2, name
            assert loop.count("s_barrier") == 2, name
            assert caw.check_loop(loop) == [], name
            b_wait, bar_wait = max(_waits(loop)), min(_waits(loop))
            for w in (b_wait, bar_wait):
                mutated = re.sub(r"s_waitcnt vmcnt\(%d\)" % w, "s_waitcnt vmcnt(%d)" % (w + 1), loop)
                assert caw.check_loop(mutated) != [], (name, w)
    assert caw.check_loop_entries(text, KERNEL) == []
    assert caw.check_scalar_operands(text, KERNEL) == []
    # against the split kernel: an iteration of either loop covers two K chunks -- 2 x 16 channels split, 2 x 32 one-term
    split = _asm(tmp_path, "i2v_conv16w4")
    for (nt, bn, nth), ns in mfma_per_chunk.items():
        m = re.search(r"^_ZN3i2v23conv_wino4_f16x3_kernelILi%dELi%sELi%sEEEvNS_6W4ArgsE:[^\n]*\n(.*?)\.end_amdhsa_kernel" % (nt, bn, nth),
                      split, flags=re.S | re.M)
        n_split = [lp.count("v_mfma_f32_32x32x16_f16") for lp in _loops(m.group(1))]
        assert len(n_split) == len(ns) == 2
        for n, n16 in zip(ns, n_split):
            assert 3 * n * 32 == n16 * 64, ((nt, bn, nth), n, n16)   # MFMAs per input channel: one third


def test_fp16_writer_keeps_the_range_guard():
    """The one-term writer is modulate_wino4_kernel<GB, ONE = true>: the same guard (bit 0 on |V| > 65504 or non-finite, the maximum
    |activation| into the layer's slot) as the split writer -- no separate kernel that could drop it."""
    src = open(os.path.join(PKG, "csrc", "i2v_dec_writers.hip")).read()
    body = src[src.index("__global__ __launch_bounds__(256) void modulate_wino4_kernel("):]
    body = body[:body.index("\n}\n")]
    assert "if constexpr (ONE)" in body and "atomicOr(range_flag, 1)" in body and "publish_umax(umax, vmax)" in body
    assert "modulate_wino4_kernel<true, true>" in src and "modulate_wino4_kernel<false, true>" in src
