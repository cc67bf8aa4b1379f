"""CPU checks of the F(4,3) kernel that skips the temporal taps reading only zero padding (csrc/i2v_conv16w4e.hip): the dead-unit rule
against a brute force over the staged rows (tests/f43_tskip_host_check.cpp, plain C++, also under the host sanitizers), and the static
checks of every compiled tap loop of the new translation unit -- the recipe of test_f43_kernel_keeps_its_hand_counted_waits_valid with
the MFMA and operand-read counts of each loop variant derived from the rule's closed form."""
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
CSRC = os.path.join(PKG, "csrc")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_dead_unit_rule_equals_the_brute_force(tmp_path, san):
    """T in {2, 4, 6, 8, 12, 16, 32} x KT in {2 (pairs, both parities), 3} x TH in {4, 8, 16, 32} x every t-brick: w4_unit_dead equals the
    enumeration of w4_tables' `ok` flag over every staged row a unit reads, the dead units per launch equal the closed form, the per-wave
    masks are the same bits, and the three wrong rules (pt off by one, parities swapped, a dead unit spanning two frames) are flagged.
    The same program, built stand-alone with -fsanitize=address,undefined and run directly, is clean."""
    exe = tmp_path / "f43_tskip_host_check"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O1"]
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + CSRC, os.path.join(REPO, "tests", "f43_tskip_host_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    if san and r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libclang_rt\.\w+san", r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    m = re.search(r"(\d+) units in (\d+) launches, (\d+) dead, (\d+) mismatches, (\d+) bad counts, (\d+) dead units spanning frames; "
                  r"controls flagged (\d+) / (\d+) / (\d+) \((\d+) spanning\): ok", out.stdout)
    assert m, out.stdout
    units, launches, dead, mism, badc, span, c1, c2, c3, c3s = map(int, m.groups())
    assert units > 10000 and launches >= 40 and dead > 0 and mism == badc == span == 0 and min(c1, c2, c3, c3s) > 0, out.stdout


def waits_of(loop):
    return [int(x) for x in re.findall(r"s_waitcnt vmcnt\((\d+)\)", loop)]


def _variants(kt, wm, tt):
    """Dead units (kt, wm) of the loop variants one pass of a wave with `wm` row blocks can run, from the geometry alone: a frame is
    4 / tt row blocks; front = kt 0 on the first frame's row blocks, back = kt KT - 1 on the last frame's -- of the row blocks the wave
    holds: all four (wm = 4), a half (2) or one (1) of the brick's.  Returns the sorted list of dead-unit counts, the full loop included."""
    rbpf = 4 // tt
    front, back = min(rbpf, wm), min(rbpf, wm)
    counts = [0, front, back]
    if wm == 4 and kt == 3:          # a wave that holds the whole brick of a clip of TT frames (3x3x3 only: pairs have one end per parity)
        counts.append(front + back)
    return sorted(counts)


def test_edge_kernel_loops_hold_what_the_rule_says(tmp_path):
    """Every instantiation of conv_wino4e_f16x3_kernel and of its one-term form conv_wino4e_f16_kernel (two MFMAs per product): no scratch, <= 256 VGPRs (two waves per SIMD at 512 threads); every MFMA loop is a
    single block that the replay of the in-order VMEM queue finds clean and tight; per loop variant the MFMA count is 3 (one-term: 2) x
    (taps WM - dead units x 3 kh) over the 2 chunks of an iteration with the dead units of the rule's closed form, the A-operand reads shrink with them, and the weight loads,
    LDS-DMA requests, barriers and counted waits are those of the kernel without a mask."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    asm = tmp_path / "w4e.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + CSRC, "-S", "--cuda-device-only",
                    os.path.join(CSRC, "i2v_conv16w4e.hip"), "-o", str(asm)], check=True, capture_output=True, timeout=900)
    text = asm.read_text()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_asm_waits as caw
    assert "conv_wino4_f16x3_kernel" not in text        # the pinned kernel is instantiated in its own unit only
    kernels = re.findall(r"^(_ZN3i2v2[42]conv_wino4e_f16(x3|)_kernelILi(\d)ELi(\d+)ELi512ELi(\d)EEEvNS_6W4ArgsE):[^\n]*\n(.*?)\.end_amdhsa_kernel", text,
                         flags=re.S | re.M)
    # <9,64> <6,64> <9,32> <6,32> on the 4 x 8 brick; the pair kernels also on the 2 x 16 brick of two-frame inputs
    assert sorted((k[1], k[2], k[3], k[4]) for k in kernels) == sorted(
        [(x3, nt, bn, tt) for x3 in ("x3", "") for nt, bn, tt in (("9", "64", "4"), ("6", "64", "4"), ("9", "32", "4"), ("6", "32", "4"),
                                                                   ("6", "64", "2"), ("6", "32", "2"))]), [k[0] for k in kernels]
    for name, x3, nt, bn, tt, whole in kernels:
        nt, tt = int(nt), int(tt)
        nterm = 3 if x3 else 2                              # MFMAs per (tap, row block)
        kt = nt // 3
        assert "scratch_" not in whole and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", whole), name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", whole).group(1)) <= 256, name
        loops = [mm.group(2) for mm in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n((?:(?!^\.LBB).)*?)s_cbranch_\w+ \1\n", whole, flags=re.S | re.M)
                 if "v_mfma" in mm.group(2)]
        seen = {4: [], 2: [], 1: []}
        for loop in loops:
            taps = 2 * nt                                   # two chunks per iteration
            mf = loop.count("v_mfma_f32_32x32x16_f16")
            # which pass: pass A requests 8 V pieces per chunk, pass B 4
            lds_dma = len(re.findall(r"buffer_load_dwordx4 [^\n]* lds", loop))
            assert lds_dma in (16, 8) and loop.count("global_load_lds_dwordx4") == 0, name
            wm = ((4, 2) if bn == "64" else (2, 1))[0 if lds_dma == 16 else 1]
            assert mf % (6 * nterm) == 0 and loop.count("ds_read_b128") * nterm == mf * 2, (name, mf)   # two operand reads per (tap, row block)
            dead = (taps * nterm * wm - mf) // (6 * nterm)  # dead units: 3 kh taps x nterm MFMAs x 2 chunks each
            assert taps * nterm * wm - mf == 6 * nterm * dead, (name, mf)
            seen[wm].append(dead)
            assert len(re.findall(r"global_load_dwordx4", loop)) == taps * 2, name
            assert loop.count("s_barrier") == 2, name
            assert caw.check_loop(loop) == [], name
            b_wait, bar_wait = max(waits_of(loop)), min(waits_of(loop))
            assert len(waits_of(loop)) == taps + 2, name                                     # one per tap + one per chunk barrier
            for w in (b_wait, bar_wait):
                mutated = re.sub(r"s_waitcnt vmcnt\(%d\)" % w, "s_waitcnt vmcnt(%d)" % (w + 1), loop)
                assert caw.check_loop(mutated) != [], (name, w)
        wma, wmb = (4, 2) if bn == "64" else (2, 1)
        assert sorted(seen[wma]) == _variants(kt, wma, tt) and sorted(seen[wmb]) == _variants(kt, wmb, tt), (name, seen)
        assert len(loops) == len(_variants(kt, wma, tt)) + len(_variants(kt, wmb, tt)), (name, len(loops))
    assert caw.check_loop_entries(text, "conv_wino4e_f16") == []
    assert caw.check_scalar_operands(text, "conv_wino4e_f16") == []


def test_libraries_carry_the_edge_kernel_and_only_the_measurement_build_its_switch():
    """Both builds carry conv_wino4e_f16x3_kernel next to the kernels it leaves every other case to; I2V_W4_TSKIP (the A/B and bit
    reference path) exists in the measurement build only."""
    lib, mlib = os.path.join(PKG, "lib", "libi2v_hip.so"), os.path.join(PKG, "lib", "libi2v_hip_measure.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    blob = open(lib, "rb").read()
    for nt, bn, tt in ((9, 64, 4), (6, 64, 4), (9, 32, 4), (6, 32, 4), (6, 64, 2), (6, 32, 2)):
        assert b"conv_wino4e_f16x3_kernelILi%dELi%dELi512ELi%dE" % (nt, bn, tt) in blob
        assert b"conv_wino4e_f16_kernelILi%dELi%dELi512ELi%dE" % (nt, bn, tt) in blob
    assert b"conv_wino4_f16x3_kernelILi9ELi64ELi512E" in blob and b"I2V_W4_TSKIP" not in blob
    if os.path.exists(mlib):
        assert b"I2V_W4_TSKIP" in open(mlib, "rb").read()
