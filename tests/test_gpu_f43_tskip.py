"""The F(4,3) kernel that skips the temporal taps reading only zero padding (csrc/i2v_conv16w4e.hip) against the full tap loops of
conv_wino4_f16x3_kernel: the products it leaves out are exact zeros and the order of the remaining accumulation is untouched, so its
outputs must be the same BITS.  The full loops stay reachable in the measurement build only (I2V_W4_TSKIP=0), so every comparison runs
in tests/f43_tskip_worker.py, a process of its own with I2V_LIB_PATH on lib/libi2v_hip_measure.so.

Shapes: the smallest at which each edge class can go wrong -- 16 x 16 maps (one h-brick or two, one w-brick), T = 4 (one brick, both
ends), 8 (front and back in different bricks), 16 (interior bricks too); T = 2 is run as well, but a 3x3x3 halo brick of 2 x 16 rows does
not fit the kernel's V buffers (wino4_tiling), so those blocks never reach an F(4,3) kernel -- the worker asserts exactly that.  The
2 x 16 brick exists for the pair kernels (g_1.conv_0 of every decoder: T_out = 4).  Cin, Cout in {32, 64}, B in {1, 3}, 32- and
64-channel workgroups (I2V_W4_BN=64: at these sizes the plan would narrow every 64-channel layer) and the 512-thread geometry for the
layers with 32 output channels (I2V_W4_NTH=512: by default they run as 256-thread workgroups, whose row blocks span two frames)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(part):
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    if not os.path.exists(i2v_native.MEASURE_LIB_PATH):
        i2v_native.build_measure()                               # (normally built by __graft_entry__.build())
    env = dict(os.environ, I2V_LIB_PATH=os.path.join("image2video-synthesis-using-cinns_amd", "lib", "libi2v_hip_measure.so"))
    for k in ("I2V_W4_TSKIP", "I2V_W4_BN", "I2V_W4_NTH", "I2V_W4_TRACE", "I2V_DEC_WINO4"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "f43_tskip_worker.py"), part], env=env, capture_output=True, text=True,
                       timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"F43TSKIP {part}: {res}")
    return res


def test_blocks_keep_the_bits_and_the_fp64_gates():
    """Stand-alone GeneratorBlocks through i2v_gblock_forward (3x3x3 conv_0 with fused statistics feeding ADAIN, conv_1 with the residual
    epilogue, identity and learned shortcut): 64 -> 64, 32 -> 32, 32 -> 64 and 64 -> 32 convs x T in {2, 4, 8, 16} x B in {1, 3} x the plan's own /
    64-channel / all-512-thread workgroups.  Per case: torch.equal between I2V_W4_TSKIP=0 and the default, the edge form really ran (launch trace), and the block
    output within the stand-alone block's float64 gates (tests/test_gpu_decoder_configs.py)."""
    res = _worker("blocks")
    assert res["cases"] == 3 * 4 * 2 * 3 and res["bad"] == [], res


def test_decoders_keep_the_bits_and_count_what_they_issue():
    """Decoder handles (nf = 8, 16; B = 1, 3; split-fp16 and the one-term fp16 form): the temporal-duplication pair kernels at T_out = 4 (2 x 16 brick), 8 and 16 with both
    parities, residuals through the x2 / x2 up-sampling map, fused statistics, the lrelu epilogue.  Frames bit-identical, and every
    F(4,3) layer's issued-MFMA FLOPs in the layer profile shrink by exactly the closed-form dead share of its launch."""
    res = _worker("decoders")
    assert res["cases"] == 8 and res["bad"] == [] and len(res["shares"]) >= 8 and min(res["shares"].values()) < 0.8, res


def test_whole_decoders_keep_the_bits_on_the_goldens():
    """dec_nf64_bair and dec_nf32_128, 3 samples as in test_f43_structure_switches_keep_the_bits, split-fp16 and mma = "fp16": the shipped
    kernel choice, frames bit-identical with and without the skip, the golden sample held."""
    res = _worker("goldens")
    assert res["cases"] == 4 and res["bad"] == [], res


def test_units_on_the_edge_kernel_hold_the_fp64_bounds():
    """Every unit of nf40_bair with F(4,3) on every layer it tiles -- convs (3x3x3 and pairs, with residual and lrelu epilogues) and the
    fused statistics on the edge kernel -- within the element-wise bounds tests/test_gpu_dec_units.py derives against float64."""
    res = _worker("units")
    assert res["bad"] == [] and max(v for k, v in res["worst"].items() if k.startswith(("conv_f43", "stats"))) <= 1.0, res
