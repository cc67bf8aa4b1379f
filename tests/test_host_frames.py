"""Device-side output stage (csrc/i2v_frames.hip), the parts that need no GPU: the C ABI is declared, the Python wrappers check their
arguments before any device is touched, the CPU paths of the new ``utils.auxiliaries`` functions give the bytes of the existing host
code, and the compiled kernels have the structure the design relies on (no scratch, 16-byte loads, two roundings in the de-normalisation)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, REPO


def test_header_declares_the_frames_abi():
    import i2v_native
    hdr = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    for name in ("i2v_frames_peak", "i2v_frames_to_u8"):
        assert re.search(r"\b%s\(" % name, hdr) and name in i2v_native.SYMBOLS, name
    assert "i2v_frames_cfg" in hdr and "utils/auxiliaries.py:15-22" in hdr and "53-55" in hdr
    # the ctypes mirror has the header's fields in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} i2v_frames_cfg;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"int(?:32|64)_t ([^;]+);", body) for n in decl.split(",")]
    assert fields == [f[0] for f in i2v_native.FramesCfg._fields_]


def test_frames_arguments_are_checked_before_any_device():
    import i2v_native
    from i2v_pipeline import FrameSink
    E = i2v_native.I2VError
    good = torch.zeros(2, 4, 3, 8, 8)
    assert i2v_native.frames_geometry(good) == (2, 1, 4, 8, 8, 4 * 3 * 8 * 8)
    assert i2v_native.frames_geometry(torch.zeros(2, 32, 3, 8, 8)[:, :16]) == (2, 1, 16, 8, 8, 32 * 3 * 8 * 8)
    assert i2v_native.frames_geometry(torch.zeros(6, 4, 3, 8, 8).view(2, 3, 4, 3, 8, 8)) == (6, 3, 4, 8, 8, 4 * 3 * 8 * 8)
    assert i2v_native.frames_geometry(torch.zeros(6, 32, 3, 8, 8).view(2, 3, 32, 3, 8, 8)[:, :, :16]) == (6, 3, 16, 8, 8, 32 * 3 * 8 * 8)
    for bad in (torch.zeros(2, 4, 1, 8, 8), torch.zeros(4, 3, 8, 8), torch.zeros(2, 4, 3, 8, 8, dtype=torch.float64),
                torch.zeros(2, 4, 3, 8, 16)[..., ::2], torch.zeros(0, 4, 3, 8, 8), torch.zeros(2, 3, 4, 3, 8, 8)[:, ::2]):
        with pytest.raises(E, match="frames"):
            i2v_native.frames_peak(bad)
        with pytest.raises(E, match="frames"):
            i2v_native.frames_to_u8(bad, mode="unit")
    with pytest.raises(E, match="accumulate"):
        i2v_native.frames_peak(good, accumulate=True)
    with pytest.raises(E, match="one element"):
        i2v_native.frames_peak(good, out=torch.zeros(2))
    with pytest.raises(E, match="mode"):
        i2v_native.frames_to_u8(good, mode="gif")
    with pytest.raises(E, match="layout"):
        i2v_native.frames_to_u8(good, mode="unit", layout="planar")
    with pytest.raises(E, match="takes no peak"):
        i2v_native.frames_to_u8(good, peak=torch.zeros(1), mode="unit")
    with pytest.raises(E, match="col0"):
        i2v_native.frames_to_u8(good, mode="unit", col0=-1)
    with pytest.raises(E, match="does not fit"):
        i2v_native.frames_to_u8(good, mode="unit", out=torch.zeros(4, 8, 16, 3, dtype=torch.uint8), col0=8)
    with pytest.raises(E, match="out must be"):
        i2v_native.frames_to_u8(good, mode="unit", out=torch.zeros(4, 8, 16, 3))
    with pytest.raises(E, match="out must be"):
        i2v_native.frames_to_u8(good, mode="unit", layout="clips", out=torch.zeros(2, 4, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(E, match="no placement"):
        i2v_native.frames_to_u8(good, mode="unit", layout="clips", col0=8)
    # well-formed CPU tensors: refused for the device they live on, still without touching one
    with pytest.raises(E, match="HIP device"):
        i2v_native.frames_peak(good)
    with pytest.raises(E, match="HIP device"):
        i2v_native.frames_to_u8(good, mode="unit")
    with pytest.raises(ValueError, match="mode"):
        FrameSink(mode="gif")
    with pytest.raises(ValueError, match="budget_bytes"):
        FrameSink(budget_bytes=-1)


def test_model_u8_methods_exist():
    from get_model import Model
    assert callable(Model.synthesize_u8) and callable(Model.sample_u8)


def _frames(shape, gain, seed):
    return torch.tanh(gain * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def _restate_strip_f32(x):
    """The device arithmetic written out in float32 numpy: peak from the RAW maximum, multiply and add rounded separately, the scale
    float32(255.0 / float(d_peak)), truncating cast."""
    a = x.numpy()
    half = np.float32(0.5)
    d = np.clip(a * half + half, np.float32(0), np.float32(1))
    dp = np.clip(np.float32(a.max()) * half + half, np.float32(0), np.float32(1))
    s = np.float32(255.0 / float(dp))
    n, t, c, h, w = a.shape
    return (d * s).astype(np.uint8).transpose(1, 3, 0, 4, 2).reshape(t, h, n * w, c)


@pytest.mark.parametrize("gain", [0.3, 1.0, 3.0, 30.0])
def test_cpu_paths_give_the_host_bytes(gain):
    from utils import auxiliaries as aux
    for seed, shape in enumerate([(3, 4, 3, 8, 12), (1, 16, 3, 16, 16), (5, 2, 3, 7, 9)]):
        x = _frames(shape, gain, seed)
        ref = aux.convert_seq2gif(x).astype(np.uint8)
        out = aux.convert_seq2gif_u8(x)
        assert out.dtype == np.uint8 and np.array_equal(out, ref)
        assert np.array_equal(_restate_strip_f32(x), ref)       # what the kernel computes, restated on the host
        clips = aux.to_uint8_clips(x)
        expr = torch.clamp(x * 0.5 + 0.5, 0.0, 1.0).mul(255).add(0.5).clamp(0, 255).permute(0, 1, 3, 4, 2).to(torch.uint8)
        assert clips.dtype == torch.uint8 and clips.is_contiguous() and torch.equal(clips, expr)
    g = _frames((2, 3, 4, 3, 8, 12), gain, 11)
    out = aux.convert_grid2gif_u8(g)
    assert out.dtype == np.uint8 and np.array_equal(out, aux.convert_grid2gif(g).astype(np.uint8))
    assert np.array_equal(aux.convert_grid2gif_u8(g[:, :1]), aux.convert_seq2gif_u8(g[:, 0]))
    assert torch.equal(aux.to_uint8_clips(g), aux.to_uint8_clips(g.reshape(6, 4, 3, 8, 12)).view(2, 3, 4, 8, 12, 3))
    with pytest.raises(ValueError):
        aux.convert_seq2gif_u8(g)
    with pytest.raises(ValueError):
        aux.convert_grid2gif_u8(g[0])


def _asm(tmp_path, name):
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / (name + ".s")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(PKG, "csrc"), "-S",
                    "--cuda-device-only", os.path.join(PKG, "csrc", name + ".hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    return out.read_text()


def test_frames_kernels_are_compiled(tmp_path):
    """Both kernels present in every instantiation, zero scratch; the vector converters load 16 bytes per lane and plane and store the
    12 bytes of four pixels in one instruction; no fused multiply-add between the loads and the store (the de-normalisation's multiply
    and add round separately, as torch's do -- the only FMAs of the kernel are the scale's division, ahead of the loop); the peak
    kernel ends in one integer atomic per workgroup, not a compare-and-swap loop."""
    text = _asm(tmp_path, "i2v_frames")
    bodies = dict(re.findall(r"^(\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M))
    peak = {n: b for n, b in bodies.items() if "frames_peak_kernel" in n}
    conv = {n: b for n, b in bodies.items() if "frames_to_u8_kernel" in n}
    assert len(peak) == 2 and len(conv) == 4, sorted(bodies)
    for name, body in {**peak, **conv}.items():
        assert "scratch_" not in body and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
    vec_peak = [b for n, b in peak.items() if "ILb1E" in n]
    assert len(vec_peak) == 1 and "global_load_dwordx4" in vec_peak[0]
    for body in peak.values():
        assert "global_atomic_smax" in body and "global_atomic_umin" in body and "cmpswap" not in body
    for pk in ("ILb1ELb1E", "ILb0ELb1E"):                          # PEAK and UNIT mode, vector form
        (body,) = [b for n, b in conv.items() if pk in n]
        code = body.split("s_endpgm")[0]
        loops = [m.group(2) for m in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n((?:(?!^\.LBB).)*?)s_cbranch_\w+ \1\n", code, flags=re.S | re.M)
                 if "global_load_dwordx4" in m.group(2)]
        assert len(loops) == 1, pk
        main = loops[0]
        assert main.count("global_load_dwordx4") == 3 and main.count("global_store_dwordx3") == 1 and "global_store_byte" not in main, pk
        between = main[main.index("global_load_dwordx4"):main.index("global_store_dwordx3")]
        assert not re.search(r"\bv_(pk_)?fma|\bv_fmac|\bv_mad_f32|\bv_mac_f32", between), pk
        assert len(re.findall(r"\bv_(?:pk_)?mul_f32", between)) >= 12 // 2 and "v_add_f32" in between, pk
    for pk in ("ILb1ELb0E", "ILb0ELb0E"):                          # the scalar forms: any W >= 1
        (body,) = [b for n, b in conv.items() if pk in n]
        code = body.split("s_endpgm")[0]
        assert code.count("global_store_byte") == 3 and not re.search(r"\bv_mad_f32|\bv_mac_f32", code), pk
        loop = code[code.index("global_load_dword"):code.rindex("global_store_byte")]
        assert not re.search(r"\bv_(pk_)?fma|\bv_fmac", loop), pk
