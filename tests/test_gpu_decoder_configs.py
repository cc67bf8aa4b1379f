"""The decoder at ragged channel counts and every up-sampling plan, layer by layer, against a float64 oracle.

Every decoder test elsewhere runs channel_factor 8, 32 or 64 (8 * 2^k channels per layer) and the plans (2, 1) / (2, 2).  Here:

  config     nf  upsample_s upsample_t  g_3 / g_4 maps                   reaches
  nf24_p11   24  (1, 1)     (1, 1)      8x32x32, 8x32x32                 Cout 48 / 24 padded; SPADE 12 groups; F(4,3) 192 -> 96 (3 tiles)
  nf40_bair  40  (2, 1)     (2, 1)      16x64x64, 16x64x64               Cout 80 -> pad 128; 320 -> 160 (5 tiles); SPADE 10 groups
  nf48_p22   48  (2, 2)     (1, 1)      8x64x64, 8x128x128               Cout 96 -> pad 128 on the big maps
  nf8_s4     8   (4, 1)     (1, 2)      8x128x128, 16x128x128            x4 spatial; pair weights (tdup) at g_4
  nf16_t4    16  (1, 4)     (4, 1)      32x32x32, 32x128x128             x4 temporal, residual factor 4
  nf16_s4    16  (4, 1)     (1, 1)      8x128x128, 8x128x128             x4 spatial residual on F(4,3) (g_3: 64 -> 32)

each in seven kernel modes (MODES; the env switches are read when a handle is created).  Per (config, mode): the full final frames,
and through the debug tap (i2v_dec_debug_tap) at every block: SPADE's (1 + gamma | beta) (tap 0), conv_0's output with its bias
(tap 2 -- ADAIN's instance norm right behind it removes any per-channel affine error from everything downstream), the learned
shortcut (tap 4) and the block output (tap 5; g_4's is lrelu(.), fused into conv_1's epilogue).  Taps 1 and 3 (the conv operands)
hold fp32 maps only in exact-fp32 mode on layers that run the direct kernel; elsewhere the buffer holds the split-fp16 / Winograd
operand or is not written, so they are checked there only.  Every tap buffer is filled with NaN first: a tap that is not written
fails.  With a tap set the handle runs the learned shortcut inline (no side stream), so tap 4 is written in every mode.

Four metrics per tensor against the fp64 oracle (oracle.decoder_ref.generator_taps): global rel-L2, worst per-channel rel-L2,
worst per-frame rel-L2 and max|err| / rms(ref).  Gates per kernel family (split-fp16 / exact fp32) and metric: 4x the largest
value measured over the matrix on an MI355X, never above the 1e-4 contract.

Measured on an MI355X (largest over all configs, modes of the family, blocks and taps) and the gates (4x, capped at 1e-4):

  family                       global    channel   frame     max/rms
  split-fp16 (mma 1, auto)     3.02e-6   5.03e-6   3.71e-6   2.73e-5     gates 1.2e-5  2.0e-5  1.5e-5  1e-4 (contract)
  exact fp32 (mma 0)           6.62e-6   8.23e-6   7.65e-6   6.75e-5     gates 2.7e-5  3.3e-5  3.1e-5  1e-4 (contract)
  stand-alone GeneratorBlock   2.19e-6   2.46e-6   2.45e-6   2.80e-5     gates 8.8e-6  9.8e-6  9.8e-6  1e-4 (contract)
  CPU fp32 vs fp64 (noise)     1.85e-6   5.96e-6   2.24e-6   2.73e-5

The exact-fp32 modes are also held, tensor by tensor, to a multiple of the CPU's own fp32 distance to fp64 for the same tensor
(NOISE_FACTOR).  Measured, the GPU's exact-fp32 result is within 10x of that noise for every tensor but one: g_0.conv_0 at nf = 48
(768 -> 768 at 2x8x8) reaches 9.6x / 12.4x / 9.5x / 28x.  That layer reduces K = 27 * 768 products per output in fp32 MFMA chains,
while the CPU's blocked reduction is unusually accurate there (3.8e-7).  So the family gates sit at 14x (global), 5.5x, 14x and
3.7x of the largest CPU noise of any tensor: they are 4x the GPU's worst tensor, not 4x the CPU's.

A coverage ledger (i2v_dec_get_layer_profile's kernel code per layer, over the whole matrix) asserts that the sweep really ran the
kernels at the shapes it exists for."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i2v_synth as synth

pytestmark = pytest.mark.gpu
CONTRACT = 1e-4
B, ZD = 2, 64

CONFIGS = {   # name: (nf, upsample_s, upsample_t, start frame (h, w), weight seed)
    "nf24_p11": (24, (1, 1), (1, 1), (64, 64), 124),
    "nf40_bair": (40, (2, 1), (2, 1), (48, 80), 140),
    "nf48_p22": (48, (2, 2), (1, 1), (64, 64), 148),
    "nf8_s4": (8, (4, 1), (1, 2), (48, 80), 108),
    "nf16_t4": (16, (1, 4), (4, 1), (64, 64), 116),
    "nf16_s4": (16, (4, 1), (1, 1), (48, 80), 216),
}
MODES = {     # name: (mma, env)
    "mma1": (1, {}),
    "mma1_w4all": (1, {"I2V_DEC_WINO4": "2"}),
    "mma1_f23": (1, {"I2V_DEC_WINO4": "0"}),
    "mma1_direct": (1, {"I2V_DEC_WINO": "0"}),
    "mma0": (0, {}),
    "mma0_direct": (0, {"I2V_DEC_WINO32": "0"}),
    "auto": (2, {}),
}
METRICS = ("global", "channel", "frame", "max")
# 4x the largest value measured on an MI355X (module docstring), capped at the contract
GATES = {
    "f16": dict(global_=1.2e-5, channel=2.0e-5, frame=1.5e-5, max=CONTRACT),
    "f32": dict(global_=2.7e-5, channel=3.3e-5, frame=3.1e-5, max=CONTRACT),
    "gblock": dict(global_=8.8e-6, channel=9.8e-6, frame=9.8e-6, max=CONTRACT),
}
# exact-fp32 modes, per tensor: at most this many times the CPU's own fp32 distance to fp64 of the same tensor (4x the largest
# ratio measured: 9.6 / 12.4 / 9.5 / 28.5)
NOISE_FACTOR = dict(global_=40.0, channel=50.0, frame=40.0, max=120.0)
CIN = (16, 16, 16, 8, 4, 2)
COUT = (16, 16, 8, 4, 2, 1)
# i2v_dec_get_layer_profile kernel codes
K_F32, K_F16_DIRECT, K_F23, K_F43, K_F43_GEN, K_F32_WINO = range(6)


def _gate(family, metric):
    return GATES[family]["global_" if metric == "global" else metric]


def family(mode):
    return "f32" if MODES[mode][0] == 0 else "f16"


def metrics(out, ref, ch_dim, frame_dims):
    """The four error metrics of ``out`` against the float64 reference ``ref`` (same shape, same device), in float64:
    global rel-L2, worst per-channel rel-L2 (channel axis ``ch_dim``), worst per-frame rel-L2 (a frame = one index of the axes
    ``frame_dims``) and max|err| / rms(ref)."""
    assert out.shape == ref.shape, (tuple(out.shape), tuple(ref.shape))
    e2 = (out.double() - ref) ** 2
    r2 = ref * ref
    nd = ref.dim()
    ch_dim %= nd
    frame_dims = tuple(d % nd for d in frame_dims)
    other_c = tuple(d for d in range(nd) if d != ch_dim)
    other_f = tuple(d for d in range(nd) if d not in frame_dims)

    def worst(dims):
        return float(((e2.sum(dims) / r2.sum(dims).clamp_min(1e-300)).sqrt()).max())
    return {"global": float((e2.sum() / r2.sum()).sqrt()), "channel": worst(other_c), "frame": worst(other_f),
            "max": float(e2.max().sqrt() / r2.mean().sqrt())}


def tap_layout(which):
    """(channel axis, frame axes) of a tap: 0 is [B, H, W, 2C] (a frame = a sample), the others [B, T, H, W, C]."""
    return (3, (0,)) if which == 0 else (4, (0, 1))


def ragged(c):
    """Not 8 * 2^k channels."""
    q = c // 8
    return c % 8 != 0 or (q & (q - 1)) != 0


def layer_plan(nf, ups, upt):
    """Per 3x3x3 conv layer (2 * block + i): (block, i, cin, cout, ut, us) of the level the block runs at."""
    rows = []
    for k in range(6):
        ut, us = (1, 1) if k == 0 else (2, 2) if k <= 3 else (upt[k - 4], ups[k - 4])
        n_in, n_out = CIN[k] * nf, COUT[k] * nf
        n_mid = min(n_in, n_out)
        rows.append((k, 0, n_in, n_mid, ut, us))
        rows.append((k, 1, n_mid, n_out, ut, us))
    return rows


def _inputs(name):
    nf, ups, upt, (ih, iw), seed = CONFIGS[name]
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.decoder_state_dict(seed=seed, channel_factor=nf).items()}
    img = 2 * torch.rand(B, 3, ih, iw, generator=torch.Generator().manual_seed(seed)) - 1
    z = torch.randn(B, ZD, generator=torch.Generator().manual_seed(seed + 1))
    return sd, img, z


def make_case(name):
    """The fp64 oracle of one configuration (taps and frames, on the GPU in float64) and the CPU fp32 noise of every tensor."""
    from oracle import decoder_ref
    nf, ups, upt, _, _ = CONFIGS[name]
    sd, img, z = _inputs(name)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    taps64, frames64 = decoder_ref.generator_taps({k: v.double() for k, v in sd.items()}, img.double(), z.double(), ups, upt)
    taps32, frames32 = decoder_ref.generator_taps(decoder_ref.fold_spectral_norm(sd), img, z, ups, upt)
    refs, noise = {}, {}
    for k in range(6):
        for which in sorted(taps64[k]):
            r64, r32 = taps64[k][which], taps32[k][which]
            if (k, which) == (5, 5):   # g_4's output tap holds lrelu(.): fused into conv_1's epilogue (decoder.py:117)
                r64, r32 = F.leaky_relu(r64, 0.2), F.leaky_relu(r32, 0.2)
            key = f"b{k}.t{which}"
            refs[key] = r64.cuda()
            noise[key] = metrics(r32.cuda(), refs[key], *tap_layout(which))
    refs["frames"] = frames64.cuda()
    noise["frames"] = metrics(frames32.cuda(), refs["frames"], 2, (0, 1))
    sat = float((frames64.abs() > 0.99).double().mean())
    return {"name": name, "nf": nf, "ups": ups, "upt": upt, "sd": sd, "img": img.cuda(), "z": z.cuda(), "refs": refs,
            "noise": noise, "saturated": sat}


def _handle(case_or_name, mma):
    import i2v_native
    name = case_or_name if isinstance(case_or_name, str) else case_or_name["name"]
    nf, ups, upt, _, _ = CONFIGS[name]
    h = i2v_native.NativeDecoder(nf, ZD, list(ups), list(upt), True, mma=mma)
    h.load(case_or_name["sd"] if isinstance(case_or_name, dict) else _inputs(name)[0])
    return h


def layer_kernels(h, img, z):
    """Kernel code of every 3x3x3 conv layer in one profiled forward (no tap set: the product path)."""
    import i2v_native
    h.set_profile(True)
    h.forward(img, z)
    torch.cuda.synchronize()
    rows = h.get_layer_profile()
    h.set_profile(False)
    names = i2v_native.NativeDecoder.KERNEL_NAMES
    codes = {r["layer"]: names.index(r["kernel"]) for r in rows}
    assert len(codes) == 12, rows
    return [codes[n] for n in i2v_native.NativeDecoder.LAYER_NAMES]


def run_mode(case, mode):
    """Runs one configuration in one mode (the mode's env must be set by the caller).  Returns (frames, layer kernel codes,
    {tensor: metrics}, status word)."""
    mma = MODES[mode][0]
    h = _handle(case, mma)
    img, z = case["img"], case["z"]
    codes = layer_kernels(h, img, z)
    frames = h.forward(img, z)
    res = {"frames": metrics(frames, case["refs"]["frames"], 2, (0, 1))}
    for k in range(6):
        whichs = [0, 2, 5] + ([4] if f"b{k}.t4" in case["refs"] else [])
        if mma == 0:
            whichs += [w for w, layer in ((1, 2 * k), (3, 2 * k + 1)) if codes[layer] == K_F32]
        for which in sorted(whichs):
            key = f"b{k}.t{which}"
            ref = case["refs"][key]
            dst = torch.full((ref.numel(),), float("nan"), dtype=torch.float32, device=ref.device)
            h.debug_tap(k, which, dst)
            h.forward(img, z)
            h.debug_tap(0, 0, None)
            torch.cuda.synchronize()
            n_nan = int(torch.isnan(dst).sum())
            assert n_nan == 0, f"{case['name']} {mode} {key}: {n_nan} of {dst.numel()} tap values not written"
            res[key] = metrics(dst.view(ref.shape), ref, *tap_layout(which))
    status = h.status()
    return frames, codes, res, status


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    torch.set_grad_enabled(False)


@pytest.fixture(scope="module", params=list(CONFIGS))
def case(request):
    c = make_case(request.param)
    yield c
    c["refs"].clear()
    torch.cuda.empty_cache()


def _set_env(monkeypatch, env):
    for k in ("I2V_DEC_WINO", "I2V_DEC_WINO4", "I2V_DEC_WINO32", "I2V_DEC_OVERLAP", "I2V_DEC_GEN", "I2V_DEC_MMA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("mode", list(MODES))
def test_decoder_config_layer_by_layer_vs_fp64(case, mode, monkeypatch):
    """One configuration in one kernel mode: full frames and every block's taps within the measured gates (and the contract);
    the frames are not saturated (tanh would hide errors); the range guard stays clear; mma = auto gives mma = 1's bits."""
    assert case["saturated"] < 0.05, case["saturated"]
    _set_env(monkeypatch, MODES[mode][1])
    frames, codes, res, status = run_mode(case, mode)
    assert status == 0, (case["name"], mode, status)
    fam = family(mode)
    bad = []
    for key, m in res.items():
        for metric in METRICS:
            gate = min(_gate(fam, metric), CONTRACT)
            if not m[metric] <= gate:
                bad.append(f"{key} {metric} {m[metric]:.3e} > {gate:.1e}")
            if fam == "f32":
                cap = NOISE_FACTOR["global_" if metric == "global" else metric] * case["noise"][key][metric] + 1e-8
                if not m[metric] <= cap:
                    bad.append(f"{key} {metric} {m[metric]:.3e} > {cap:.1e} (CPU fp32 noise x factor)")
    assert not bad, f"{case['name']} {mode} kernels {codes}: " + "; ".join(bad)
    if mode == "auto":
        h1 = _handle(case, 1)
        assert torch.equal(frames, h1.forward(case["img"], case["z"])), case["name"]
        h2 = _handle(case, 2)
        h2.forward(case["img"], case["z"])
        fb = h2.fallback_layers()
        assert fb["layers"] == [] and not fb["whole_handle"] and fb["reruns"] == 0, fb


def test_kernel_coverage_ledger(monkeypatch):
    """Over the whole matrix the sweep ran each kernel family at the shapes it exists for -- so that no configuration can quietly
    fall back to one kernel everywhere."""
    seen = []
    for name, (nf, ups, upt, _, _) in CONFIGS.items():
        sd, img, z = _inputs(name)
        img, z = img.cuda(), z.cuda()
        plan = layer_plan(nf, ups, upt)
        for mode, (mma, env) in MODES.items():
            _set_env(monkeypatch, env)
            h = _handle({"name": name, "sd": sd}, mma)
            for code, row in zip(layer_kernels(h, img, z), plan):
                seen.append((name, mode, code) + row)
            del h
    f16 = (K_F16_DIRECT, K_F23, K_F43, K_F43_GEN)

    def any_(pred):
        return any(pred(*s) for s in seen)
    # (name, mode, code, block, conv, cin, cout, ut, us)
    assert any_(lambda n, m, c, k, i, ci, co, ut, us: c == K_F16_DIRECT and co % 32 != 0), "direct split-fp16 at Cout % 32 != 0"
    assert any_(lambda n, m, c, k, i, ci, co, ut, us: c in (K_F43, K_F43_GEN) and co % 64 == 32 and co > 32), "F(4,3), odd 32-tiles"
    assert any_(lambda n, m, c, k, i, ci, co, ut, us: m == "mma1_f23" and c == K_F23 and ragged(co)), "F(2,3) at a ragged width"
    assert any_(lambda n, m, c, k, i, ci, co, ut, us: c == K_F32_WINO and ragged(co)), "exact-fp32 Winograd at a ragged width"
    assert any_(lambda n, m, c, k, i, ci, co, ut, us: c in f16 and k == 5 and i == 0 and ut == 2), "tdup at g_4"
    for axis in (0, 1):   # x4 residual in time (rt) and in space (rs)
        assert any_(lambda n, m, c, k, i, ci, co, *ts: c in (K_F43, K_F43_GEN) and i == 1 and ts[axis] == 4), ("x4 residual, F(4,3)", axis)
        assert any_(lambda n, m, c, k, i, ci, co, *ts: c == K_F32_WINO and i == 1 and ts[axis] == 4), ("x4 residual, fp32 Winograd", axis)


# ------------------------------------------------------------------------------------------- stand-alone GeneratorBlock
GB_PAIRS = ((24, 24), (40, 40), (200, 200), (48, 24), (96, 48), (160, 80), (1024, 1024))
GB_SHAPES = ((2, 1, 8, 8), (1, 2, 16, 16), (1, 4, 16, 32))   # (B, T, H, W)


def _block_sd(n_in, n_out, seed):
    sd = {}
    synth._block(sd, np.random.default_rng(seed), "blk", n_in, n_out, ZD, True, ())
    return {k[4:]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.mark.parametrize("wino4", [None, "2"])
@pytest.mark.parametrize("pair", GB_PAIRS, ids=[f"{a}-{b}" for a, b in GB_PAIRS])
def test_generator_block_ragged_widths_vs_fp64(pair, wino4, monkeypatch):
    """Stand-alone GeneratorBlock at ragged widths (200: 10 SPADE groups; 1024: the top of the statistics / coef staging) on three
    geometries, default kernels and F(4,3) wherever its tiling allows, against the fp64 block oracle."""
    from oracle import decoder_ref
    from stage1_VAE.modules import decoder as dec
    _set_env(monkeypatch, {"I2V_DEC_WINO4": wino4} if wino4 else {})
    n_in, n_out = pair
    sd = _block_sd(n_in, n_out, seed=n_in * 7 + n_out)
    sd64 = {"blk." + k: v.double() for k, v in sd.items()}
    blk = dec.GeneratorBlock(n_in, n_out, True, ZD)
    blk.load_state_dict(sd)
    blk = blk.cuda().eval()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = torch.Generator().manual_seed(n_in + n_out)
    bad = []
    for (b, t, hh, ww) in GB_SHAPES:
        x = torch.randn(b, n_in, t, hh, ww, generator=g)
        img = 2 * torch.rand(b, 3, 24, 40, generator=g) - 1
        z = torch.randn(b, ZD, generator=g)
        ref = decoder_ref.generator_block(sd64, "blk", x.double(), z.double(), img.double(), faithful=False)
        out = blk(x.cuda(), z.cuda(), img.cuda())
        m = metrics(out, ref.cuda(), 1, (0, 2))
        for metric in METRICS:
            gate = min(_gate("gblock", metric), CONTRACT)
            if not m[metric] <= gate:
                bad.append(f"{(b, t, hh, ww)} {metric} {m[metric]:.3e} > {gate:.1e}")
    assert not bad, f"{pair} wino4={wino4}: " + "; ".join(bad)
    assert blk.native().status() == 0


def test_learned_shortcut_without_16_groups_is_refused():
    """A learned shortcut's Norm3D is GroupNorm(16, n_in): the C ABI refuses n_in % 16 != 0 (it used to run, and the shortcut read
    group totals that were never written for channels 16..23 of a 24-channel input); so does a stand-alone Norm3D handle."""
    import i2v_native
    lib = i2v_native.lib()
    for mma in (0, 1):
        h = ctypes.c_void_p()
        assert lib.i2v_gblock_create(24, 8, ZD, 1, mma, ctypes.byref(h)) == -1   # I2V_E_INVALID
        assert lib.i2v_gblock_create(40, 24, ZD, 1, mma, ctypes.byref(h)) == -1
        assert lib.i2v_gblock_create(48, 24, ZD, 1, mma, ctypes.byref(h)) == 0
        lib.i2v_gblock_destroy(h)
    with pytest.raises(i2v_native.I2VError, match=r"failed \(-1\)"):
        i2v_native.NativeGBlock(24, 8, ZD)
    n3 = i2v_native.NativeNorm("norm3d", 24, 0)
    n3.load({"bn.weight": torch.ones(24), "bn.bias": torch.zeros(24)})
    with pytest.raises(i2v_native.I2VError, match=r"failed \(-1\)"):
        n3.forward(torch.randn(1, 24, 2, 8, 8, device="cuda"), None)


def test_mma_auto_runs_standalone_blocks_as_split_fp16(monkeypatch):
    """I2V_DEC_MMA=auto (the setting the README advertises) on the stand-alone modules: a block has no re-run loop, so auto runs them
    in split-fp16 mode -- the bits of mma = 1."""
    from stage1_VAE.modules import decoder as dec, normalization_layer as nl
    sd = _block_sd(48, 24, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 48, 4, 16, 16, generator=g).cuda()
    img = (2 * torch.rand(1, 3, 24, 40, generator=g) - 1).cuda()
    z = torch.randn(1, ZD, generator=g).cuda()
    outs = {}
    for mma in ("1", "auto"):
        monkeypatch.setenv("I2V_DEC_MMA", mma)
        blk = dec.GeneratorBlock(48, 24, True, ZD)
        blk.load_state_dict(sd)
        sp = nl.Spade(48)
        sp.load_state_dict({k[len("norm_0."):]: v for k, v in sd.items() if k.startswith("norm_0.")})
        outs[mma] = (blk.cuda()(x, z, img), sp.cuda()(x, img))
    assert torch.equal(outs["1"][0], outs["auto"][0]) and torch.equal(outs["1"][1], outs["auto"][1])
