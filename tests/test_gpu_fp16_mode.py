"""The opt-in half-precision decoder mode (mma = 3, "fp16"): the 3x3x3 block convs that run the F(4,3) kernel in mma = 1 run its
one-term form (csrc/i2v_conv16w4h.hip: fp16 operands, one MFMA per product, fp32 accumulation) on the one-term operand
(modulate_wino4_kernel<GB, true>); every other launch is the mma = 1 launch.

Pins, from tight to loose:
  * the conv: conv_0 of a temporal-duplication block and of a plain block recomputed in float64 from the TAPPED fp16 operand and the
    fp16 weights as the packer rounds them -- only the fp32 arithmetic may differ (summation order, the output transform);
  * the writer: the one-term operand equals the hi parts of the split operand (mma = 1), re-laid out, bit for bit;
  * the frames against the fp32 reference goldens and against mma = 1 (uint8 agreement), with bounds at ~2x the measured values
    (INTEGRATION.md §3 records them), under the ceilings 1e-2 (frames) and 3e-3 (any single conv, against mma = 0);
  * determinism (batch shards, repeat runs, graph replay), the range guard, and the stand-alone GeneratorBlock."""
import numpy as np
import pytest
import torch

import i2v_synth as synth
from conftest import load_golden, rel_l2
from dec_units_common import _v_onehot_channels, _v_split_hi

pytestmark = pytest.mark.gpu

K_F43, K_F43H = 3, 6                 # i2v_dec_get_layer_profile kernel codes: conv_wino4_f16x3, conv_wino4_f16
FRAME_CEIL, CONV_CEIL = 1e-2, 3e-3   # the contract's ceilings
# ~2x the values measured on an MI355X
#   frames vs the golden: 1.32e-3 (BAIR nf = 64), 1.06e-3 (128x128 nf = 32), 7.96e-4 (model nf = 8, T = 32)
#   worst conv output vs mma = 0 (g_4.conv_1, errors carried from the earlier convs included): 1.32e-3 / 1.23e-3
#   stand-alone GeneratorBlock vs mma = 1: 9.5e-4;  uint8 frames vs mma = 1: 100 % within +-1 level, max |delta| 1
FRAME_BOUND = {"dec_nf64_bair": 2.7e-3, "dec_nf32_128": 2.2e-3, "model_nf8": 1.6e-3}
CONV_BOUND = 2.7e-3
BLOCK_BOUND = 2e-3
U8_WITHIN1, U8_MAXDELTA = 0.999, 2   # uint8 agreement with mma = 1: share within +-1 level, largest |delta|


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    torch.set_grad_enabled(False)


def _gen(meta, mma):
    from stage1_VAE.modules.decoder import Generator
    gen = Generator({"channel_factor": meta["synth"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"],
                     "upsample_t": meta["upsample_t"], "spectral_norm": True, "mma": mma})
    gen.load_state_dict(T(synth.decoder_state_dict(**meta["synth"])))
    return gen.cuda().eval()


def _kernels(gen, img, z):
    import i2v_native
    h = gen.native()
    h.set_profile(True)
    gen(img, z)
    torch.cuda.synchronize()
    rows = h.get_layer_profile()
    h.set_profile(False)
    return {r["layer"]: r["kernel"] for r in rows}, rows


def _tap(gen, img, z, block, which, n):
    h = gen.native()
    dst = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    h.debug_tap(block, which, dst)
    gen(img, z)
    h.debug_tap(0, 0, None)
    torch.cuda.synchronize()
    return dst


def _u8(x):
    return ((x.double().clamp(-1, 1) + 1) / 2 * 255).round().to(torch.int16)


# ------------------------------------------------------------------------------------------------ the mode runs where it should
@pytest.mark.parametrize("golden", ["dec_nf64_bair", "dec_nf32_128"])
def test_fp16_mode_runs_the_one_term_kernel_on_every_f43_layer(golden):
    g, meta = load_golden(golden)
    img, z = cu(g["img"]), cu(g["z"])
    g1, g3 = _gen(meta, 1), _gen(meta, "fp16")
    assert g3.mma == 3
    k1, _ = _kernels(g1, img, z)
    k3, rows3 = _kernels(g3, img, z)
    assert set(k1) == set(k3)
    f43 = [n for n, k in k1.items() if k == "conv_wino4_f16x3"]
    assert f43, k1
    for n in k1:   # exactly the F(4,3) layers change kernel; every other layer keeps its mma = 1 kernel
        assert k3[n] == ("conv_wino4_f16" if n in f43 else k1[n]), (n, k1[n], k3[n])
    # one MFMA product per Winograd product: 1/3 of the split kernel's count on the same layer
    ex1 = {r["layer"]: r["mfma_flops"] for r in _kernels(g1, img, z)[1]}
    for r in rows3:
        if r["layer"] in f43:
            assert abs(r["mfma_flops"] * 3 - ex1[r["layer"]]) <= 1e-9 * ex1[r["layer"]], r
    a, b = g1(img, z), g3(img, z)
    assert bool(torch.isfinite(b).all()) and not torch.equal(a, b)
    assert g3.native().status() == 0


# ------------------------------------------------------------------------------------------------ tight pins: writer and conv
def _levels(meta):
    """Per block: (T, H, W, ut) of the level it runs at (i2v_dec_create)."""
    ups, upt = meta["upsample_s"], meta["upsample_t"]
    T, S, out = 1, 4, []
    for k in range(6):
        ut, us = (1, 1) if k == 0 else (2, 2) if k <= 3 else (upt[k - 4], ups[k - 4])
        T, S = T * ut, S * us
        out.append((T, S, S, ut))
    return out


def _sn_weight64(sd, name):
    w = sd[name + ".weight_orig"].double()
    u, v = sd[name + ".weight_u"].double(), sd[name + ".weight_v"].double()
    sigma = u @ (w.reshape(w.shape[0], -1) @ v)
    return w.float().double() / sigma


def _u16(w3):
    """[nset][Cout][Cin][KT][3][3] fp64 -> the packer's U: fp16(fp32(G g 2^wexp)) [nset][6][Cout][Cin][KT][3] and wexp."""
    g0, g1, g2 = w3[..., 0], w3[..., 1], w3[..., 2]
    u = torch.stack([g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6, g0 / 24 - g1 / 12 + g2 / 6, g2], 1)
    wmax = float(u.abs().max())
    wexp = max(-40, min(40, int(np.floor(np.log2(16384.0 / wmax)))))
    return (u * 2.0 ** wexp).float().half().double(), wexp


@pytest.mark.parametrize("golden", ["dec_nf64_bair", "dec_nf32_128"])
def test_fp16_conv_and_writer_pinned_to_the_tapped_operand(golden):
    import i2v_native
    g, meta = load_golden(golden)
    img, z = cu(g["img"]), cu(g["z"])
    g1, g3 = _gen(meta, 1), _gen(meta, "fp16")
    k3, _ = _kernels(g3, img, z)
    sd = g3.state_dict()
    nf = meta["synth"]["channel_factor"]
    cin_f = (16, 16, 16, 8, 4, 2)
    cout_f = (16, 16, 8, 4, 2, 1)
    names = ("head_0", "g_0", "g_1", "g_2", "g_3", "g_4")
    lv = _levels(meta)
    picked = {}
    for k in range(6):
        if k3[f"{names[k]}.conv_0"] == "conv_wino4_f16":
            picked.setdefault(lv[k][3] == 2, k)   # the first temporal-duplication block and the first plain one
    assert picked, k3
    # the writer is pinned on the FIRST one-term layer: every launch in front of it is the mma = 1 launch, so both writers see the
    # same activations (behind it they do not: the earlier fp16 convs have moved them by ~1e-3)
    first = min(i for i, n in enumerate(i2v_native.NativeDecoder.LAYER_NAMES) if k3[n] == "conv_wino4_f16")
    assert first % 2 == 0, k3
    for tdup, k in sorted(picked.items()):
        To, H, W, _ = lv[k]
        Cin, Cmid = cin_f[k] * nf, min(cin_f[k], cout_f[k]) * nf
        Cp, J, Ti = (Cin + 63) // 64 * 64, W // 4, To // 2 if tdup else To
        nv = Ti * H * W * Cp * 3 // 4                      # floats the one-term tap holds (B = 1)
        raw = _tap(g3, img, z, k, 1, nv)
        V = _v_onehot_channels(raw, 1, Ti, Cp, H, J)[..., :Cin].double()
        assert int((_v_onehot_channels(raw, 1, Ti, Cp, H, J)[..., Cin:] != 0).sum()) == 0    # padding channels are zeros
        out = _tap(g3, img, z, k, 2, To * H * W * Cmid).view(1, To, H, W, Cmid).double().cpu()
        if 2 * k == first:   # writer pin: the split tap holds the first 2/3 of the split operand's rows
            raw1 = _tap(g1, img, z, k, 1, Ti * H * W * Cin)
            nrows = Ti * H * W * Cin * 4 // 64
            hi = _v_split_hi(raw1, 1, Ti, Cin, H, J, nrows).view(-1)
            C16 = Cin // 16
            full = nrows // (C16 * 6 * H * J)                 # whole frames in the split tap
            mine = V[0, :full].float().half().view(full, 6, H, J, C16, 16).permute(0, 4, 1, 2, 3, 5).reshape(-1)
            ndiff = int((mine.view(torch.int16) != hi[: mine.numel()].view(torch.int16)).sum())
            print(f"{golden} {names[k]} writer: {ndiff} of {mine.numel()} fp16 values differ from the split writer's hi parts")
            assert ndiff == 0
        # conv pin: float64 recomputation from the tapped fp16 operand and the packer's fp16 weights
        w = _sn_weight64(sd, f"{names[k]}.conv_0").cpu()   # [Cmid][Cin][3][3][3]
        bias = sd[f"{names[k]}.conv_0.bias"].double().cpu()
        if tdup:
            w3 = torch.stack([torch.stack([w[:, :, 0], w[:, :, 1] + w[:, :, 2]], 2), torch.stack([w[:, :, 0] + w[:, :, 1], w[:, :, 2]], 2)])
        else:
            w3 = w[None]
        U, wexp = _u16(w3)                                 # [nset][6][Cmid][Cin][KT][3]

        def recompute(dt):
            Vc, Uc, bc = V.cpu().to(dt), U.to(dt), bias.to(dt)
            ref = torch.zeros(1, To, H, W, Cmid, dtype=dt)
            for par in range(Uc.shape[0]):
                M = []
                for x in range(6):
                    vx = Vc[:, :, x].permute(0, 4, 1, 2, 3)       # [1][Cin][Ti][H][J]
                    m = torch.nn.functional.conv3d(vx, Uc[par, x][..., None], padding=(1, 1, 0))
                    if tdup:   # parity 0: frames (t - 1, t), parity 1: (t, t + 1)
                        m = m[:, :, :Ti] if par == 0 else m[:, :, 1:Ti + 1]
                    M.append(m.permute(0, 2, 3, 4, 1))             # [1][T][H][J][Cmid]
                y = torch.stack([M[0] + M[1] + M[2] + M[3] + M[4], M[1] - M[2] + 2 * M[3] - 2 * M[4], M[1] + M[2] + 4 * M[3] + 4 * M[4],
                                 M[1] - M[2] + 8 * M[3] - 8 * M[4] + M[5]], 4)   # [1][T][H][J][4][Cmid]
                y = y.reshape(1, Ti, H, W, Cmid) * 2.0 ** -wexp + bc
                if tdup:
                    ref[:, par::2] = y
                else:
                    ref = y
            return ref
        ref = recompute(torch.float64)
        err = rel_l2(out, ref)
        noise = rel_l2(recompute(torch.float32).double(), ref)   # the same arithmetic in fp32 on the CPU, another summation order
        print(f"{golden} {names[k]} (tdup {tdup}): conv_0 rel-L2 vs the float64 recomputation {err:.2e} (CPU fp32: {noise:.2e})")
        # measured 6.6e-6 ... 1.26e-5 (the CPU's fp32 recomputation: 3.7e-7 ... 2.0e-6): the kernel accumulates the 9 Cin products of
        # a plane in one fp32 chain of MFMA k-steps, and A^T's cancellation (y3 = M1 - M2 + 8 M3 - 8 M4 + M5) amplifies what that
        # rounds; a wrong operand, weight or layout shows at >= 1e-3
        assert err <= 2e-5


# ------------------------------------------------------------------------------------------------ loose pins: frames and convs
def _frames_report(golden, out3, out1, ref):
    e = rel_l2(out3.cpu(), ref)
    d = (_u8(out3) - _u8(out1)).abs()
    within1, dmax = float((d <= 1).double().mean()), int(d.max())
    print(f"{golden}: frames rel-L2 vs golden {e:.2e} (mma = 1: {rel_l2(out1.cpu(), ref):.2e}); uint8 vs mma = 1: "
          f"{100 * within1:.3f} % within +-1, max |delta| {dmax}")
    return e, within1, dmax


@pytest.mark.parametrize("golden", ["dec_nf64_bair", "dec_nf32_128"])
def test_fp16_frames_and_convs_against_fp32(golden):
    g, meta = load_golden(golden)
    img, z = cu(g["img"]), cu(g["z"])
    g0, g1, g3 = _gen(meta, 0), _gen(meta, 1), _gen(meta, "fp16")
    out3, out1 = g3(img, z), g1(img, z)
    e, within1, dmax = _frames_report(golden, out3[..., ::2, ::2], out1[..., ::2, ::2], torch.from_numpy(g["out_s2"]))
    assert e <= FRAME_BOUND[golden] <= FRAME_CEIL
    assert within1 >= U8_WITHIN1 and dmax <= U8_MAXDELTA
    k3, _ = _kernels(g3, img, z)
    names = ("head_0", "g_0", "g_1", "g_2", "g_3", "g_4")
    nf = meta["synth"]["channel_factor"]
    lv = _levels(meta)
    worst = 0.0
    for k in range(6):
        To, H, W, _ = lv[k]
        for i, which in ((0, 2), (1, 5)):
            if k3[f"{names[k]}.conv_{i}"] != "conv_wino4_f16":
                continue
            c = (min((16, 16, 8, 4, 2, 1)[k], (16, 16, 16, 8, 4, 2)[k]) if i == 0 else (16, 16, 8, 4, 2, 1)[k]) * nf
            n = To * H * W * c
            a, b = _tap(g3, img, z, k, which, n), _tap(g0, img, z, k, which, n)
            # the conv's output tap (conv_1: the block output, conv_1 + shortcut) on the same start frame and latent: what this conv
            # adds AND what the earlier convs carried into its input -- an upper bound of the conv's own error
            err = float(((a.double() - b.double()).norm() / b.double().norm()))
            print(f"{golden} {names[k]}.conv_{i}: output rel-L2 vs mma = 0 {err:.2e}")
            worst = max(worst, err)
    assert worst <= CONV_BOUND <= CONV_CEIL


def test_fp16_model_against_golden(tmp_path):
    from test_gpu_parity import _write_checkpoints
    from get_model import Model
    g, meta = load_golden("model_nf8")
    ck = _write_checkpoints(tmp_path, meta)
    m3, m1 = Model(ck, 32, mma="fp16"), Model(ck, 32, mma=1)
    assert m3.decoder.mma == 3 and m1.decoder.mma == 1
    y3 = m3(cu(g["x1"]), residual=cu(g["r1"]), embed=cu(g["e1"]))
    y1 = m1(cu(g["x1"]), residual=cu(g["r1"]), embed=cu(g["e1"]))
    e, within1, dmax = _frames_report("model_nf8", y3, y1, torch.from_numpy(g["y32"]))
    assert e <= FRAME_BOUND["model_nf8"] and within1 >= U8_WITHIN1 and dmax <= U8_MAXDELTA
    m3.check()


# ------------------------------------------------------------------------------------------------ determinism
def test_fp16_determinism_shards_repeats_graph():
    _, meta = load_golden("dec_nf64_bair")
    gen = _gen(meta, "fp16")
    img8, z8, _ = synth.bench_inputs(8, 64, 64)
    img8, z8 = img8.cuda(), z8.cuda()
    full = gen(img8, z8).clone()
    for r0 in (0, 2, 6):
        assert torch.equal(gen(img8[r0:r0 + 2].contiguous(), z8[r0:r0 + 2].contiguous()), full[r0:r0 + 2])
    assert torch.equal(gen(img8, z8), full)
    x_s, z_s = img8.clone(), z8.clone()
    gen(x_s, z_s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_s = gen(x_s, z_s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_s, full)


# ------------------------------------------------------------------------------------------------ range guard
def test_fp16_range_guard(tmp_path):
    import i2v_native
    from stage1_VAE.modules.decoder import Generator
    from test_gpu_parity import _write_checkpoints
    from get_model import Model
    sd = T(synth.decoder_state_dict(seed=5, channel_factor=32))
    sd["g_3.norm_0.conv_gamma.bias"] = sd["g_3.norm_0.conv_gamma.bias"] * 0 + 3.0e6   # SPADE (1 + gamma) past the fp16 range
    cfg = {"channel_factor": 32, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True, "mma": "fp16"}
    x0, z, _ = synth.bench_inputs(2, 64, 64)
    gen = Generator(cfg)
    gen.load_state_dict(sd)
    gen = gen.cuda().eval()
    k, _ = _kernels(gen, x0.cuda(), z.cuda())
    assert k["g_3.conv_0"] == "conv_wino4_f16", k
    gen.native().status(reset=True)
    gen(x0.cuda(), z.cuda())
    assert gen.native().status() & 1
    with pytest.raises(i2v_native.I2VError, match="fp16 range"):
        gen(x0.cuda(), z.cuda())
    assert gen.native().status(reset=True) & 1 and gen.native().status() == 0
    # Model.check() names the fallback of this mode
    g, meta = load_golden("model_nf8")
    model = Model(_write_checkpoints(tmp_path, meta), 16, mma="fp16")
    sd8 = model.decoder.state_dict()
    sd8["g_2.norm_0.conv_gamma.bias"] = sd8["g_2.norm_0.conv_gamma.bias"] * 0 + 3.0e6
    model.decoder.load_state_dict(sd8)
    model(cu(g["x1"]), residual=cu(g["r1"]), embed=cu(g["e1"]))
    with pytest.raises(RuntimeError, match="mma = fp16"):
        model.check()


# ------------------------------------------------------------------------------------------------ stand-alone GeneratorBlock
@pytest.mark.parametrize("wino4", [None, "2"])
def test_fp16_generator_block_shape_sweep(wino4, monkeypatch):
    """GeneratorBlock(..., mma="fp16") against the same block in mma = 1 over the geometries of
    test_generator_block_shape_sweep_winograd_and_fallback (I2V_DEC_WINO4=2: the F(4,3) kernel wherever its tiling allows)."""
    from stage1_VAE.modules import decoder as dec
    monkeypatch.delenv("I2V_DEC_MMA", raising=False)
    if wino4:
        monkeypatch.setenv("I2V_DEC_WINO4", wino4)
    sd = T(synth.decoder_state_dict(seed=5, channel_factor=8))
    g = torch.Generator().manual_seed(31)
    worst = 0.0
    for name, n_out in (("g_0", 128), ("g_1", 64)):
        part = {k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}
        blk1 = dec.GeneratorBlock(128, n_out, True, 64, mma=1)
        blk3 = dec.GeneratorBlock(128, n_out, True, 64, mma="fp16")
        blk1.load_state_dict(part)
        blk3.load_state_dict(part)
        blk1, blk3 = blk1.cuda().eval(), blk3.cuda().eval()
        for (B, Tn, H, W) in ((2, 1, 16, 16), (1, 2, 16, 16), (1, 4, 8, 8), (1, 4, 16, 16), (2, 4, 8, 32), (1, 8, 32, 16),
                              (1, 16, 16, 8), (1, 2, 8, 64)):
            x = torch.randn(B, 128, Tn, H, W, generator=g).cuda()
            img = (2 * torch.rand(B, 3, 24, 40, generator=g) - 1).cuda()
            z = torch.randn(B, 64, generator=g).cuda()
            a, b = blk1(x, z, img), blk3(x, z, img)
            err = float((a.double() - b.double()).norm() / a.double().norm())
            worst = max(worst, err)
            assert bool(torch.isfinite(b).all()) and err <= BLOCK_BOUND, (name, B, Tn, H, W, err)
    print(f"GeneratorBlock sweep (I2V_DEC_WINO4={wino4}): worst rel-L2 fp16 vs mma = 1 {worst:.2e}")
    if wino4:
        assert worst > 0.0   # the one-term kernel really ran somewhere
