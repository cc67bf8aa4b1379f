"""The units of the stage-1 decoder's GeneratorBlocks one by one against float64 at derived element-wise bounds: the fused and the
stand-alone normalisation statistics, ``coef_kernel``'s (A, B) tables, the four operand writers (``modulate_kernel<HL16>``,
``modulate_wino_kernel``, ``modulate_wino4_kernel<GB, ONE>``, ``modulate_wino4_f32``) and the 3x3x3 convs given their operand (direct
fp32, direct split-fp16 with its split-K pass, split F(2,3), split and one-term F(4,3), exact-fp32 F(4,3)) with their fused epilogues.

Per (configuration, mode) every one of the six blocks is tapped (i2v_dec_debug_tap, taps 0 .. 12, each into a NaN-filled buffer: a tap
that is not written fails) and every unit is recomputed in float64 from what the GPU itself left in the taps in front of it -- the
bound of a unit holds per unit, not along the chain.  References, layout decoders, bounds and the gate: tests/dec_units_common.py
(checked on the CPU by tests/test_host_dec_units.py).  The float64 references run on the GPU as matmuls over shifted views.

Configurations (tests/test_gpu_decoder_configs.py, B = 2 with distinct start frames): nf24_p11 (ragged 48 / 24, 12 SPADE groups, F(4,3) with
three tiles), nf8_s4 (x4 spatial, tdup at g_4), nf16_t4 (x4 temporal, residual factor 4), nf40_bair (Cout 80 -> pad 128, five tiles) --
the smallest decoders that reach every writer and epilogue variant -- in the modes mma1, mma1_w4all, mma1_f23, mma1_direct, mma0,
mma0_direct and mma = "fp16".  The measured fractions of the bounds: profiles/dec_units_gate.md."""
import pytest
import torch

import dec_units_common as du
from test_gpu_decoder_configs import CONFIGS, MODES, _handle, _inputs, _set_env, layer_kernels

pytestmark = pytest.mark.gpu
UNIT_CONFIGS = ("nf24_p11", "nf8_s4", "nf16_t4", "nf40_bair")
UNIT_MODES = {m: MODES[m] for m in ("mma1", "mma1_w4all", "mma1_f23", "mma1_direct", "mma0", "mma0_direct")}
UNIT_MODES["fp16"] = ("fp16", {})
LEDGER = set()
WORST = {}
RAN = set()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(prev)
    # the source of profiles/dec_units_gate.md: whatever ran in this session, printed once at its end
    print("\nDECUNITS worst |err| / bound per unit kind:", {k: f"{v:.3f}" for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module", params=UNIT_CONFIGS)
def config(request):
    sd, img, z = _inputs(request.param)
    yield {"name": request.param, "sd": sd, "img": img.cuda(), "z": z.cuda()}
    torch.cuda.empty_cache()


def _tap(h, cfg, k, which, n):
    dst = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    h.debug_tap(k, which, dst)
    h.forward(cfg["img"], cfg["z"])
    h.debug_tap(0, 0, None)
    torch.cuda.synchronize()
    return dst


def _tap64(h, cfg, k, which, pairs):
    dst = h.debug_tap_f64(k, which, pairs, "cuda")
    h.forward(cfg["img"], cfg["z"])
    h.debug_tap(0, 0, None)
    torch.cuda.synchronize()
    return dst


def _note(worst, key, f, bad, what):
    worst[key] = max(worst.get(key, 0.0), f)
    WORST[key] = max(WORST.get(key, 0.0), f)
    if not f <= 1.0:
        bad.append(f"{what} {key}: |err| / bound {f:.3g}")


@pytest.mark.parametrize("mode", list(UNIT_MODES))
def test_decoder_units_vs_fp64(config, mode, monkeypatch):
    """Every unit of every block of one configuration in one mode within its derived bound."""
    import i2v_native
    mma, env = UNIT_MODES[mode]
    _set_env(monkeypatch, env)
    name = config["name"]
    nf, ups, upt, _, _ = CONFIGS[name]
    h = _handle(config, i2v_native.parse_mma(mma))
    codes = layer_kernels(h, config["img"], config["z"])
    sd, z = config["sd"], config["z"]
    B = z.shape[0]
    lv = du.levels(ups, upt)
    worst, bad = {}, []
    prev_fused = False
    for k in range(6):
        blk = du.NAMES[k]
        T, H, W, ut, us = lv[k]
        Tl, Hl, Wl = T // ut, H // us, W // us
        n_in, n_out = du.CIN[k] * nf, du.COUT[k] * nf
        n_mid = min(n_in, n_out)
        learned = n_in != n_out
        kind0, kind1 = du.KERNELS[codes[2 * k]], du.KERNELS[codes[2 * k + 1]]
        split0, split1 = kind0 in du.SPLIT, kind1 in du.SPLIT
        tdup = ut == 2 and split0                  # conv_0 behind a x2 temporal up-sampling reads the half-rate operand (split kernels)
        Ti, ut0 = (T // 2, 1) if tdup else (T, ut)
        fused2 = split0 and du.can_fuse_stats(T // 2 if ut == 2 else T, H, W)
        fused_out = split1 and du.can_fuse_stats(T, H, W) and k != 5
        LEDGER.update({("learned" if learned else "identity"), ("ut", ut), ("us", us), ("stats_in", "fused" if prev_fused else "kernel", min(k, 2)),
                       ("stats_mid", "fused" if fused2 else "kernel", min(k, 2))})
        if tdup:
            LEDGER.add(("tdup", kind0))
        for kind, co, cin, fused in ((kind0, n_mid, n_in, fused2), (kind1, n_out, n_mid, fused_out)):
            if co % 32:
                LEDGER.add(("ragged_cout", kind))
            if kind == "hl16" and not fused and du.splitk_factor(T * H * W, (cin + 31) // 32) > 1:
                LEDGER.add("splitk")
        tag = f"{blk}"
        # ---- block input, its statistics, SPADE's table
        x = _tap(h, config, k, 12, B * Tl * Hl * Wl * n_in).view(B, Tl, Hl, Wl, n_in)
        s_in = _tap64(h, config, k, 8, B * n_in).view(B, n_in, 2)
        ref, bound = du.stats_ref(x)
        _note(worst, "stats", du.within(s_in, ref, bound, rel=du.U64), bad, tag + " input")
        LEDGER.add(("stats", "fused" if prev_fused else "kernel"))
        c0 = _tap(h, config, k, 9, B * n_in * 2).view(B, n_in, 2)
        ref, bound = du.coef_ref(s_in, du.spade_groups(n_in), Tl * Hl * Wl)
        _note(worst, "coef", du.within(c0, ref, bound), bad, tag + " spade")
        # ---- conv_0: writer and conv
        gb = _tap(h, config, k, 0, B * H * W * 2 * n_in).view(B, H, W, 2 * n_in)
        raw = _tap(h, config, k, 1, du.operand_floats(kind0, B, Ti, H, W, n_in))
        opnd = du.decode_operand(kind0, raw, B, Ti, H, W, n_in)
        if kind0 == "f43_one":
            assert int((du.decode_operand(kind0, raw, B, Ti, H, W, n_in, parts=True)[1] != 0).sum()) == 0, (tag, "padding channels")
        ref, S = du.writer_ref(kind0, x, c0, gb, ut0, us)
        _note(worst, "writer_" + kind0, du.within(opnd, ref, du.writer_bound(kind0, ref, S)), bad, tag + " conv_0")
        LEDGER.add(("writer", kind0, "gb"))
        dx = _tap(h, config, k, 2, B * T * H * W * n_mid).view(B, T, H, W, n_mid)
        w0 = du.sn_weight64(sd, blk + ".conv_0").cuda()
        ref, S, S1 = du.conv_ref(kind0, opnd, w0, sd[blk + ".conv_0.bias"].double(), None, 1, 1, False, tdup)
        _note(worst, "conv_" + kind0, du.within(dx, ref, du.conv_bound(kind0, n_in, tdup, w0, S, S1)), bad, tag + " conv_0")
        LEDGER.add(("conv", kind0, 0))
        del opnd, raw, ref, S, S1, gb
        # ---- ADAIN: statistics of conv_0's output, its table, conv_1's writer
        s2 = _tap64(h, config, k, 6, B * n_mid).view(B, n_mid, 2)
        ref, bound = du.stats_ref(dx)
        _note(worst, "stats", du.within(s2, ref, bound, rel=du.U64), bad, tag + " conv_0 output")
        LEDGER.add(("stats", "fused" if fused2 else "kernel"))
        c1 = _tap(h, config, k, 10, B * n_mid * 2).view(B, n_mid, 2)
        adain = (z.double(), sd[blk + ".norm_1.linear.weight"].double(), sd[blk + ".norm_1.linear.bias"].double())
        ref, bound = du.coef_ref(s2, n_mid, T * H * W, adain=adain)
        _note(worst, "coef", du.within(c1, ref, bound), bad, tag + " adain")
        raw = _tap(h, config, k, 3, du.operand_floats(kind1, B, T, H, W, n_mid))
        opnd = du.decode_operand(kind1, raw, B, T, H, W, n_mid)
        if kind1 == "f43_one":
            assert int((du.decode_operand(kind1, raw, B, T, H, W, n_mid, parts=True)[1] != 0).sum()) == 0, (tag, "padding channels")
        ref, S = du.writer_ref(kind1, dx, c1, None, 1, 1)
        _note(worst, "writer_" + kind1, du.within(opnd, ref, du.writer_bound(kind1, ref, S)), bad, tag + " conv_1")
        LEDGER.add(("writer", kind1, "adain"))
        # ---- shortcut table, conv_1 with its epilogue, the statistics it leaves for the next block
        res = x
        if learned:
            cs = _tap(h, config, k, 11, B * n_in * 2).view(B, n_in, 2)
            ref, bound = du.coef_ref(s_in, 16, Tl * Hl * Wl, affine=(sd[blk + ".norm_s.bn.weight"], sd[blk + ".norm_s.bn.bias"]))
            _note(worst, "coef", du.within(cs, ref, bound), bad, tag + " shortcut")
            res = _tap(h, config, k, 4, B * Tl * Hl * Wl * n_out).view(B, Tl, Hl, Wl, n_out)
        out = _tap(h, config, k, 5, B * T * H * W * n_out).view(B, T, H, W, n_out)
        w1 = du.sn_weight64(sd, blk + ".conv_1").cuda()
        ref, S, S1 = du.conv_ref(kind1, opnd, w1, sd[blk + ".conv_1.bias"].double(), res.double(), ut, us, k == 5, False)
        _note(worst, "conv_" + kind1, du.within(out, ref, du.conv_bound(kind1, n_mid, False, w1, S, S1)), bad, tag + " conv_1")
        LEDGER.add(("conv", kind1, 1))
        LEDGER.add(("residual", kind1, ut, us))
        if k == 5:
            LEDGER.add(("lrelu", kind1))
        if fused_out:
            so = _tap64(h, config, k, 7, B * n_out).view(B, n_out, 2)
            ref, bound = du.stats_ref(out)
            _note(worst, "stats", du.within(so, ref, bound, rel=du.U64), bad, tag + " output")
        prev_fused = fused_out
        del opnd, raw, ref, S, S1, x, dx, out, res
    assert h.status() == 0, (name, mode)
    RAN.add((name, mode))
    print(f"DECUNITS {name} {mode} kernels {codes}: " + ", ".join(f"{k_} {v:.3f}" for k_, v in sorted(worst.items())))
    assert not bad, f"{name} {mode} kernels {codes}: " + "; ".join(bad)


def test_ledger_every_unit_on_every_kernel():
    """Over the matrix every unit kind ran on every kernel code it exists for, and every case of the block code occurred."""
    assert len(RAN) == len(UNIT_CONFIGS) * len(UNIT_MODES), "the ledger needs the whole module to have run"
    print("DECUNITS ledger:", sorted(map(str, LEDGER)))
    for kind in du.KERNELS.values():
        for conv in (0, 1):
            assert ("conv", kind, conv) in LEDGER, (kind, conv)
        assert ("writer", kind, "gb") in LEDGER and ("writer", kind, "adain") in LEDGER, kind
    # statistics: the stand-alone kernel at head_0 / g_0 (maps below one 256-position brick) and at the later levels (exact-fp32
    # modes), the fused epilogues at the later levels; both for the block input and for conv_0's output
    for which in ("stats_in", "stats_mid"):
        for level in (0, 1, 2):
            assert (which, "kernel", level) in LEDGER, (which, level)
        assert (which, "fused", 2) in LEDGER, which
    for kind in ("hl16", "f23", "f43", "f43_one"):
        assert ("tdup", kind) in LEDGER, kind
    for f in (1, 2, 4):
        assert ("ut", f) in LEDGER and ("us", f) in LEDGER, f
    # (x4 in space reaches 16- and 8-channel layers only in these configurations: the direct and the exact-fp32 kernels)
    for kind in ("hl16", "f23", "f43", "f43_one", "f32", "f43_f32"):
        assert any(isinstance(e, tuple) and e[:2] == ("residual", kind) and e[2] == 4 for e in LEDGER), ("x4 residual in time", kind)
    for kind in ("hl16", "f32", "f43_f32"):
        assert any(isinstance(e, tuple) and e[:2] == ("residual", kind) and e[3] == 4 for e in LEDGER), ("x4 residual in space", kind)
    assert "learned" in LEDGER and "identity" in LEDGER and "splitk" in LEDGER
    assert ("ragged_cout", "hl16") in LEDGER and ("ragged_cout", "f32") in LEDGER
    assert any(isinstance(e, tuple) and e[0] == "lrelu" for e in LEDGER)
