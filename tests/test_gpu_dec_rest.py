"""The decoder's units outside the twelve 3x3x3 block convs, one by one against float64 at derived element-wise bounds
(tests/dec_rest_common.py, checked on the CPU by tests/test_host_dec_rest.py; the measured fractions: profiles/dec_rest_gate.md).

conv_img -- through i2v_native.conv_img_unit, i.e. ConvImgSet::pack / conv_img_form / conv_img_run of csrc/i2v_convimg.hip, the three
functions the decoder itself goes through -- in all four forms at the smallest shapes that reach each edge:
  fused matrix cores   C in {16, 32, 48, 64} (KS = 1 .. 4) x {(1, 1, 8, 32): one brick, both outer temporal taps are padding; (2, 2, 8, 64): a
                       brick seam in W; (2, 3, 16, 64): seams in H and W and an interior frame}; the multi-frame schedule by the
                       production rule (C = 16, (1, 2, 512, 768): 1536 bricks -> 2 frames per workgroup) and forced to 2, 4, 8, 16 frames
                       (measurement build, tests/dec_rest_worker.py in a process of its own): bits equal to one frame per workgroup
  GEMM + gather        C in {64, 68} x {(1, 3, 7, 9), (2, 4, 16, 32)}: the transposed 81-column split-fp16 GEMM (the decoder under I2V_DEC_IMG16=1)
  vector ALU           C in {8, 12, 24, 40} x {(1, 8, 8, 8), (2, 8, 16, 24)}.  The issue's (1, 4, 8, 8) is refused by this form's predicate
                       (its brick holds 8 frames: T % 8 == 0) -- asserted as a refusal; one brick is (1, 8, 8, 8).
  generic              C = 8 x {(1, 4, 4, 4), (3, 2, 8, 8)}.  The issue's shape (1, 3, 7, 9) cannot run in this form: conv_forward tiles its
                       output into 128-position bricks and refuses (I2V_E_INVALID) geometries that do not tile -- asserted here as a
                       refusal.  NO decoder configuration reaches this form: i2v_dec_create wants channel_factor % 8 == 0, every
                       decoder ends at T = 8 * upsample_t products (a multiple of 8) and H = W = 32 * upsample_s products, so
                       conv_img_supported (T, H, W % 8 == 0, C % 4 == 0) always holds and conv_img_form never falls through to it.
Per form: a batch of 3 equals three single-sample runs bit for bit, samples stored further apart than dense leave a sentinel in the
gaps, the range flag stays clear, a form named for a geometry its predicate refuses raises I2VError.

SPADE's branch -- taps 13 (resized start frame), 14 (lrelu(Conv2d(3, 128))), 15 (Winograd operand) and 0 (gamma | beta maps) of every
block, each unit recomputed in float64 from the tap in front of it: the resize against bilinear align_corners=True (fp32 and split-fp16
rows, channels 3 .. 15 exactly zero, start frames read through a sample stride larger than dense, a non-square 48 x 80 start frame in
two configurations), Conv2d(3, 128) + lrelu from the rows, the KT = 1 Winograd operand writers (no table, no maps) from the activation,
and the gamma | beta conv ("+1" in the gamma bias) from its operand.  Modes: mma 1 (F(4,3) where 2C % 64 == 0 and the level tiles, else
F(2,3), else direct), I2V_DEC_WINO4=0 (F(2,3)), I2V_DEC_SPW=0 (direct split-fp16, the activation handed over in the operand format),
mma 0 (exact fp32) and "fp16", which takes the forms of mma 1 (the branch has no one-term kernel: wino4_supported refuses KT = 1
there, and spade_w4_wanted asks for the split form).  i2v_dec_get_spade_form tells the form per block; the ledger wants every form at a
level of 64 x 64 or larger and the direct and fp32 forms at the 4 x 4 / 8 x 8 levels too -- neither Winograd form tiles a map below 32
rows (wino4_tiling / wino16_tiling: one sample's brick is 32 rows high at T = 1).

Shortcut GEMM and fc -- through the decoder (taps 12, 11, 4 of every learned block: (x A + B) @ W_sn from the GPU's own x and (A, B)
table; tap 12 of head_0: fc(z)) in mma 1, mma 1 + I2V_DEC_PW16=0, mma 0 and "fp16" (which runs the split-fp16 GEMM: only the F(4,3)
block convs differ from mma 1) at nf 8, 16, 24, 40 (CoutPad 32, 64, 96 -> 128 and 128-multiples, ragged Cout 24 and 80), and through
i2v_native.pointwise_unit (pointwise16_forward / pointwise_forward behind it) for the tile forms no test-size decoder reaches:
128 x 128, 128 x 64, 128 x 32 and the transposed 128 x 128, with and without the affine (a 128-row tile straddling two samples'
coefficient rows), residual + lrelu, and the exact-fp32 GEMM at the same shapes.  (A 64 x 64 tile could never be selected by the tile
rule and was removed: DESIGN.md.)"""
import json
import os
import subprocess
import sys

import pytest
import torch

import dec_rest_common as dr
import dec_units_common as du
from test_gpu_decoder_configs import B as DEC_B, CONFIGS, _handle, _inputs, _set_env

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}
LEDGER = set()

MFMA_SHAPES = ((1, 1, 8, 32), (2, 2, 8, 64), (2, 3, 16, 64))
IMG_CASES = ([("mfma", C, s) for C in (16, 32, 48, 64) for s in MFMA_SHAPES] + [("mfma", 16, (1, 2, 512, 768))] +
             [("gemm", C, s) for C in (64, 68) for s in ((1, 3, 7, 9), (2, 4, 16, 32))] +
             [("valu", C, s) for C in (8, 12, 24, 40) for s in ((1, 8, 8, 8), (2, 8, 16, 24))] + [("generic", 8, s) for s in ((1, 4, 4, 4), (3, 2, 8, 8))])
SMALLEST = {"mfma": (32, (1, 8, 32)), "gemm": (68, (3, 7, 9)), "valu": (12, (8, 8, 8)), "generic": (8, (4, 4, 4))}

# (name, M, P, Cin, Cout, transposed)
PW_SHAPES = (("128x128", 65536 + 37, 32800, 32, 128, False), ("128x64", 65536 + 37, 32800, 36, 64, False), ("128x32", 300, 130, 12, 24, False),
             ("transposed", 4096 + 5, 2050, 32, 81, True))
PW_TILE = {"128x128": 128, "128x64": 64, "128x32": 32, "transposed": 128}
DEC_CONFIGS = ("nf8_s4", "nf16_t4", "nf24_p11", "nf40_bair")
DEC_MODES = {"mma1": (1, {}, "hl16"), "mma1_pw32": (1, {"I2V_DEC_PW16": "0"}, "f32"), "mma0": (0, {}, "f32"), "fp16": ("fp16", {}, "hl16")}
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
    # the source of profiles/dec_rest_gate.md: whatever ran in this session, printed once at its end
    print("\nDECREST worst |err| / bound per unit:", {k: f"{v:.3f}" for k, v in sorted(WORST.items())})


def _note(key, f):
    WORST[key] = max(WORST.get(key, 0.0), f)
    return f


# ------------------------------------------------------------------------------------------------------ tanhf
def test_device_tanhf_ulp():
    """Device tanhf against float64 tanh of the same fp32 arguments, through conv_img's exact-fp32 vector-ALU form with a one-hot
    weight (every other product is x * 0 added exactly, bias 0: the output is tanhf(x) of the chosen argument).  dec_rest_common.C_TANH
    is twice the largest error found here."""
    import i2v_native
    T, H, W, C = 8, 32, 32, 4
    n = T * H * W * 3
    g = torch.Generator().manual_seed(1)
    mag = torch.cat((torch.linspace(0, 9.5, n // 2), 2.0 ** (torch.rand(n - n // 2, generator=g) * 24 - 20)))
    arg = (mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()
    x = torch.randn(1, T, H, W, C, generator=g)
    x[..., :3] = arg.view(1, T, H, W, 3)
    w = torch.zeros(3, C, 3, 3, 3)
    for o in range(3):
        w[o, o, 1, 1, 1] = 1.0
    info = {}
    got = i2v_native.conv_img_unit(x.cuda(), w, torch.zeros(3), form="valu", info=info).cpu()
    assert info["form"] == "valu"
    ref = torch.tanh(x[..., :3].double()).permute(0, 1, 4, 2, 3)
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23)
    err = ((got.double() - ref).abs() / ulp)
    worst = float(err.max())
    at = float(x[..., :3].permute(0, 1, 4, 2, 3).reshape(-1)[int(err.argmax())])
    print(f"DECREST device tanhf: {n} arguments in +-9.5, largest error {worst:.3f} ulp at x = {at:.6g}; C_TANH = {dr.C_TANH}")
    assert worst <= dr.C_TANH / 2, worst


# ------------------------------------------------------------------------------------------------------ conv_img
@pytest.mark.parametrize("form,C,shape", IMG_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_conv_img_form_vs_fp64(form, C, shape):
    import i2v_native
    B, T, H, W = shape
    x, w, bias = dr.conv_img_inputs(B, T, H, W, C, 1000 + C + T * H)
    xg = x.cuda()
    info = {}
    got = i2v_native.conv_img_unit(xg, w, bias, form=form, info=info)
    assert info["form"] == form and info["range_flag"] == 0, info
    ref, S, S1, SW = dr.conv_img_ref(xg, w, bias)
    assert dr.saturated_share(ref) < 0.01 and float(ref.abs().max()) > 0.9, "pre-activations span about +-3, < 1 % saturated"
    f = _note("conv_img_" + form, dr.within(got, ref, dr.conv_img_bound(form, C, w.cuda(), ref, S, S1, SW), rel=0.0))
    del ref, S, S1, SW
    LEDGER.add(("form", form))
    if form == "mfma":
        LEDGER.add(("tch", info["tch"]))
        LEDGER.add(("ks", C // 16))
    # samples further apart than dense: same bits, the gaps untouched
    dense = T * 3 * H * W
    if B * dense <= 1 << 22:
        buf = torch.full((B, dense + 40), -7.0, device="cuda")
        out = buf[:, :dense].view(B, T, 3, H, W)
        i2v_native.conv_img_unit(xg, w, bias, form=form, out=out, info=info)
        assert torch.equal(out, got) and bool((buf[:, dense:] == -7.0).all()) and info["range_flag"] == 0, (form, C, shape)
    print(f"DECREST conv_img {form} C {C} {shape} tch {info['tch']}: |err| / bound {f:.3f}")
    assert f <= 1.0, (form, C, shape, f)


@pytest.mark.parametrize("form", dr.FORMS)
def test_conv_img_batch_of_three_equals_three_single_runs(form):
    import i2v_native
    C, (T, H, W) = SMALLEST[form]
    x, w, bias = dr.conv_img_inputs(3, T, H, W, C, 77)
    xg = x.cuda()
    whole = i2v_native.conv_img_unit(xg, w, bias, form=form)
    for b in range(3):
        one = i2v_native.conv_img_unit(xg[b:b + 1].contiguous(), w, bias, form=form)
        assert torch.equal(one[0], whole[b]), (form, b)


def test_conv_img_choice_and_refusals():
    """form=None is what a split-fp16 decoder of the geometry runs; a named form is refused where its predicate says no."""
    import i2v_native
    for C, shape, want in ((16, (1, 8, 8, 32), "mfma"), (8, (1, 8, 8, 32), "valu"), (80, (1, 8, 8, 32), "valu"), (8, (1, 4, 4, 4), "generic")):
        x, w, bias = dr.conv_img_inputs(*shape, C, 5)
        info = {}
        got = i2v_native.conv_img_unit(x.cuda(), w, bias, info=info)
        assert info["form"] == want, (C, shape, info)
        assert torch.equal(got, i2v_native.conv_img_unit(x.cuda(), w, bias, form=want))
        LEDGER.add(("auto", want))
    for form, C, shape in (("mfma", 8, (1, 8, 8, 32)), ("mfma", 16, (1, 8, 8, 24)), ("mfma", 80, (1, 8, 8, 32)), ("gemm", 32, (1, 8, 8, 32)),
                           ("valu", 8, (1, 4, 8, 8)), ("valu", 8, (1, 8, 8, 12)), ("generic", 8, (1, 3, 7, 9)), (None, 8, (1, 3, 7, 9))):
        x, w, bias = dr.conv_img_inputs(*shape, C, 5)
        with pytest.raises(i2v_native.I2VError):
            i2v_native.conv_img_unit(x.cuda(), w, bias, form=form)


def test_conv_img_forced_frames_per_workgroup_keep_the_bits():
    """I2V_CONVIMG_TCH in {2, 4, 8, 16} (measurement build, a process of its own): C = 32, (1, 16, 8, 32); every value gives the bits of
    one frame per workgroup, which is the one compared with float64."""
    import i2v_native
    if not os.path.exists(i2v_native.MEASURE_LIB_PATH):
        i2v_native.build_measure()                               # (normally built by __graft_entry__.build())
    env = dict(os.environ, I2V_LIB_PATH=os.path.join("image2video-synthesis-using-cinns_amd", "lib", "libi2v_hip_measure.so"))
    env.pop("I2V_CONVIMG_TCH", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "dec_rest_worker.py")], env=env, capture_output=True, text=True, timeout=300,
                       cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"DECREST conv_img forced TCH: {res}")
    assert res["tch"] == [1, 2, 4, 8, 16] and res["equal"] == [True] * 4 and res["range_flag"] == 0, res
    _note("conv_img_mfma", res["fraction"])
    assert res["fraction"] <= 1.0, res
    for t in res["tch"]:
        LEDGER.add(("tch_forced", t))


# ------------------------------------------------------------------------------------------------------ pointwise GEMM, unit entry
@pytest.mark.parametrize("kind", ("hl16", "f32"))
@pytest.mark.parametrize("shape", PW_SHAPES, ids=lambda s: s[0])
def test_pointwise_unit_vs_fp64(shape, kind):
    import i2v_native
    name, M, P, Cin, Cout, transposed = shape
    transposed = transposed and kind == "hl16"          # (the exact-fp32 GEMM at the same shape, plain output)
    variants = [(False, False), (False, True)] if transposed else [(a, e) for a in (False, True) for e in (False, True)]
    for affine, epi in variants:                        # epi: residual + lrelu (the transposed form takes no residual: lrelu alone)
        x, w, b, coef, r = dr.pw_inputs(M, P, Cin, Cout, 31 * M % 1000 + Cin + affine + 2 * epi, affine, epi and not transposed)
        xg, cg, rg = x.cuda(), None if coef is None else coef.cuda().contiguous(), None if r is None else r.cuda()
        info = {}
        got = i2v_native.pointwise_unit(xg, w, b, res=rg, coef=cg, rows_per_sample=P, lrelu=epi, split16=kind == "hl16", transposed=transposed,
                                        info=info)
        if transposed:
            assert got.shape == (Cout, M)
            got = got.t()
        want_tile = 32 if name == "transposed" and not transposed else PW_TILE[name]     # (Cout 81 -> pad 128 at 33 row tiles: narrowed to 32)
        assert info["range_flag"] == 0 and info["tile_n"] == want_tile, (name, kind, info)
        if affine:
            assert M > P and P % 128, "a 128-row tile straddles two samples' coefficient rows"
        ref, S, S1, SW = dr.pw_ref(xg, w, b, rg, cg, P, epi)
        f = _note("pointwise_" + kind + ("_t" if transposed else ""), dr.within(got, ref, dr.pw_bound(kind, Cin, w, S, S1, SW, affine)))
        print(f"DECREST pointwise {kind} {name} affine {affine} res/lrelu {epi}: tile 128 x {info['tile_n']}, |err| / bound {f:.3f}")
        assert f <= 1.0, (name, kind, affine, epi, f)
        LEDGER.add(("pw", kind, "transposed" if transposed else info["tile_n"], affine, epi))


# ------------------------------------------------------------------------------------------------------ shortcut GEMM and fc in the decoder
@pytest.fixture(scope="module", params=DEC_CONFIGS)
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


@pytest.mark.parametrize("mode", list(DEC_MODES))
def test_decoder_shortcut_and_fc_vs_fp64(config, mode, monkeypatch):
    import i2v_native
    mma, env, kind = DEC_MODES[mode]
    monkeypatch.delenv("I2V_DEC_PW16", raising=False)
    _set_env(monkeypatch, env)
    name = config["name"]
    nf, ups, upt, _, _ = CONFIGS[name]
    sd = config["sd"]
    h = _handle(config, i2v_native.parse_mma(mma))
    lv = du.levels(ups, upt)
    bad = []
    x0 = _tap(h, config, 0, 12, DEC_B * 16 * 16 * nf).view(DEC_B, 1, 4, 4, 16 * nf)
    ref, bound = dr.fc_ref(config["z"], sd["fc.weight"], sd["fc.bias"], nf)
    f = _note("fc", dr.within(x0, ref, bound))
    out = [f"fc {f:.3f}"]
    if not f <= 1.0:
        bad.append(f"fc {f:.3g}")
    for k in range(6):
        n_in, n_out = du.CIN[k] * nf, du.COUT[k] * nf
        if n_in == n_out:
            continue
        T, H, W, ut, us = lv[k]
        P = (T // ut) * (H // us) * (W // us)
        x = _tap(h, config, k, 12, DEC_B * P * n_in).view(DEC_B * P, n_in)
        cs = _tap(h, config, k, 11, DEC_B * n_in * 2).view(DEC_B, n_in, 2)
        got = _tap(h, config, k, 4, DEC_B * P * n_out).view(DEC_B * P, n_out)
        w = du.sn_weight64(sd, du.NAMES[k] + ".conv_s").view(n_out, n_in).cuda()
        ref, S, S1, SW = dr.pw_ref(x, w, None, None, cs, P, False)
        f = _note("shortcut_" + kind, dr.within(got, ref, dr.pw_bound(kind, n_in, w, S, S1, SW, True, wround=1)))
        out.append(f"{du.NAMES[k]} {n_in}->{n_out} {f:.3f}")
        LEDGER.add(("shortcut", kind, (n_out + 31) // 32 * 32, n_out % 32 != 0))
        if not f <= 1.0:
            bad.append(f"{du.NAMES[k]} shortcut {f:.3g}")
    assert h.status() == 0, (name, mode)
    RAN.add((name, mode))
    print(f"DECREST {name} {mode} ({kind}): " + ", ".join(out))
    assert not bad, (name, mode, bad)


# ------------------------------------------------------------------------------------------------------ SPADE's branch
SPADE_MODES = {"mma1": (1, {}), "mma1_f23": (1, {"I2V_DEC_WINO4": "0"}), "mma1_direct": (1, {"I2V_DEC_SPW": "0"}), "mma0": (0, {}), "fp16": ("fp16", {})}
SPADE_RAN = set()


@pytest.mark.parametrize("mode", list(SPADE_MODES))
def test_spade_branch_units_vs_fp64(config, mode, monkeypatch):
    import i2v_native
    mma, env = SPADE_MODES[mode]
    monkeypatch.delenv("I2V_DEC_SPW", raising=False)
    monkeypatch.delenv("I2V_DEC_PW16", raising=False)
    _set_env(monkeypatch, env)
    name = config["name"]
    nf, ups, upt, (ih, iw), _ = CONFIGS[name]
    sd = config["sd"]
    h = _handle(config, i2v_native.parse_mma(mma))
    # the start frames 24 floats further apart than dense: the branch reads them through the sample stride
    buf = torch.full((DEC_B, 3 * ih * iw + 24), float("nan"), device="cuda")
    buf[:, :3 * ih * iw] = config["img"].reshape(DEC_B, -1)
    cfg = dict(config, img=buf[:, :3 * ih * iw].view(DEC_B, 3, ih, iw))
    assert cfg["img"].stride(0) == 3 * ih * iw + 24
    h.forward(cfg["img"], cfg["z"])
    forms = h.spade_forms()
    lv = du.levels(ups, upt)
    bad, out = [], []

    def note(key, f, what):
        _note(key, f)
        if not f <= 1.0:
            bad.append(f"{what} {key} {f:.3g}")
    for k in range(6):
        form = forms[k]
        _, H, W, _, _ = lv[k]
        C = du.CIN[k] * nf
        split = form != "f32"
        F_ = DEC_B
        w1, b1, wgb, bgb = dr.spade_weights(sd, du.NAMES[k], "cuda")
        # resize
        raw = _tap(h, cfg, k, 13, F_ * H * W * 16)
        y0 = du.decode_operand("hl16" if split else "f32", raw, F_, 1, H, W, 16)
        ref, bound = dr.resize_ref(config["img"], H, W, split)
        assert int((y0[..., 3:] != 0).sum()) == 0, (name, mode, k, "channels 3 .. 15")
        note("resize_" + ("hl16" if split else "f32"), dr.within(y0, ref, bound), du.NAMES[k])
        # Conv2d(3, 128) + lrelu from the rows
        kind1 = "hl16" if split else "f32"
        raw = _tap(h, cfg, k, 14, F_ * H * W * 128)
        y1 = du.decode_operand("hl16" if form == "hl16" else "f32", raw, F_, 1, H, W, 128)
        ref, S, S1 = du.conv_ref(kind1, y0, w1, b1, None, 1, 1, True, False)
        bound = du.conv_bound(kind1, 16 if split else 3, False, w1, S, S1, kt=1)
        if form == "hl16":
            bound = dr.stored_hl16(ref, bound)
        note("spade_conv1_" + kind1 + ("_stored" if form == "hl16" else ""), dr.within(y1, ref, bound), du.NAMES[k])
        # the Winograd operand from the activation
        opnd = y1
        if form in ("f43", "f23"):
            raw = _tap(h, cfg, k, 15, du.operand_floats(form, F_, 1, H, W, 128))
            opnd = du.decode_operand(form, raw, F_, 1, H, W, 128)
            ref, S = du.writer_ref(form, y1, None, None, 1, 1)
            note("spade_writer_" + form, dr.within(opnd, ref, du.writer_bound(form, ref, S)), du.NAMES[k])
        # gamma | beta from its operand
        gb = _tap(h, cfg, k, 0, F_ * H * W * 2 * C).view(F_, 1, H, W, 2 * C)
        ref, S, S1 = du.conv_ref(form, opnd, wgb, bgb, None, 1, 1, False, False)
        note("spade_gb_" + form, dr.within(gb, ref, du.conv_bound(form, 128, False, wgb, S, S1, kt=1)), du.NAMES[k])
        LEDGER.add(("spade", form, "fine" if H <= 8 else "coarse" if H >= 64 else "mid"))
        out.append(f"{du.NAMES[k]} {H}x{W} {form}")
        del raw, y0, y1, opnd, gb, ref, S, S1, bound
    assert h.status() == 0, (name, mode)
    assert h.spade_forms() == forms, "the tapped forwards took the same forms"
    SPADE_RAN.add((name, mode))
    print(f"DECREST spade {name} {mode}: " + ", ".join(out))
    assert not bad, (name, mode, bad)


# ------------------------------------------------------------------------------------------------------ ledger
def test_ledger_every_form_ran():
    assert len(RAN) == len(DEC_CONFIGS) * len(DEC_MODES), "the ledger needs the whole module to have run"
    print("DECREST ledger:", sorted(map(str, LEDGER)))
    for form in dr.FORMS:
        assert ("form", form) in LEDGER, form
    for want in ("mfma", "valu", "generic"):
        assert ("auto", want) in LEDGER, want
    assert {("ks", k) for k in (1, 2, 3, 4)} <= LEDGER
    assert ("tch", 1) in LEDGER and ("tch", 2) in LEDGER, "the production rule's one and two frames per workgroup"
    assert {("tch_forced", t) for t in (1, 2, 4, 8, 16)} <= LEDGER
    for kind in ("hl16", "f32"):
        for tile in (128, 64, 32):
            for affine in (False, True):
                for epi in (False, True):
                    assert ("pw", kind, tile, affine, epi) in LEDGER, (kind, tile, affine, epi)
        assert any(e[:2] == ("shortcut", kind) for e in LEDGER if isinstance(e, tuple)), kind
    assert ("pw", "hl16", "transposed", False, False) in LEDGER and ("pw", "hl16", "transposed", False, True) in LEDGER
    pads = {e[2] for e in LEDGER if isinstance(e, tuple) and e[:2] == ("shortcut", "hl16")}
    assert {32, 64, 96, 128} <= pads, pads                               # Cout rounded up to 32: nf 8, 16, 24 (-> 128 in the packer), 40
    assert any(e[0] == "shortcut" and e[3] for e in LEDGER if isinstance(e, tuple)), "a ragged Cout (24 / 80)"
    # SPADE's branch: every form at a level of 64 x 64 or larger; the direct and the fp32 form at the 4 x 4 / 8 x 8 levels as well.  The
    # Winograd forms cannot run there: at T = 1 their bricks are 32 rows high (wino4_tiling / wino16_tiling want H % 32 == 0).
    assert len(SPADE_RAN) == len(DEC_CONFIGS) * len(SPADE_MODES), "the ledger needs the whole module to have run"
    for form in ("f43", "f23", "hl16", "f32"):
        assert ("spade", form, "coarse") in LEDGER, form
    for form in ("hl16", "f32"):
        assert ("spade", form, "fine") in LEDGER, form
    for form in ("f43", "f23"):
        assert ("spade", form, "fine") not in LEDGER, form
