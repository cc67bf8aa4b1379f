"""CPU checks of tests/dec_rest_common.py, the gate of tests/test_gpu_dec_rest.py (the pattern of tests/test_host_dec_units.py):

  * every new reference agrees with the torch float64 op it stands for (conv3d + tanh in the frame layout, linear with the affine
    folded into the input, the fc view), and the extended dec_units_common.conv_ref with one temporal tap agrees with conv2d;
  * an fp32 emulation of every unit in every form (operands split where the kernel splits them) stays at <= 0.5 of the derived bound
    (SPADE's units that store split-fp16 values: <= 1, see there);
  * every named mutation exceeds the gate on every case it applies to (smallest factor printed: profiles/dec_rest_gate.md);
  * the inputs keep the comparisons whole: no element is excluded anywhere, and fewer than 1 % of conv_img's reference outputs are
    saturated (|tanh| > 0.99) while the pre-activations still span +-3.

Also: the new entries are declared, exported and refuse host tensors."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dec_rest_common as dr
import dec_units_common as du

torch.set_grad_enabled(False)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (form, C, (B, T, H, W))
IMG_CASES = [("mfma", 16, (1, 3, 8, 32)), ("mfma", 48, (2, 2, 8, 32)), ("gemm", 64, (1, 3, 7, 9)), ("gemm", 68, (2, 2, 5, 6)),
             ("valu", 12, (1, 8, 8, 8)), ("valu", 40, (2, 8, 8, 8)), ("generic", 8, (1, 3, 7, 9))]
# (kind, M, P, Cin, Cout, affine, res, lrelu)
PW_CASES = [("hl16", 300, 130, 12, 24, True, True, True), ("hl16", 300, 130, 12, 24, False, False, False), ("hl16", 517, 200, 36, 64, True, False, True),
            ("hl16", 261, 100, 32, 128, True, True, False), ("hl16", 133, 133, 64, 81, False, False, False),
            ("f32", 300, 130, 12, 24, True, True, True), ("f32", 517, 200, 36, 64, True, False, False), ("f32", 261, 100, 32, 128, False, True, True)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _img_run(case, seed, mutate=None):
    form, C, (B, T, H, W) = case
    x, w, bias = dr.conv_img_inputs(B, T, H, W, C, seed)
    ref, S, S1, SW = dr.conv_img_ref(x, w, bias)
    got = dr.conv_img_emulate(form, x, w, bias, mutate)
    return dr.within(got, ref, dr.conv_img_bound(form, C, w, ref, S, S1, SW), rel=0.0)


def _pw_run(case, seed, mutate=None):
    kind, M, P, Cin, Cout, affine, res, lrelu = case
    x, w, b, coef, r = dr.pw_inputs(M, P, Cin, Cout, seed, affine, res)
    ref, S, S1, SW = dr.pw_ref(x, w, b, r, coef, P, lrelu)
    got = dr.pw_emulate(kind, x, w, b, r, coef, P, lrelu, mutate)
    return dr.within(got, ref, dr.pw_bound(kind, Cin, w, S, S1, SW, affine))


# ------------------------------------------------------------------------------------------------------ references vs torch float64
@pytest.mark.parametrize("case", IMG_CASES, ids=str)
def test_conv_img_reference_is_conv3d_tanh_in_frames(case):
    form, C, (B, T, H, W) = case
    x, w, bias = dr.conv_img_inputs(B, T, H, W, C, 7)
    ref, S, S1, SW = dr.conv_img_ref(x, w, bias)
    pre = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.double(), bias.double(), padding=1)      # [B, 3, T, H, W]
    want = torch.tanh(pre).permute(0, 2, 1, 3, 4)
    assert ref.shape == (B, T, 3, H, W) and float((ref - want).abs().max()) < 1e-13
    s_want = F.conv3d(x.double().abs().permute(0, 4, 1, 2, 3), w.double().abs(), bias.double().abs(), padding=1).permute(0, 2, 1, 3, 4)
    assert float((S - s_want).abs().max()) < 1e-12
    sw_want = F.conv3d(torch.ones(B, C, T, H, W, dtype=torch.float64), w.double().abs(), None, padding=1).permute(0, 2, 1, 3, 4)
    assert float((SW - sw_want).abs().max()) < 1e-12
    # the inputs: pre-activations span +-3, fewer than 1 % saturated outputs, nothing excluded from the comparison
    assert float(pre.abs().max()) > 2.0 and dr.saturated_share(ref) < 0.01, (float(pre.abs().max()), dr.saturated_share(ref))
    bound = dr.conv_img_bound(form, C, w, ref, S, S1, SW)
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())


@pytest.mark.parametrize("case", PW_CASES, ids=str)
def test_pointwise_reference_is_linear_of_the_normalised_input(case):
    kind, M, P, Cin, Cout, affine, res, lrelu = case
    x, w, b, coef, r = dr.pw_inputs(M, P, Cin, Cout, 11, affine, res)
    ref, S, S1, SW = dr.pw_ref(x, w, b, r, coef, P, lrelu)
    xa = x.double()
    if affine:
        rows = torch.arange(M) // P
        assert int(rows.max()) >= 1 and (P % 128 != 0)           # a 128-row tile straddles two samples' coefficient rows
        xa = xa * coef[rows, :, 0].double() + coef[rows, :, 1].double()
    want = F.linear(xa, w.double(), b.double())
    if res:
        want = want + r.double()
    if lrelu:
        want = F.leaky_relu(want, 0.2)
    assert float((ref - want).abs().max()) < 1e-12
    assert bool((dr.pw_bound(kind, Cin, w, S, S1, SW, affine) > 0).all())


def test_fc_reference_is_the_linear_layer_viewed_channels_last():
    nf, zd, B = 8, 64, 3
    g = torch.Generator().manual_seed(3)
    z, w, b = torch.randn(B, zd, generator=g), torch.randn(16 * nf * 16, zd, generator=g) / 8, torch.randn(16 * nf * 16, generator=g)
    ref, bound = dr.fc_ref(z, w, b, nf)
    want = F.linear(z.double(), w.double(), b.double()).view(B, 16 * nf, 1, 4, 4).permute(0, 2, 3, 4, 1)
    assert ref.shape == (B, 1, 4, 4, 16 * nf) and float((ref - want).abs().max()) < 1e-13
    emu = F.linear(z, w, b).view(B, 16 * nf, 1, 4, 4).permute(0, 2, 3, 4, 1)
    assert dr.within(emu, ref, bound) <= 0.5
    assert dr.within(emu.roll(1, 4), ref, bound) > 1.0            # channels-first order read as channels-last


def test_conv_ref_with_one_temporal_tap_is_conv2d():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 6, 8, 16, generator=g)
    w = torch.randn(24, 16, 1, 3, 3, generator=g).double() / 12
    bias = torch.randn(24, generator=g).double()
    ref, S, S1 = du.conv_ref("f32", x.double(), w, bias, None, 1, 1, True, False)
    want = F.leaky_relu(F.conv2d(x[:, 0].double().permute(0, 3, 1, 2), w[:, :, 0], bias, padding=1), 0.2).permute(0, 2, 3, 1)
    assert float((ref[:, 0] - want).abs().max()) < 1e-12
    assert du.conv_chain("hl16", 128, False, kt=1) == 16 * 9 * 3 + 24 and du.conv_chain("hl16", 128, False) == 16 * 27 * 3 + 24
    assert du.conv_chain("f32", 16, False, kt=1) == 8 * 9 + 10 and du.conv_chain("f43", 128, False, kt=1) == 16 * 9 + 24


# ------------------------------------------------------------------------------------------------------ emulation and mutations
def test_fp32_emulation_of_conv_img_stays_at_half_the_bound():
    worst = {}
    for i, case in enumerate(IMG_CASES):
        f = _img_run(case, 200 + i)
        worst[case[0]] = max(worst.get(case[0], 0.0), f)
        assert f <= 0.5, (case, f)
    print("DECREST host conv_img: worst CPU fp32 |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_fp32_emulation_of_the_pointwise_gemm_stays_at_half_the_bound():
    worst = {}
    for i, case in enumerate(PW_CASES):
        f = _pw_run(case, 300 + i)
        worst[case[0]] = max(worst.get(case[0], 0.0), f)
        assert f <= 0.5, (case, f)
    print("DECREST host pointwise: worst CPU fp32 |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _applies(mutation, unit, case):
    if unit == "img":
        return {"tap_order_reversed": case[2][1] > 1, "frames_b3t": case[2][1] > 1, "tanh_omitted": True,
                "lo_dropped": case[0] in dr.SPLIT_FORMS}.get(mutation, False)
    return {"lo_dropped": case[0] == "hl16", "affine_after_gemm": case[5], "coef_row_neighbour": case[5],
            "lrelu_slope_001": case[7]}.get(mutation, False)


@pytest.mark.parametrize("mutation", dr.MUTATIONS)
def test_mutation_exceeds_the_gate(mutation):
    factors = []
    for unit, cases, run in (("img", IMG_CASES, _img_run), ("pw", PW_CASES, _pw_run)):
        for i, case in enumerate(cases):
            if _applies(mutation, unit, case):
                f = run(case, 400 + i, mutate=mutation)
                factors.append(f)
                assert f > 1.0, (mutation, unit, case, f)
    assert len(factors) >= 2, mutation
    print(f"DECREST mutation {mutation}: smallest |err| / bound over {len(factors)} cases {min(factors):.1f}")


# ------------------------------------------------------------------------------------------------------ SPADE's branch
# (form of the gamma | beta conv, C of the block, start frame (h, w), level (H, W))
SPADE_CASES = [("f43", 32, (48, 80), (32, 32)), ("f23", 16, (64, 64), (32, 16)), ("hl16", 24, (48, 80), (4, 4)), ("f32", 24, (64, 64), (8, 8)),
               ("hl16", 8, (20, 12), (16, 16))]


def _spade_sd(C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"b.norm_0.conv.weight": r(128, 3, 3, 3) / 27 ** 0.5, "b.norm_0.conv.bias": 0.1 * r(128),
            "b.norm_0.conv_gamma.weight": r(C, 128, 3, 3) / 1152 ** 0.5, "b.norm_0.conv_gamma.bias": 0.1 * r(C),
            "b.norm_0.conv_beta.weight": r(C, 128, 3, 3) / 1152 ** 0.5, "b.norm_0.conv_beta.bias": 0.1 * r(C)}


def _writer43_as_the_kernel(y1):
    """B^T d of F(4,3) with modulate_wino4_kernel's expressions (csrc/i2v_dec_writers.hip: at most three roundings per value), fp32."""
    t = F.pad(y1.float(), (0, 0, 1, 1)).unfold(3, 6, 4)                     # [B, 1, H, J, C, 6]
    d = [t[..., i] for i in range(6)]
    fma = lambda a, x, c: (a * x.double() + c.double()).float()
    return torch.stack([fma(4.0, d[0], fma(-5.0, d[2], d[4])), fma(-4.0, d[1] + d[2], d[3] + d[4]), fma(4.0, d[1] - d[2], d[4] - d[3]),
                        fma(2.0, d[3] - d[1], d[4] - d[2]), fma(2.0, d[1] - d[3], d[4] - d[2]), fma(4.0, d[1], fma(-5.0, d[3], d[5]))], 2)


def _spade_run(case, seed, mutate=None):
    """The four units of the branch in the case's form, each emulated in fp32 from the (format-rounded) output of the unit in front of it
    -> {unit: |err| / bound}."""
    form, C, (ih, iw), (H, W) = case
    split = form != "f32"
    sd = _spade_sd(C, seed)
    img = 2 * torch.rand(2, 3, ih, iw, generator=_g(seed + 1)) - 1
    w1, b1, wgb, bgb = dr.spade_weights(sd, "b")
    out = {}
    store = lambda kind, v: du.decode_operand(kind, du.encode_operand(kind, v), 2, 1, H, W, v.shape[-1])
    ref, bound = dr.resize_ref(img, H, W, split)
    emu, _ = dr.resize_ref(img, H, W, split, dtype=torch.float32, mutate=mutate)
    y0 = store("hl16" if split else "f32", emu)
    assert int((y0[..., 3:] != 0).sum()) == 0
    out["resize"] = dr.within(y0, ref, bound)
    kind1 = "hl16" if split else "f32"
    ref, S, S1 = du.conv_ref(kind1, y0, w1, b1, None, 1, 1, True, False)
    bound = du.conv_bound(kind1, 16 if split else 3, False, w1, S, S1, kt=1)
    emu = du.conv_ref(kind1, y0, w1, b1, None, 1, 1, False, False, dtype=torch.float32)[0]
    emu = torch.where(emu >= 0, emu, (0.01 if mutate == "lrelu_slope_001" else 0.2) * emu)
    if form == "hl16":
        bound = dr.stored_hl16(ref, bound)
    y1 = store("hl16" if form == "hl16" else "f32", emu)
    out["conv1"] = dr.within(y1, ref, bound)
    opnd = y1
    if form in du.PLANES:
        ref, S = du.writer_ref(form, y1, None, None, 1, 1)
        emu = _writer43_as_the_kernel(y1) if form == "f43" else du.writer_ref(form, y1, None, None, 1, 1, dtype=torch.float32)[0]
        opnd = du.decode_operand(form, du.encode_operand(form, emu), 2, 1, H, W, 128)
        out["writer"] = dr.within(opnd, ref, du.writer_bound(form, ref, S))
    ref, S, S1 = du.conv_ref(form, opnd, wgb, bgb, None, 1, 1, False, False)
    bias = bgb.clone()
    if mutate == "gamma_bias_without_one":
        bias[:C] -= 1.0
    emu = du.conv_ref(form, opnd, wgb, bias, None, 1, 1, False, False, dtype=torch.float32)[0]
    if mutate == "gamma_beta_swapped":
        emu = emu.roll(C, -1)
    out["gb"] = dr.within(emu, ref, du.conv_bound(form, 128, False, wgb, S, S1, kt=1))
    return out


def test_spade_references_are_the_torch_ops():
    form, C, (ih, iw), (H, W) = SPADE_CASES[0]
    sd = _spade_sd(C, 9)
    img = 2 * torch.rand(2, 3, ih, iw, generator=_g(10)) - 1
    for size in ((4, 4), (32, 32), (128, 128), (ih, iw)):
        ref, bound = dr.resize_ref(img, *size, False)
        want = F.interpolate(img.double(), size, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        assert ref.shape == (2, 1, *size, 16) and float((ref[:, 0, :, :, :3] - want).abs().max()) < 1e-14 and float(ref[..., 3:].abs().max()) == 0
    w1, b1, wgb, bgb = dr.spade_weights(sd, "b")
    p = "b.norm_0."
    y0 = dr.resize_ref(img, H, W, False)[0]
    y1 = du.conv_ref("f32", y0, w1, b1, None, 1, 1, True, False)[0]
    want1 = F.leaky_relu(F.conv2d(y0[:, 0, :, :, :3].permute(0, 3, 1, 2), sd[p + "conv.weight"].double(), sd[p + "conv.bias"].double(), padding=1), 0.2)
    assert float((y1[:, 0] - want1.permute(0, 2, 3, 1)).abs().max()) < 1e-12
    gamma = F.conv2d(want1, sd[p + "conv_gamma.weight"].double(), sd[p + "conv_gamma.bias"].double(), padding=1)
    beta = F.conv2d(want1, sd[p + "conv_beta.weight"].double(), sd[p + "conv_beta.bias"].double(), padding=1)
    want = torch.cat((1 + gamma, beta), 1).permute(0, 2, 3, 1)            # normalized * (1 + gamma) + beta (normalization_layer.py:20-23)
    for kind in ("f32", "f43", "f23"):
        opnd = y1 if kind == "f32" else du.writer_ref(kind, y1, None, None, 1, 1)[0]
        gb = du.conv_ref(kind, opnd, wgb, bgb, None, 1, 1, False, False)[0]
        assert float((gb[:, 0] - want).abs().max()) < 1e-11, kind


def test_fp32_emulation_of_the_spade_units_stays_at_half_the_bound():
    worst = {}
    for i, case in enumerate(SPADE_CASES):
        for unit, f in _spade_run(case, 500 + i).items():
            key = f"{unit}_{case[0]}"
            worst[key] = max(worst.get(key, 0.0), f)
            # (a unit whose output is STORED in the split-fp16 format: where the value is close to zero nothing is left of the bound but
            #  the format's 2^-25, the exact worst case of rounding the lo part to an fp16 subnormal -- correct code attains it: <= 1)
            stored = unit == "writer" or (unit == "resize" and case[0] != "f32") or (unit == "conv1" and case[0] == "hl16")
            assert f <= (1.0 if stored else 0.5), (case, unit, f)
    print("DECREST host spade: worst CPU fp32 |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("mutation", dr.SPADE_MUTATIONS)
def test_spade_mutation_exceeds_the_gate(mutation):
    unit = {"align_corners_false": "resize", "gamma_bias_without_one": "gb", "gamma_beta_swapped": "gb", "lrelu_slope_001": "conv1"}[mutation]
    factors = []
    for i, case in enumerate(SPADE_CASES):
        if mutation == "align_corners_false" and case[2] == case[3]:
            continue
        f = _spade_run(case, 600 + i, mutate=mutation)[unit]
        factors.append(f)
        assert f > 1.0, (mutation, case, f)
    assert len(factors) >= 2, mutation
    print(f"DECREST mutation {mutation}: smallest |err| / bound over {len(factors)} cases {min(factors):.1f}")


# ------------------------------------------------------------------------------------------------------ the entries
def test_unit_entries_are_declared_exported_and_refuse_host_tensors():
    import i2v_native
    hdr = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    lib = i2v_native.lib()
    assert "#define I2V_DEC_TAP_LAST 15" in hdr and i2v_native.NativeDecoder.SPADE_FORMS == ("f43", "f23", "hl16", "f32")
    for name in ("i2v_conv_img_unit", "i2v_pointwise_unit", "i2v_dec_get_spade_form"):
        assert re.search(r"\b%s\(" % name, hdr) and name in i2v_native.SYMBOLS and hasattr(lib, name), name
    assert i2v_native.CONV_IMG_FORMS == dr.FORMS
    x, w, bias = dr.conv_img_inputs(1, 1, 8, 8, 8, 1)
    with pytest.raises(i2v_native.I2VError):
        i2v_native.conv_img_unit(x, w, bias)
    with pytest.raises(i2v_native.I2VError):
        i2v_native.pointwise_unit(torch.zeros(4, 8), torch.zeros(8, 8))
