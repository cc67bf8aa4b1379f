"""CPU checks of tests/dec_units_common.py, the gate of tests/test_gpu_dec_units.py:

  * every layout decoder inverts its encoder on random data at ragged channel counts (the one-term format's padding channels included);
  * a plain fp32 torch emulation of every unit (the same expressions in float32, through the operand formats) stays at <= 0.5 of the
    unit's derived bound against the float64 reference -- the bound is reachable by correct fp32 code;
  * every named mutation of that emulation exceeds the gate on every case it applies to -- the bound is not vacuous.  The smallest
    factor per mutation is printed (run with -s; recorded in profiles/dec_units_gate.md).

The cases are the unit shapes of the GPU test's configurations (nf24_p11, nf8_s4, nf16_t4: ragged 24 / 48 / 96 channels, x2 / x4
nearest maps in time and space, temporal-duplication pairs, learned and identity residuals, lrelu on the last block) on maps small
enough for the CPU."""
import pytest
import torch

import dec_units_common as du

torch.set_grad_enabled(False)


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("kind,C", [("f32", 24), ("hl16", 24), ("hl16", 40), ("f23", 32), ("f23", 96), ("f43", 96), ("f43", 160),
                                    ("f43_f32", 24), ("f43_one", 96), ("f43_one", 32), ("f43_one", 128)])
def test_layout_decoder_inverts_encoder(kind, C):
    B, T, H, W = 2, 3, 4, 16
    P = du.PLANES.get(kind)
    shape = (B, T, H, W, C) if not P else (B, T, P, H, W // (2 if P == 4 else 4), C)
    v = torch.randn(shape, generator=_g(C)) * torch.rand(shape, generator=_g(C + 1)) * 8
    raw = du.encode_operand(kind, v)
    assert raw.dtype == torch.float32 and raw.numel() == du.operand_floats(kind, B, T, H, W, C)
    got = du.decode_operand(kind, raw, B, T, H, W, C)
    if kind in ("f32", "f43_f32"):
        assert torch.equal(got, v.double())
    elif kind == "f43_one":
        assert torch.equal(got, v.half().double())
        vals, padc = du.decode_operand(kind, raw, B, T, H, W, C, parts=True)
        assert padc.shape[-1] == du.pad64(C) - C and int((padc != 0).sum()) == 0
        # a marker in every padding channel comes back in the padding part only
        Cp = du.pad64(C)
        if Cp > C:
            full = torch.cat((v, torch.full(shape[:-1] + (Cp - C,), 3.0)), -1)
            vals2, pad2 = du.decode_operand(kind, du.encode_operand(kind, full), B, T, H, W, Cp, parts=True)
            assert torch.equal(vals2[..., :C], vals) and bool((vals2[..., C:] == 3.0).all())
    else:
        hi, lo = du.decode_operand(kind, raw, B, T, H, W, C, parts=True)
        eh, el = du.split16(v)
        assert torch.equal(hi, eh.double()) and torch.equal(lo, el.double()) and torch.equal(got, hi + lo)
        assert float((got - v.double()).abs().max()) <= 2.0 ** -22 * float(v.abs().max()) + 2.0 ** -25


def test_split_hi_view_matches_the_decoder():
    B, T, H, W, C = 1, 2, 4, 16, 32
    v = torch.randn(B, T, 6, H, W // 4, C, generator=_g(3))
    raw = du.encode_operand("f43", v)
    nrows = raw.numel() // 16
    hi = du._v_split_hi(raw, B, T, C, H, W // 4, nrows).view(B, T, C // 16, 6, H, W // 4, 16)
    ref = du.decode_operand("f43", raw, B, T, H, W, C, parts=True)[0]
    assert torch.equal(hi.permute(0, 1, 3, 4, 5, 2, 6).reshape(ref.shape).double(), ref)


# ------------------------------------------------------------------------------------------------------ unit cases
# writer: (kind, C, (Tl, Hl, Wl), ut, us, with SPADE maps)
WRITER_CASES = [("f32", 24, (2, 2, 4), 4, 1, True), ("f32", 24, (2, 4, 4), 1, 1, False), ("hl16", 24, (2, 4, 4), 1, 1, True),
                ("hl16", 48, (2, 2, 2), 1, 2, True), ("hl16", 8, (2, 2, 2), 2, 4, True), ("f23", 32, (2, 4, 16), 1, 2, True),
                ("f23", 96, (2, 4, 8), 1, 1, False), ("f43", 96, (1, 2, 4), 4, 4, True), ("f43", 32, (2, 2, 72), 1, 1, False),
                ("f43", 192, (2, 4, 8), 1, 2, True), ("f43_one", 96, (2, 4, 8), 1, 2, True), ("f43_one", 32, (1, 4, 4), 2, 4, False),
                ("f43_f32", 24, (2, 2, 4), 1, 4, True), ("f43_f32", 48, (2, 4, 8), 4, 1, False)]
# conv: (kind, cin, cout, (T, H, W), tdup, residual (rt, rs) or None, lrelu)
CONV_CASES = [("f32", 24, 24, (2, 4, 4), False, (1, 1), False), ("f32", 48, 24, (8, 4, 4), False, (4, 1), True),
              ("hl16", 48, 24, (2, 4, 4), False, None, False), ("hl16", 16, 8, (4, 4, 4), True, None, False),
              ("hl16", 24, 24, (2, 8, 8), False, (1, 4), True), ("hl16", 384, 384, (1, 4, 4), False, (1, 1), False),
              ("f23", 32, 48, (2, 8, 8), False, (2, 2), False), ("f23", 32, 16, (4, 4, 8), True, None, False),
              ("f43", 96, 48, (8, 4, 8), False, (4, 1), False), ("f43", 32, 32, (4, 4, 16), True, None, False),
              ("f43", 192, 96, (2, 4, 8), False, (2, 2), True), ("f43_one", 96, 48, (4, 4, 8), True, None, False),
              ("f43_one", 32, 24, (2, 4, 8), False, (1, 2), True), ("f43_f32", 24, 12, (4, 8, 8), False, (4, 4), True),
              ("f43_f32", 48, 48, (2, 4, 8), False, (1, 1), False)]
STATS_CASES = [(24, (2, 4, 4)), (80, (2, 8, 8)), (48, (4, 4, 8)), (8, (16, 16, 16))]
# coef: (kind, C, groups, count)
COEF_CASES = [("spade", 24, 12, 64), ("spade", 40, 10, 16), ("spade", 384, 16, 16), ("gn", 48, 16, 256), ("gn", 16, 16, 4096),
              ("adain", 24, 24, 128), ("adain", 80, 80, 16), ("adain", 8, 8, 4096)]


def _writer_inputs(case, seed):
    kind, C, (Tl, Hl, Wl), ut, us, with_gb = case
    g = _g(seed)
    x = torch.randn(2, Tl, Hl, Wl, C, generator=g) * 1.5 + 0.3
    coef = torch.stack((0.5 + torch.rand(2, C, generator=g), torch.randn(2, C, generator=g) * 0.5), 2)
    gb = torch.cat((1 + 0.3 * torch.randn(2, Hl * us, Wl * us, C, generator=g), 0.3 * torch.randn(2, Hl * us, Wl * us, C, generator=g)), 3) if with_gb else None
    return x, coef, gb


def _writer_run(case, seed, mutate=None):
    kind, C, (Tl, Hl, Wl), ut, us, _ = case
    x, coef, gb = _writer_inputs(case, seed)
    ref, S = du.writer_ref(kind, x, coef, gb, ut, us)
    emu, _ = du.writer_ref(kind, x, coef, gb, ut, us, dtype=torch.float32, mutate=None if mutate == "lo_dropped_plane" else mutate)
    raw = du.encode_operand(kind, emu, drop_lo_plane=1 if mutate == "lo_dropped_plane" else None)
    got = du.decode_operand(kind, raw, 2, Tl * ut, Hl * us, Wl * us, C)
    return du.within(got, ref, du.writer_bound(kind, ref, S))


def _conv_run(case, seed, mutate=None):
    kind, cin, cout, (T, H, W), tdup, res, lrelu = case
    g = _g(seed)
    Ti = T // 2 if tdup else T
    P = du.PLANES.get(kind)
    d = torch.randn(2, Ti, H, W, cin, generator=g)
    if P:   # a V tensor as a writer forms it: B^T of an activation map, in the format's precision
        d, _ = du.writer_ref(kind, d, torch.stack((torch.ones(2, cin), torch.zeros(2, cin)), 2), None, 1, 1, dtype=torch.float32)
    opnd = du.decode_operand(kind, du.encode_operand(kind, d), 2, Ti, H, W, cin)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g).float().double() / (27 * cin) ** 0.5
    bias = torch.randn(cout, generator=g).float().double() * 0.1
    r = None
    if res:
        r = torch.randn(2, T // res[0], H // res[1], W // res[1], cout, generator=g).float().double()
    rt, rs = res or (1, 1)
    ref, S, S1 = du.conv_ref(kind, opnd, w, bias, r, rt, rs, lrelu, tdup)
    emu, _, _ = du.conv_ref(kind, opnd, w, bias, r, rt, rs, lrelu, tdup, dtype=torch.float32, mutate=mutate)
    assert ref.shape == (2, T, H, W, cout)
    return du.within(emu, ref, du.conv_bound(kind, cin, tdup, w, S, S1))


def _stats_run(case, seed, mutate=None):
    C, (T, H, W) = case
    x = torch.randn(2, T, H, W, C, generator=_g(seed)) + 0.25
    ref, bound = du.stats_ref(x)
    return du.within(du.stats_emulate(x, mutate), ref, bound, rel=du.U64)


def _coef_run(case, seed, mutate=None):
    kind, C, groups, count = case
    g = _g(seed)
    x = torch.randn(2, count, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    sums, _ = du.stats_ref(x)
    adain = affine = None
    if kind == "adain":
        adain = (torch.randn(2, 64, generator=g), torch.randn(2 * C, 64, generator=g) / 8, torch.randn(2 * C, generator=g))
    if kind == "gn":
        affine = (1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g))
    ref, bound = du.coef_ref(sums, groups, count, adain, affine)
    emu, _ = du.coef_ref(sums, groups, count, adain, affine, mutate=mutate, dtype=torch.float32)
    return du.within(emu, ref, bound)


UNITS = {"writer": (WRITER_CASES, _writer_run), "conv": (CONV_CASES, _conv_run), "stats": (STATS_CASES, _stats_run),
         "coef": (COEF_CASES, _coef_run)}


@pytest.mark.parametrize("unit", list(UNITS))
def test_fp32_emulation_stays_at_half_the_bound(unit):
    cases, run = UNITS[unit]
    worst = {}
    for i, case in enumerate(cases):
        f = run(case, 100 + i)
        key = case[0] if isinstance(case[0], str) else "fp64"
        worst[key] = max(worst.get(key, 0.0), f)
        assert f <= 0.5, (unit, case, f)
    print(f"DECUNITS host {unit}: worst CPU fp32 |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _applies(mutation, unit, case):
    """The cases a mutation changes anything on."""
    wino = isinstance(case[0], str) and case[0] in du.PLANES
    if unit == "writer":
        return {"lo_dropped_plane": case[0] in ("f23", "f43"), "bt_row_sign": wino, "edge_from_neighbour_row": wino,
                "upsample_off_by_one": 4 in (case[3], case[4])}.get(mutation, False)
    if unit == "conv":
        return {"tdup_pairs_swapped": case[4], "bias_omitted": True, "residual_wrong_rate": bool(case[5]) and case[5] != (1, 1),
                "lrelu_omitted": case[6], "weight_plane_x2": wino}.get(mutation, False)
    if unit == "stats":
        return mutation in ("stats_without_last_tile", "stats_one_parity")
    return {"variance_unbiased": True, "group_totals_per_channel": case[1] // case[2] > 1, "adain_beta_offset": case[0] == "adain"}.get(mutation, False)


@pytest.mark.parametrize("mutation", du.MUTATIONS)
def test_mutation_exceeds_the_gate(mutation):
    factors = []
    for unit, (cases, run) in UNITS.items():
        for i, case in enumerate(cases):
            if _applies(mutation, unit, case):
                f = run(case, 100 + i, mutate=mutation)
                factors.append(f)
                assert f > 1.0, (mutation, unit, case, f)
    assert len(factors) >= 2, mutation
    print(f"DECUNITS mutation {mutation}: smallest |err| / bound over {len(factors)} cases {min(factors):.1f}")
