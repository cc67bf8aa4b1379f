"""Shared by tests/test_host_dec_units.py and tests/test_gpu_dec_units.py: the units of one GeneratorBlock of the stage-1 decoder --
statistics, coefficient tables, operand writers, 3x3x3 convs -- each with a layout decoder of what the GPU leaves in the debug taps
(include/i2v_hip.h, i2v_dec_debug_tap), a plain torch float64 reference computed FROM those taps, a bound derived from operation
counts and magnitudes, and named mutations that show what the gate catches.  No GPU code; imports without a GPU.

Layouts are written from the comments of csrc/i2v_dec_writers.hip, i2v_wino32.hip and i2v_wino_pack.h.  Decoded operands are
float64 [B, T, H, W, C] (direct) or [B, T, plane, H, J, C] (Winograd V, J = W / 2 or W / 4), hi + lo exact in float64.

Gate of every unit, element-wise:   |got - ref| <= bound + 2^-24 |ref|   (fp64 units: 2^-53 |ref|),   U = 2^-24

  stats    fp64 sums of fp32 values: gamma64(count + 8) * sum|x| (sum x^2: * sum x^2); the order (lanes, waves, atomics) is free.
  coef     computed in fp64, rounded to fp32 once (one fp32 step in all: the rounding attains half of it).  A = g rstd, B = b - g mean rstd.  The error of var = q/n - mean^2 in fp64
           ((cpg + 16) 2^-53 (q/n + mean^2)) goes through rstd' = rstd^3 / 2.  ADAIN: g | b come from an fp32 Linear(z_dim, 2C) on
           the fp32 matrix cores: gamma(z_dim + 2) * (sum |w||z| + |bias|) each, in any order.
  writer   d = lrelu(x a + b), a = A g' (1 rounding), b = fma(B, g', beta) (1), fma (1), 0.2 * (1), then B^T: at most 3 more
           (fma(-4, d1 + d2, d3 + d4)): gamma(7) * sum_k |B^T_pk| (|x||A||g'| + |B||g'| + |beta|).  Split operand: + 2^-22 |V| (the lo
           part's rounding) + 2^-25 (half an fp16 subnormal step).  One-term operand: ONE fp16 step, 2^-10 |V| + 2^-24 -- the single
           rounding to fp16 attains half a step in correct code, and the host test wants correct code at <= 0.5 of the bound.
  conv     S = sum |A^T| * (sum |U||V|) + |bias| + |residual|.  n = the accumulation chain: MFMA k-steps (8 channels per fp16 step
           and 3 steps per product in the split kernels, 16 and 1 in the one-term kernel, 2 channels in fp32) x taps, + 16 for the
           sum inside one instruction, + 8 for split-K partials / the output transform / bias, residual, lrelu.  Weights: rounded to
           fp32 once (2^-24; the direct tdup packer twice), split hi + lo (2^-22 + 2^-25 2^-wexp per |V|), the lo * lo product the
           split kernels leave out (2^-22).  One-term: the packer's fp16 rounding is emulated, no term -- as the library is built the
           value goes from fp64 to fp16 in ONE rounding ("rounded to fp16 once", i2v_wino_pack.h: the compiler folds the packer's
           (float) step into the conversion), not fp16(fp32(.)): the two differ in ~2^-15 of the weights by one fp16 step, which
           this bound sees (profiles/dec_units_gate.md).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
U64 = 2.0 ** -53
K_F32, K_F16, K_F23, K_F43, K_F43_GEN, K_F32_WINO, K_F43_ONE = range(7)
KERNELS = {K_F32: "f32", K_F16: "hl16", K_F23: "f23", K_F43: "f43", K_F32_WINO: "f43_f32", K_F43_ONE: "f43_one"}
SPLIT = ("hl16", "f23", "f43", "f43_one")          # formats read by the split-fp16 / one-term kernels (is_split in i2v_dec_block.h)
PLANES = {"f23": 4, "f43": 6, "f43_f32": 6, "f43_one": 6}
CIN = (16, 16, 16, 8, 4, 2)
COUT = (16, 16, 8, 4, 2, 1)
NAMES = ("head_0", "g_0", "g_1", "g_2", "g_3", "g_4")

BT = {4: torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64),
      6: torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                       [0, 4, 0, -5, 0, 1]], dtype=torch.float64)}
AT = {4: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64),
      6: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)}

MUTATIONS = ("lo_dropped_plane", "bt_row_sign", "edge_from_neighbour_row", "upsample_off_by_one", "tdup_pairs_swapped", "bias_omitted",
             "residual_wrong_rate", "lrelu_omitted", "stats_without_last_tile", "stats_one_parity", "variance_unbiased",
             "group_totals_per_channel", "adain_beta_offset", "weight_plane_x2")


def gamma(n):
    return n * U / (1.0 - n * U)


def gamma64(n):
    return n * U64 / (1.0 - n * U64)


def pad64(c):
    return (c + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------------ layout decoders / encoders
def _halfs(raw, n):
    return raw.contiguous().view(-1).view(torch.float16)[:n]


def _v_onehot_channels(raw, B, T, Cp, H, J):
    """One-term operand bytes -> fp16 [B, T, 6, H, J, Cp] in channel order (pieces of a row: c0-7 | c16-23 | c8-15 | c24-31)."""
    v = raw.view(torch.float16)[: B * T * Cp // 32 * 6 * H * J * 32].view(B, T, Cp // 32, 6, H, J, 4, 8)
    v = v[:, :, :, :, :, :, [0, 2, 1, 3], :]
    return v.permute(0, 1, 3, 4, 5, 2, 6, 7).reshape(B, T, 6, H, J, Cp)


def _v_split_hi(raw, B, T, C, H, J, nrows):
    """Split operand bytes (first nrows rows of 64 B) -> hi parts fp16 [rows of (b, t, chunk16, x, h, j)][16 channels]."""
    v = raw.view(torch.float16)[: nrows * 32].view(nrows, 4, 8)
    return v[:, [0, 2], :].reshape(nrows, 16)


def operand_floats(kind, B, T, H, W, C):
    """Floats of the whole operand (the count tap 1 / 3 copies)."""
    pos = B * T * H * W
    return {"f32": pos * C, "hl16": pos * C, "f23": pos * C * 2, "f43": pos * C * 3 // 2, "f43_f32": pos * C * 3 // 2,
            "f43_one": pos * pad64(C) * 3 // 4}[kind]


def decode_operand(kind, raw, B, T, H, W, C, parts=False):
    """raw: float32 [operand_floats] -> float64 values (module docstring).  parts = True (split formats): (hi, lo) instead; the
    one-term format returns (values, padding channels)."""
    if kind == "f32":
        return raw[: B * T * H * W * C].view(B, T, H, W, C).double()
    if kind == "hl16":
        v = _halfs(raw, B * T * H * W * C * 2).view(B, T, H, W, C // 8, 2, 8).double()
        hi, lo = v[..., 0, :].reshape(B, T, H, W, C), v[..., 1, :].reshape(B, T, H, W, C)
        return (hi, lo) if parts else hi + lo
    P = PLANES[kind]
    J = W // (2 if P == 4 else 4)
    if kind == "f43_f32":
        return raw[: 6 * B * T * H * J * C].view(6, B, T, H, J, C).permute(1, 2, 0, 3, 4, 5).double()
    if kind == "f43_one":
        Cp = pad64(C)
        v = _v_onehot_channels(raw.contiguous().view(-1), B, T, Cp, H, J).double()
        return (v[..., :C], v[..., C:]) if parts else v[..., :C]
    v = _halfs(raw, B * T * (C // 16) * P * H * J * 32).view(B, T, C // 16, P, H, J, 2, 2, 8).double()
    v = v.permute(0, 1, 3, 4, 5, 2, 6, 7, 8)            # [B, T, P, H, J, C16, group of 8, hi | lo, 8]
    hi, lo = v[..., 0, :].reshape(B, T, P, H, J, C), v[..., 1, :].reshape(B, T, P, H, J, C)
    return (hi, lo) if parts else hi + lo


def split16(v):
    """fp32 values -> (hi, lo) fp16 as the writers form them: hi = (half)v, lo = (half)(v - (float)hi)."""
    v = v.float()
    hi = v.half()
    return hi, (v - hi.float()).half()


def encode_operand(kind, v, drop_lo_plane=None):
    """Values (fp32-representable; [B, T, H, W, C] or [B, T, P, H, J, C]) -> the raw float32 buffer of the format."""
    v = v.float()
    if kind == "f32":
        return v.contiguous().view(-1)
    if kind == "hl16":
        B, T, H, W, C = v.shape
        hi, lo = split16(v)
        out = torch.stack((hi.view(B, T, H, W, C // 8, 8), lo.view(B, T, H, W, C // 8, 8)), 5)
        return out.contiguous().view(-1).view(torch.float32)
    B, T, P, H, J, C = v.shape
    if kind == "f43_f32":
        return v.permute(2, 0, 1, 3, 4, 5).contiguous().view(-1)
    if kind == "f43_one":
        Cp = pad64(C)
        h = F.pad(v.half(), (0, Cp - C)).view(B, T, P, H, J, Cp // 32, 4, 8)[..., [0, 2, 1, 3], :]
        return h.permute(0, 1, 5, 2, 3, 4, 6, 7).contiguous().view(-1).view(torch.float32)
    hi, lo = split16(v)
    if drop_lo_plane is not None:
        lo = lo.clone()
        lo[:, :, drop_lo_plane] = 0
    out = torch.stack((hi.view(B, T, P, H, J, C // 16, 2, 8), lo.view(B, T, P, H, J, C // 16, 2, 8)), 7)
    return out.permute(0, 1, 5, 2, 3, 4, 6, 7, 8).contiguous().view(-1).view(torch.float32)


# ------------------------------------------------------------------------------------------------------ statistics
def stats_ref(x, mutate=None):
    """x [B, ..., C] (float32 values) -> ((sum, sumsq) [B, C, 2] float64, bound [B, C, 2])."""
    B, C = x.shape[0], x.shape[-1]
    x = x.double()
    if mutate == "stats_one_parity":
        x = x[:, 0::2]
    x = x.reshape(B, -1, C)
    n = x.shape[1]
    s, q, a = x.sum(1), (x * x).sum(1), x.abs().sum(1)
    if mutate == "stats_without_last_tile":
        c0 = (C - 1) // 32 * 32
        s, q = s.clone(), q.clone()
        s[:, c0:] = 0
        q[:, c0:] = 0
    g = gamma64(n + 8)
    return torch.stack((s, q), 2), torch.stack((g * a, g * q), 2)


def stats_emulate(x, mutate=None):
    """The kernels' arithmetic on the host: fp64 accumulation of the fp32 values in another order (partials of 64 positions)."""
    B, C = x.shape[0], x.shape[-1]
    if mutate == "stats_one_parity":
        x = x[:, 0::2]
    x = x.double().reshape(B, -1, C)
    pad = (-x.shape[1]) % 64
    x = F.pad(x, (0, 0, 0, pad)).view(B, -1, 64, C)
    s, q = x.sum(2).flip(1).sum(1), (x * x).sum(2).flip(1).sum(1)
    if mutate == "stats_without_last_tile":
        c0 = (C - 1) // 32 * 32
        s[:, c0:] = 0
        q[:, c0:] = 0
    return torch.stack((s, q), 2)


# ------------------------------------------------------------------------------------------------------ coefficient tables
def coef_ref(sums, groups, count, adain=None, affine=None, mutate=None, dtype=torch.float64):
    """sums [B, C, 2] float64 (tapped) -> ((A, B) [B, C, 2] float64, bound [B, C, 2]).  adain = (z [B, Z], weight [2C, Z], bias [2C]):
    gamma | beta = Linear(z) in float64; affine = (weight [C], bias [C]) of a GroupNorm; neither: plain normalisation."""
    B, C, _ = sums.shape
    cpg = C // groups
    if mutate == "group_totals_per_channel":
        cpg = 1
    tot = sums.double().view(B, C // cpg, cpg, 2).sum(2)
    n = float(count) * cpg
    mean = tot[..., 0] / n
    ex2 = tot[..., 1] / n
    var = (ex2 - mean * mean).clamp_min(0)
    if mutate == "variance_unbiased":
        var = var * (n / (n - 1))
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    e_rstd = 0.5 * rstd ** 3 * ((cpg + 16) * U64 * (ex2 + mean * mean))
    mean, rstd, e_rstd = (t.repeat_interleave(cpg, 1) for t in (mean, rstd, e_rstd))
    g = torch.ones(B, C, dtype=torch.float64, device=sums.device)
    b = torch.zeros_like(g)
    eg, eb = torch.zeros_like(g), torch.zeros_like(g)
    if adain is not None:
        z, w, bias = (t.to(sums.device).to(dtype) for t in adain)
        lin = (z @ w.t() + bias).double()
        s_lin = z.double().abs() @ w.double().abs().t() + bias.double().abs()
        off = C - 1 if mutate == "adain_beta_offset" else C
        g, b = lin[:, :C], lin[:, off:off + C]
        eg, eb = gamma(z.shape[1] + 2) * s_lin[:, :C], gamma(z.shape[1] + 2) * s_lin[:, C:]
    elif affine is not None:
        g = affine[0].to(sums.device).double()[None].expand(B, C)
        b = affine[1].to(sums.device).double()[None].expand(B, C)
    A = g * rstd
    Bc = b - g * mean * rstd
    # (+ U |.|: with the gate's own 2^-24 |ref| one fp32 step -- the table's single rounding to fp32 attains half a step)
    eA = rstd * eg + g.abs() * e_rstd + 4 * U64 * A.abs() + U * A.abs()
    eB = eb + (mean * rstd).abs() * eg + g.abs() * mean.abs() * e_rstd + 4 * U64 * (b.abs() + (g * mean * rstd).abs()) + U * Bc.abs()
    if dtype != torch.float64:       # the host emulation: the table rounded to fp32 as the kernel stores it
        A, Bc = A.float().double(), Bc.float().double()
    return torch.stack((A, Bc), 2), torch.stack((eA, eB), 2)


# ------------------------------------------------------------------------------------------------------ operand writers
def _nearest(x, dim, f, size, off_by_one):
    idx = torch.arange(size, device=x.device)
    idx = ((idx + 1) // f).clamp_max(size // f - 1) if off_by_one and f == 4 else idx // f
    return x.index_select(dim, idx)


def writer_ref(kind, x, coef, gb, ut, us, dtype=torch.float64, mutate=None):
    """The operand a writer forms, from the tapped block input / conv_0 output x [B, Tl, Hl, Wl, C], the tapped (A, B) table coef
    [B, C, 2] and the tapped maps gb [B, H, W, 2C] (None behind ADAIN): d = lrelu((x A + B) g' + beta) through the nearest map, then
    B^T along W with zero padding.  (ut = 1 on the half-rate operand of a temporal-duplication conv.)  -> (values, S) in `dtype`:
    [B, T, H, W, C] or [B, T, P, H, J, C]; S = the same expression over absolute values.  coef = None (SPADE's own branch: the
    128-channel activation goes to the Winograd operand as it is): d = x, no table, no maps, no lrelu."""
    B, Tl, Hl, Wl, C = x.shape
    T, H, W = Tl * ut, Hl * us, Wl * us
    x = x.to(dtype)
    ob1 = mutate == "upsample_off_by_one"
    xu = _nearest(_nearest(_nearest(x, 1, ut, T, ob1), 2, us, H, ob1), 3, us, W, ob1)
    if coef is None:
        d, S = xu, xu.abs()
    else:
        a = coef[..., 0].to(dtype).view(B, 1, 1, 1, C)
        b = coef[..., 1].to(dtype).view(B, 1, 1, 1, C)
        sb = b.abs()
        if gb is not None:
            ga, be = gb[..., :C].to(dtype).unsqueeze(1), gb[..., C:].to(dtype).unsqueeze(1)
            sb = sb * ga.abs() + be.abs()
            b = b * ga + be
            a = a * ga
        r = xu * a + b
        d = torch.where(r >= 0, r, 0.2 * r)
        S = xu.abs() * a.abs() + sb
    if kind in ("f32", "hl16"):
        return d, S.expand_as(d)
    P = PLANES[kind]
    step = 2 if P == 4 else 4
    J = W // step

    def tiles(v):
        if mutate == "edge_from_neighbour_row":   # the flat [H * W] row read one element past its ends
            flat = F.pad(v.reshape(B, T, H * W, C), (0, 0, 1, 1))
            idx = (torch.arange(H, device=v.device) * W)[:, None] + torch.arange(W + 2, device=v.device)[None]
            vp = flat[:, :, idx.reshape(-1)].view(B, T, H, W + 2, C)
        else:
            vp = F.pad(v, (0, 0, 1, 1))
        return vp.unfold(3, P, step)              # [B, T, H, J, C, P positions]
    bt = BT[P].to(x.device).to(dtype)
    if mutate == "bt_row_sign":
        bt = bt.clone()
        bt[1] = -bt[1]
    V = torch.einsum("pk,bthjck->btphjc", bt, tiles(d))
    SV = torch.einsum("pk,bthjck->btphjc", BT[P].to(x.device).to(dtype).abs(), tiles(S.expand_as(d)))
    assert V.shape == (B, T, P, H, J, C)
    return V, SV


def writer_bound(kind, ref, S):
    e = gamma(7) * S.double()
    v = ref.abs() + e
    if kind == "f43_one":
        return e + 2.0 ** -10 * v + 2.0 ** -24
    if kind in SPLIT:
        return e + 2.0 ** -22 * v + 2.0 ** -25
    return e


# ------------------------------------------------------------------------------------------------------ convs
def sn_weight64(sd, name):
    """The spectral-norm-folded weight in float64 (the fp32 parameters, sigma = u . (W v) in float64)."""
    w = sd[name + ".weight_orig"].double()
    u, v = sd[name + ".weight_u"].double(), sd[name + ".weight_v"].double()
    return w / (u @ (w.reshape(w.shape[0], -1) @ v))


def pair_sets(w, tdup):
    """w [O, C, 3, 3, 3] -> [nset, O, C, KT, 3, 3]: the kernel itself, or the two pair-summed 2-tap temporal kernels of a conv behind
    a x2 temporal duplication (parity 0: (W0, W1 + W2), parity 1: (W0 + W1, W2))."""
    if not tdup:
        return w[None]
    return torch.stack([torch.stack([w[:, :, 0], w[:, :, 1] + w[:, :, 2]], 2), torch.stack([w[:, :, 0] + w[:, :, 1], w[:, :, 2]], 2)])


def wino_u(w3, P):
    """[..., 3] -> U = G g [P, ...] with the packer's expressions (wino_g23 / wino_g43)."""
    g0, g1, g2 = w3[..., 0], w3[..., 1], w3[..., 2]
    if P == 4:
        return torch.stack([g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2])
    return torch.stack([g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6, g0 / 24 - g1 / 12 + g2 / 6, g2])


def half_once(x):
    """float64 -> the nearest fp16 value, rounded ONCE (numpy's conversion; torch's goes through fp32), back in float64."""
    return torch.from_numpy(x.detach().cpu().numpy().astype(np.float16).astype(np.float64)).to(x.device)


def prescale_exp(wmax):
    return max(-40, min(40, int(np.floor(np.log2(16384.0 / wmax))))) if wmax > 0 else 0


def _corr(x, w, tpad):
    """x [B, T, H, R, C], w [O, C, KT, KH, KW] -> [B, T', H, R, O]: correlation with zero padding 1 in H, (KW - 1) / 2 in R and
    tpad = (front, back) in T, as matmuls over shifted views (float64 on any device)."""
    O, C, KT, KH, KW = w.shape
    B, T, H, R, _ = x.shape
    pw = (KW - 1) // 2
    xp = F.pad(x, (0, 0, pw, pw, 1, 1, tpad[0], tpad[1]))
    To = T + tpad[0] + tpad[1] - KT + 1
    out = torch.zeros(B, To, H, R, O, dtype=x.dtype, device=x.device)
    for kt in range(KT):
        for kh in range(KH):
            for kw in range(KW):
                out += xp[:, kt:kt + To, kh:kh + H, kw:kw + R] @ w[:, :, kt, kh, kw].t()
    return out


def conv_ref(kind, opnd, w, bias, res, rt, rs, lrelu, tdup, dtype=torch.float64, mutate=None):
    """The conv on its decoded operand (float64 [B, Ti, H, W, C] or [B, Ti, P, H, J, C]; Ti = T / 2 for tdup) with the folded
    weights w [O, C, KT, 3, 3] float64 (KT = 3, or 1: the 2-D convs of SPADE's branch, no padding in time), + bias + the residual read through the (rt, rs) nearest map, optional lrelu.
    -> (out [B, T, H, W, O], S, S1): S = sum |A^T| sum |U||V| + |bias| + |res|, S1 = sum |A^T| sum |V| (for the weights' subnormal
    floor).  dtype = float32: the host emulation (weights rounded to fp32 as the packers do, fp32 accumulation)."""
    dev = opnd.device
    ws = pair_sets(w.to(dev), tdup)
    nset, O, C, KT = ws.shape[:4]
    P = PLANES.get(kind)
    wexp = 0
    if P:
        Us = wino_u(ws, P)                                   # [P, nset, O, C, KT, 3]
        if mutate == "weight_plane_x2":
            Us = Us.clone()
            Us[1] = 2 * Us[1]
        if kind == "f43_one":   # the packer's rounding: G g 2^wexp in fp64, rounded to fp16 once; undone by the epilogue's 2^-wexp
            wexp = prescale_exp(float(wino_u(ws, P).abs().max()))
            Us = half_once(Us * 2.0 ** wexp)
        Ws = [[Us[p, s][..., None] for p in range(P)] for s in range(nset)]
    else:
        Ws = [[ws[s]] for s in range(nset)]
    if dtype != torch.float64 and kind != "f43_one":
        Ws = [[u.float() for u in row] for row in Ws]
    x = opnd.to(dtype)
    Ti = x.shape[1]
    outs, Ss, S1s = [], [], []
    for s in range(nset):
        tpad = ((KT - 1) // 2, (KT - 1) // 2) if not tdup else ((1, 0) if s == 0 else (0, 1))
        if mutate == "tdup_pairs_swapped" and tdup:
            tpad = (0, 1) if s == 0 else (1, 0)
        if P:
            at = AT[P].to(dev)
            M = torch.stack([_corr(x[:, :, p], Ws[s][p].to(dtype), tpad) for p in range(P)])      # [P, B, T, H, J, O]
            SM = torch.stack([_corr(x[:, :, p].abs().double(), Ws[s][p].abs().double(), tpad) for p in range(P)])
            S1 = torch.stack([_corr(x[:, :, p].abs().double(), torch.ones(1, C, KT, 3, 1, dtype=torch.float64, device=dev), tpad) for p in range(P)])
            def back(m, a):
                y = torch.einsum("mp,pbthjo->bthjmo", a.to(m.dtype), m)
                return y.reshape(y.shape[0], y.shape[1], y.shape[2], -1, y.shape[5])
            outs.append(back(M, at) * 2.0 ** -wexp)
            Ss.append(back(SM, at.abs()) * 2.0 ** -wexp)
            S1s.append(back(S1, at.abs()))
        else:
            outs.append(_corr(x, Ws[s][0].to(dtype), tpad))
            Ss.append(_corr(x.abs().double(), Ws[s][0].abs().double(), tpad))
            S1s.append(_corr(x.abs().double(), torch.ones(1, C, KT, 3, 3, dtype=torch.float64, device=dev), tpad))

    def merge(parts):
        if nset == 1:
            return parts[0]
        y = torch.stack(parts, 2)                            # [B, Ti, parity, H, W, O]
        return y.reshape(y.shape[0], 2 * Ti, *y.shape[3:])
    y, S, S1 = merge(outs), merge(Ss), merge(S1s)
    if mutate != "bias_omitted":
        y = y + bias.to(dev).to(dtype)
    S = S + bias.to(dev).double().abs()
    if res is not None:
        B, T, H, W, _ = y.shape
        r = res.to(dtype)
        if mutate == "residual_wrong_rate":                  # read at the output's own rate (factor 1), clamped to the low-rate tensor
            ru = r
            for dim, size in ((1, T), (2, H), (3, W)):
                ru = ru.index_select(dim, torch.arange(size, device=dev).clamp_max(r.shape[dim] - 1))
        else:
            ru = _nearest(_nearest(_nearest(r, 1, rt, T, False), 2, rs, H, False), 3, rs, W, False)
        y = y + ru
        S = S + ru.abs().double()
    if lrelu and mutate != "lrelu_omitted":
        y = torch.where(y >= 0, y, 0.2 * y)
    return y, S, S1


def conv_chain(kind, cin, tdup, kt=None):
    """Length of the fp32 accumulation chain of one output (module docstring).  kt: temporal taps (default 3, 2 for a tdup pair; 1 for
    the 2-D convs of SPADE's branch)."""
    kt = kt or (2 if tdup else 3)
    if kind == "f32":
        return (cin + 1) // 2 * 9 * kt + 2 + 8
    if kind == "f43_f32":
        return (cin + 1) // 2 * 3 * kt + 2 + 8
    if kind == "hl16":
        return (cin + 7) // 8 * kt * 9 * 3 + 16 + 8
    if kind == "f43_one":
        return pad64(cin) // 16 * kt * 3 + 16 + 8
    return (cin + 7) // 8 * kt * 3 * 3 + 16 + 8


def conv_bound(kind, cin, tdup, w, S, S1, kt=None):
    """Element-wise bound of a conv output (module docstring).  w: the folded weights (for the prescale exponent)."""
    e = gamma(conv_chain(kind, cin, tdup, kt)) * S
    if kind in ("f32", "f43_f32"):
        return e + 2 * U * S
    if kind == "f43_one":
        return e
    ws = pair_sets(w, tdup)
    P = PLANES.get(kind)
    wexp = prescale_exp(float((wino_u(ws, P) if P else ws).abs().max()))
    return e + (2 * U + 2.0 ** -22 + 2.0 ** -22) * S + 2.0 ** -25 * 2.0 ** -wexp * S1


def within(got, ref, bound, rel=U):
    """Worst |got - ref| / (bound + rel |ref|) over the elements; NaN (an unwritten tap) counts as infinite."""
    r = (got.double() - ref.double()).abs() / (bound.double() + rel * ref.double().abs() + 1e-300)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------ decoder geometry
def levels(ups, upt):
    """Per block: (T, H, W, ut, us) of the level it runs at (i2v_dec_create)."""
    T, S, out = 1, 4, []
    for k in range(6):
        ut, us = (1, 1) if k == 0 else (2, 2) if k <= 3 else (upt[k - 4], ups[k - 4])
        T, S = T * ut, S * us
        out.append((T, S, S, ut, us))
    return out


def spade_groups(c, g=16):
    while c % g:
        g -= 1
    return g


def can_fuse_stats(T, H, W):
    """conv16_can_fuse_stats: the 256-position brick of the split kernels lies inside one sample."""
    return T * H * W >= 256


def splitk_factor(pos, nchunk):
    """conv16_splitk_factor of the direct split kernel (positions per sample, 32-channel chunks)."""
    s = 8 if pos <= 16 else 4 if pos <= 128 else 1
    while s > 1 and nchunk // s < 2:
        s //= 2
    return s
