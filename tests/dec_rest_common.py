"""Shared by tests/test_host_dec_rest.py and tests/test_gpu_dec_rest.py: the units of the stage-1 decoder OUTSIDE the twelve 3x3x3 block
convs -- conv_img (+ tanh, the frame layout), SPADE's branch, the learned shortcut's 1x1x1 GEMM with the folded Norm3D affine, and fc -- each with a plain
torch float64 reference of that unit alone, an fp32 emulation of the kernel's arithmetic for the CPU, a bound derived from operation
counts and magnitudes the way tests/dec_units_common.py derives them (its gamma(n), layout helpers and 3x3x3 correlation are used, not
copied), and named mutations that show what the gate catches.  No GPU code; imports without a GPU.

Gate, element-wise:   |got - ref| <= bound + 2^-24 |ref|   (dec_units_common's; conv_img: bound alone, it carries tanhf's rounding)

  conv_img   pre = sum w x + bias over 27 C products, then tanh.
             chain n per form (csrc/i2v_convimg.hip):
               mfma     C / 16 k-steps x 3 MFMAs into one accumulator, + 16 inside an instruction, + 27 gather adds, + 1 bias
               gemm     ceil(C / 32) stages x 2 steps x 3 MFMAs, + 16, + 1 (the 2^-wexp fma), + 27 gather adds, + 1 bias
               valu     one fmaf per (tap, channel of the 8-channel chunks): 27 * 8 * ceil(C / 8), + 1 bias
               generic  dec_units_common.conv_chain("f32", C): fp32 matrix cores, 2 channels per step
             split forms (mfma, gemm): the weights are split hi + lo (2^-22 |w|, and half an fp16 subnormal step 2^-25 -- times
             2^-wexp where the packer prescales: gemm only), the activations are split in the kernel (2^-22 |x| + 2^-25), the lo * lo
             product is left out (2^-22):   pre_bound = gamma(n) S + 3 * 2^-22 S + 2^-25 2^-wexp S1 + 2^-25 SW,
             S = sum |w||x| + |bias|, S1 = sum |x|, SW = sum |w| over the taps inside the clip.
             out:  (1 - ref^2) pre_bound + C_TANH U |ref|   (tanh' = 1 - tanh^2; C_TANH: device tanhf's error in ulp, below)
  pointwise  out = act((x A + B) @ W^T + bias + res).  S = (|x||A| + |B|) @ |W|^T + |bias| + |res|.
             chain: f32 16 steps per 32-channel stage, + 2 + 8; split-fp16 2 steps x 3 MFMAs per stage, + 16 + 8.  The affine's fmaf
             rounds once (U S).  Weights rounded to fp32 `wround` times (0: the unit entry takes fp32 weights; 1: W / sigma at load).
             split: + 3 * 2^-22 S + 2^-25 2^-wexp S1 + 2^-25 SW as above (the activation is split after the affine).
  fc         z @ W^T + b on the fp32 matrix cores: gamma(z_dim + 1) S (the issue's figure: every product and the bias added once).

  resize     bilinear, align_corners: v = lh0 (lw0 x00 + lw1 x01) + lh1 (lw0 x10 + lw1 x11), six roundings: gamma(6) S.  The source
             coordinate f = (float)(Hi - 1) / (Ho - 1) * h is rounded twice (2 U f <= 2 U Hi), which moves the weights by as much:
             + 2 U (Hi + Wi) (|x00| + |x01| + |x10| + |x11|).  Split-fp16 rows: + 2^-22 |v| + 2^-25.  Channels 3 .. 15 are exactly zero.
  SPADE      Conv2d(3, 128) + lrelu, the Winograd operand writer and the gamma | beta Conv2d(128, 2C) are dec_units_common's conv_ref /
             writer_ref / conv_bound with ONE temporal tap (kt = 1); an activation stored in the split-fp16 operand format (the direct
             form's first conv) adds 2^-22 |v| + 2^-25.

C_TANH.  No document on the build machine states the accuracy of the device library's tanhf, so it was measured once (test
test_device_tanhf_ulp prints it: conv_img's exact-fp32 forms with a one-hot weight compute tanhf(x) of chosen fp32 arguments, no kernel
was added for it) against float64 tanh of the same arguments: profiles/dec_rest_gate.md has the figure (1.055 ulp); C_TANH is 2x it."""
import torch
import torch.nn.functional as F

import dec_units_common as du

U = du.U
C_TANH = 2.12         # ulp: 2 x the 1.055 ulp measured on an MI355X (profiles/dec_rest_gate.md), rounded up in the last digit
FORMS = ("mfma", "gemm", "valu", "generic")
SPLIT_FORMS = ("mfma", "gemm")
MUTATIONS = ("tap_order_reversed", "frames_b3t", "tanh_omitted", "lo_dropped", "affine_after_gemm", "coef_row_neighbour", "lrelu_slope_001")


# ------------------------------------------------------------------------------------------------------ conv_img
def conv_img_inputs(B, T, H, W, C, seed):
    """Activations and weights for which the pre-activations have a standard deviation of 0.9 (over the temporal taps that lie inside a
    clip of T frames): they span about +-3 and fewer than 1 % of the outputs have |tanh| > 0.99 (|pre| > 2.65: 0.3 % of such a normal;
    the zero padding in H and W only lowers the variance at the borders)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, H, W, C, generator=g)
    w = 0.9 * torch.randn(3, C, 3, 3, 3, generator=g) / (9 * min(T, 3) * C) ** 0.5
    bias = 0.1 * torch.randn(3, generator=g)
    return x, w, bias


def conv_img_chain(form, C):
    return {"mfma": C // 16 * 3 + 16 + 27 + 1, "gemm": (C + 31) // 32 * 6 + 16 + 1 + 27 + 1, "valu": 27 * 8 * ((C + 7) // 8) + 1,
            "generic": du.conv_chain("f32", C, False)}[form]


def _c3(x, w, dtype):
    z = torch.zeros(w.shape[0], dtype=torch.float64)
    return du.conv_ref("f32", x, w.double(), z, None, 1, 1, False, False, dtype=dtype)


def frames_of(y):
    """channels-last [B, T, H, W, 3] -> frames [B, T, 3, H, W]."""
    return y.permute(0, 1, 4, 2, 3).contiguous()


def conv_img_ref(x, w, bias):
    """x [B, T, H, W, C] (fp32 values, any device), w [3, C, 3, 3, 3], bias [3] -> float64 (frames [B, T, 3, H, W], S, S1, SW), the
    three magnitude sums in the frames' layout."""
    dev = x.device
    w, bias = w.to(dev).double(), bias.to(dev).double()
    pre, S, S1 = du.conv_ref("f32", x.double(), w, bias, None, 1, 1, False, False)
    SW = du._corr(torch.ones_like(x, dtype=torch.float64), w.abs(), (1, 1))
    return frames_of(torch.tanh(pre)), frames_of(S), frames_of(S1.expand_as(S)), frames_of(SW)


def conv_img_bound(form, C, w, ref, S, S1, SW):
    pre = du.gamma(conv_img_chain(form, C)) * S
    if form in SPLIT_FORMS:
        wexp = du.prescale_exp(float(w.abs().max())) if form == "gemm" else 0
        pre = pre + 3 * 2.0 ** -22 * S + 2.0 ** -25 * 2.0 ** -wexp * S1 + 2.0 ** -25 * SW
    return (1 - ref * ref) * pre + C_TANH * U * ref.abs()


def conv_img_emulate(form, x, w, bias, mutate=None):
    """The form's arithmetic in fp32 on the host (operands split as the kernels split them) -> frames [B, T, 3, H, W] float32."""
    if mutate == "tap_order_reversed":
        w = w.flip(2)
    x, w = x.float(), w.float()
    if form in SPLIT_FORMS:
        scale = 2.0 ** du.prescale_exp(float(w.abs().max())) if form == "gemm" else 1.0
        xh, xl = du.split16(x)
        wh, wl = du.split16(w * scale)
        pre = _c3(xh.float(), wh.float(), torch.float32)[0] + _c3(xl.float(), wh.float(), torch.float32)[0]
        if mutate != "lo_dropped":
            pre = pre + _c3(xh.float(), wl.float(), torch.float32)[0]
        pre = pre * (1.0 / scale) + bias.float()
    else:
        pre = _c3(x, w, torch.float32)[0] + bias.float()
    y = pre if mutate == "tanh_omitted" else torch.tanh(pre)
    if mutate == "frames_b3t":          # stored [B][3][T][H][W], read as [B][T][3][H][W]
        B, T, H, W, _ = y.shape
        return y.permute(0, 4, 1, 2, 3).contiguous().view(B, T, 3, H, W)
    return frames_of(y)


def saturated_share(ref):
    return float((ref.abs() > 0.99).double().mean())


# ------------------------------------------------------------------------------------------------------ SPADE's branch
SPADE_MUTATIONS = ("align_corners_false", "gamma_bias_without_one", "gamma_beta_swapped", "lrelu_slope_001")


def _axis(n_out, n_in, align, dev, dtype):
    i = torch.arange(n_out, device=dev, dtype=dtype)
    if align:
        f = i * (torch.tensor(n_in - 1, dtype=dtype) / torch.tensor(n_out - 1, dtype=dtype) if n_out > 1 else 0.0)
    else:
        f = ((i + 0.5) * (n_in / n_out) - 0.5).clamp(0, n_in - 1)
    i0 = f.floor().long().clamp_max(n_in - 1)
    return i0, (i0 + 1).clamp_max(n_in - 1), f - i0.to(dtype)


def resize_ref(img, H, W, hl16, dtype=torch.float64, mutate=None):
    """img [F, 3, Hi, Wi] (fp32 values) -> (rows [F, 1, H, W, 16] channels-last with channels 3 .. 15 zero, bound) -- the level's input
    of SPADE's Conv2d(3, 128), bilinear with align_corners=True.  dtype = float32: the kernel's arithmetic on the host."""
    F_, C, Hi, Wi = img.shape
    dev = img.device
    align = mutate != "align_corners_false"
    h0, h1, lh = _axis(H, Hi, align, dev, dtype)
    w0, w1, lw = _axis(W, Wi, align, dev, dtype)
    x = img.to(dtype)
    c = [x[:, :, hi][:, :, :, wi] for hi in (h0, h1) for wi in (w0, w1)]
    lh, lw = lh[:, None], lw[None]

    def lerp(c00, c01, c10, c11):
        return (1 - lh) * ((1 - lw) * c00 + lw * c01) + lh * ((1 - lw) * c10 + lw * c11)
    v = lerp(*c)
    S = lerp(*(t.abs() for t in c)).double()
    A4 = sum(t.abs() for t in c).double()
    bound = du.gamma(6) * S + 2 * U * (Hi + Wi) * A4
    if hl16:
        bound = bound + 2.0 ** -22 * (v.abs().double() + bound) + 2.0 ** -25
    cl = lambda t: F.pad(t.permute(0, 2, 3, 1), (0, 13)).unsqueeze(1)
    return cl(v), cl(bound)


def spade_weights(sd, blk, dev="cpu"):
    """-> float64 (w1 [128, 16, 1, 3, 3] (input channels padded 3 -> 16), b1, wgb [2C, 128, 1, 3, 3], bgb with the +1 in the gamma half)."""
    p = blk + ".norm_0."
    w1 = F.pad(sd[p + "conv.weight"].double(), (0, 0, 0, 0, 0, 13)).unsqueeze(2)
    wgb = torch.cat((sd[p + "conv_gamma.weight"], sd[p + "conv_beta.weight"])).double().unsqueeze(2)
    bgb = torch.cat((sd[p + "conv_gamma.bias"].double() + 1.0, sd[p + "conv_beta.bias"].double()))
    return w1.to(dev), sd[p + "conv.bias"].double().to(dev), wgb.to(dev), bgb.to(dev)


def stored_hl16(ref, bound):
    """A value stored in the split-fp16 operand format: + the lo part's rounding and half an fp16 subnormal step."""
    return bound + 2.0 ** -22 * (ref.abs() + bound) + 2.0 ** -25


# ------------------------------------------------------------------------------------------------------ pointwise GEMM
def pw_inputs(M, P, Cin, Cout, seed, affine=True, res=False, bias=True):
    g = torch.Generator().manual_seed(seed)
    nb = (M + P - 1) // P
    x = torch.randn(M, Cin, generator=g) * 1.5 + 0.3
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    b = 0.1 * torch.randn(Cout, generator=g) if bias else None
    coef = torch.stack((0.5 + torch.rand(nb, Cin, generator=g), 0.5 * torch.randn(nb, Cin, generator=g)), 2) if affine else None
    r = torch.randn(M, Cout, generator=g) if res else None
    return x, w, b, coef, r


def _affine(x, coef, P, dtype, neighbour=False):
    if coef is None:
        return x.to(dtype), x.abs().double()
    rows = torch.arange(x.shape[0], device=x.device) // P
    if neighbour:
        rows = (rows + 1) % coef.shape[0]
    A, Bc = coef[rows, :, 0], coef[rows, :, 1]
    return x.to(dtype) * A.to(dtype) + Bc.to(dtype), x.abs().double() * A.abs().double() + Bc.abs().double()


def pw_ref(x, w, bias, res, coef, P, lrelu):
    """-> float64 (out [M, Cout], S, S1, SW)."""
    dev = x.device
    w = w.to(dev).double()
    xa, sa = _affine(x, coef, P, torch.float64)
    y, S = xa @ w.t(), sa @ w.abs().t()
    if bias is not None:
        y, S = y + bias.to(dev).double(), S + bias.to(dev).double().abs()
    if res is not None:
        y, S = y + res.double(), S + res.double().abs()
    if lrelu:
        y = torch.where(y >= 0, y, 0.2 * y)
    return y, S, sa.sum(1, keepdim=True).expand_as(S), w.abs().sum(1)[None].expand_as(S)


def pw_chain(kind, cin):
    stages = (cin + 31) // 32
    return stages * 16 + 2 + 8 if kind == "f32" else stages * 6 + 16 + 8


def pw_bound(kind, cin, w, S, S1, SW, affine, wround=0):
    e = du.gamma(pw_chain(kind, cin)) * S + (U * S if affine else 0) + wround * U * S
    if kind == "f32":
        return e
    wexp = du.prescale_exp(float(w.abs().max()))
    return e + 3 * 2.0 ** -22 * S + 2.0 ** -25 * 2.0 ** -wexp * S1 + 2.0 ** -25 * SW


def pw_emulate(kind, x, w, bias, res, coef, P, lrelu, mutate=None):
    """fp32 emulation on the host -> [M, Cout] float32."""
    w = w.float()
    late = mutate == "affine_after_gemm" and coef is not None
    xa = x.float() if late else _affine(x, coef, P, torch.float32, neighbour=mutate == "coef_row_neighbour")[0]
    if kind == "f32":
        y = xa @ w.t()
    else:
        scale = 2.0 ** du.prescale_exp(float(w.abs().max()))
        xh, xl = du.split16(xa)
        wh, wl = du.split16(w * scale)
        y = xh.float() @ wh.float().t() + xl.float() @ wh.float().t()
        if mutate != "lo_dropped":
            y = y + xh.float() @ wl.float().t()
        y = y * (1.0 / scale)
    if late:   # norm applied to the GEMM's output (rows of the table cycled over the output channels)
        rows = torch.arange(x.shape[0]) // P
        idx = torch.arange(w.shape[0]) % x.shape[1]
        y = y * coef[rows][:, idx, 0] + coef[rows][:, idx, 1]
    if bias is not None:
        y = y + bias.float()
    if res is not None:
        y = y + res.float()
    if lrelu:
        y = torch.where(y >= 0, y, (0.01 if mutate == "lrelu_slope_001" else 0.2) * y)
    return y


# ------------------------------------------------------------------------------------------------------ fc
def fc_ref(z, w, b, nf):
    """head_0's input as tap 12 holds it: Linear(z_dim, 16 nf * 16)(z) viewed [B, 16 nf, 1, 4, 4] (decoder.py:99), channels-last
    [B, 1, 4, 4, 16 nf] -> float64 (ref, bound)."""
    dev = z.device
    z, w, b = z.double(), w.to(dev).double(), b.to(dev).double()
    y = z @ w.t() + b
    S = z.abs() @ w.abs().t() + b.abs()
    cl = lambda t: t.view(-1, 16 * nf, 1, 4, 4).permute(0, 2, 3, 4, 1).contiguous()
    return cl(y), cl(du.gamma(z.shape[1] + 1) * S)


def within(got, ref, bound, rel=U):
    """dec_units_common's gate |got - ref| <= bound + rel |ref| (conv_img: rel = 0, its bound carries tanhf's rounding)."""
    return du.within(got, ref, bound, rel=rel)
