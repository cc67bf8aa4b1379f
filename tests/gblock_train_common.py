"""Shared by tests/test_host_gblock_train.py, tests/test_gpu_gblock_train.py and tests/golden/make_golden_gblock_train.py: the fixtures'
configurations, seeded parameters and inputs, a float64 oracle of one GeneratorBlock (decoder.py:7-52) whose backward is written out by
hand from the formulas of DESIGN.md 12.8, float64 oracles of the new kernel families with the deliberate errors the gate must catch,
and the bounds of the unit tests.

Gates.  The module against the fixtures: relative L2 <= 1e-4 per tensor, the project's gate.  The units, element-wise, the dot-product
gate of tests/i3d_units_common.py, |got - ref64| <= gamma(n) S + u |ref64| with S the same sum over absolute values:
  pointwise conv (1x1x1) and its input gradient   n = K + 1                       (K: the channels summed over; + 1: the added term)
  a conv's input gradient                         n = taps cout + 1
  a weight gradient                               n = slices + slice length       (fp32 MFMA sums inside a slice, fp32 over the slices)
  the spectral-norm projection                    bound(dW) / sigma + gamma(4) (|dW| + |<dW, W>| |u| |v|) / sigma + |proj| bound(<dW, W>) / sigma
  bias gradient, Linear backward                  float64 sums rounded once: n = 1
  modulated norm backward                         the sums are float64; fp32 enters through ga = 0.2 g (one rounding), the final rounding and
                                                  the add: n = 4 on S = rstd (|ga m| + |mean terms|) + |add|; the maps dgamma / dbeta: n = 2"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from i3d_units_common import U, gamma, gate, gate_bound  # noqa: F401

TOL_L2 = 1e-4
SGD_STEPS = 6
SGD_LR = 1e-3   # measured when the fixtures were made (make_golden_gblock_train.py --check prints the fp32 / float64 distance per step)

#            n_in, n_out, spectral, z_dim, B, (T, H, W), (img_h, img_w), seed
FIXTURES = {
    "a": dict(n_in=32, n_out=16, spectral=True, z_dim=8, B=2, map=(3, 5, 6), img=(11, 13), seed=11),
    "b": dict(n_in=16, n_out=16, spectral=False, z_dim=4, B=1, map=(1, 4, 4), img=(4, 4), seed=12),
    "c": dict(n_in=48, n_out=64, spectral=True, z_dim=8, B=3, map=(2, 4, 4), img=(9, 7), seed=13),
}


def param_shapes(cfg):
    """{state_dict key: shape} in the order of GeneratorBlock.state_dict()."""
    n_in, n_out, z, sn = cfg["n_in"], cfg["n_out"], cfg["z_dim"], cfg["spectral"]
    n_mid, learned = min(n_in, n_out), n_in != n_out
    out = {}

    def conv(name, co, ci, k, bias):
        if bias:
            out[name + ".bias"] = (co,)
        if sn:
            out[name + ".weight_orig"] = (co, ci) + k
            out[name + ".weight_u"] = (co,)
            out[name + ".weight_v"] = (ci * int(np.prod(k)),)
        else:
            out[name + ".weight"] = (co, ci) + k
    conv("conv_0", n_mid, n_in, (3, 3, 3), True)
    conv("conv_1", n_out, n_mid, (3, 3, 3), True)
    if learned:
        conv("conv_s", n_out, n_in, (1, 1, 1), False)
    for name, co, ci in (("norm_0.conv", 128, 3), ("norm_0.conv_gamma", n_in, 128), ("norm_0.conv_beta", n_in, 128)):
        out[name + ".weight"] = (co, ci, 3, 3)
        out[name + ".bias"] = (co,)
    out["norm_1.linear.weight"] = (2 * n_mid, z)
    out["norm_1.linear.bias"] = (2 * n_mid,)
    if learned:
        out["norm_s.bn.weight"] = (n_in,)
        out["norm_s.bn.bias"] = (n_in,)
    return out


def is_buffer(key):
    return key.endswith(".weight_u") or key.endswith(".weight_v")


def synthetic_state(cfg):
    """Seeded fp32 parameters (numpy): weights ~ N(0, 1 / fan_in) scaled up so that activations stay O(1), unit u / v, GroupNorm weights
    around 1."""
    rng = np.random.default_rng(cfg["seed"])
    sd = {}
    for k, shp in param_shapes(cfg).items():
        a = rng.standard_normal(shp)
        if is_buffer(k):
            a = a / np.linalg.norm(a)
        elif k.endswith("bn.weight"):
            a = 1.0 + 0.3 * a
        elif k.endswith(".bias"):
            a = 0.2 * a
        else:
            a = a * (1.5 / np.sqrt(np.prod(shp[1:])))
        sd[k] = a.astype(np.float32)
    return sd


def inputs(cfg):
    """x [B, n_in, T, H, W], z [B, z_dim], img [B, 3, h, w] and the loss coefficients c [B, n_out, T, H, W], fp32."""
    rng = np.random.default_rng(cfg["seed"] + 1000)
    B, (T, H, W) = cfg["B"], cfg["map"]
    x = rng.standard_normal((B, cfg["n_in"], T, H, W)).astype(np.float32)
    z = rng.standard_normal((B, cfg["z_dim"])).astype(np.float32)
    img = rng.uniform(-1, 1, (B, 3) + tuple(cfg["img"])).astype(np.float32)
    c = rng.standard_normal((B, cfg["n_out"], T, H, W)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, z, img, c))


# ---------------------------------------------------------------------------------------------------------------- the float64 oracle
def lrelu(x):
    return torch.where(x > 0, x, 0.2 * x)


def lrelu_slope(h, slope_at_zero=0.2):
    s = torch.where(h > 0, torch.ones_like(h), torch.full_like(h, 0.2))
    return torch.where(h == 0, torch.full_like(h, slope_at_zero), s)


def _unit(v):
    return v / v.norm().clamp_min(1e-12)


def spectral(w, u, v, iterate):
    """torch.nn.utils.spectral_norm's compute_weight with one power iteration: -> (W / sigma, u, v, sigma)."""
    m = w.reshape(w.shape[0], -1)
    if iterate:
        v = _unit(m.t() @ u)
        u = _unit(m @ v)
    sigma = u @ (m @ v)
    return w / sigma, u, v, sigma


def sn_project(dwn, wn, u, v, sigma, drop_projection=False):
    """dW_orig = (dW - <dW, W> u v^T) / sigma, W = W_orig / sigma."""
    if drop_projection:
        return dwn / sigma
    return (dwn - (dwn * wn).sum() * torch.outer(u, v).view_as(dwn)) / sigma


def group_stats(x, groups, unbiased=False):
    B, C = x.shape[:2]
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    var = xg.var(-1, unbiased=unbiased, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = ((xg - mean) * rstd).reshape(x.shape)
    return xhat, rstd.expand(B, groups, C // groups).reshape(B, C, *([1] * (x.dim() - 2)))


def norm_backward(gp, xhat, rstd, groups):
    """dx = rstd (g' - mean_G g' - xhat mean_G (g' xhat)) with the means over each group's channels and all positions."""
    B = gp.shape[0]
    m1 = gp.reshape(B, groups, -1).mean(-1)
    m2 = (gp * xhat).reshape(B, groups, -1).mean(-1)
    cpg = gp.shape[1] // groups
    ex = lambda m: m.repeat_interleave(cpg, 1).reshape(B, gp.shape[1], *([1] * (gp.dim() - 2)))  # noqa: E731
    return rstd * (gp - ex(m1) - xhat * ex(m2))


def conv_grads(x, w, g, pad):
    """(dx, dw, db) of a stride-1 conv in any number of dimensions: the full correlation with the flipped taps, the correlation of the
    input with g."""
    nd = w.dim() - 2
    tconv = F.conv_transpose3d if nd == 3 else F.conv_transpose2d
    dx = tconv(g, w, padding=pad)
    conv = F.conv3d if nd == 3 else F.conv2d
    # dw[co, ci, k] = sum_b,p g[b, co, p] x[b, ci, p + k - pad]: a conv of x (channels as batch) with g as the kernel
    dw = conv(x.transpose(0, 1), g.transpose(0, 1), padding=pad).transpose(0, 1)
    db = g.sum(dim=[0] + list(range(2, g.dim())))
    return dx, dw, db


def block(sd, x, z, img, cfg, c=None, train=True, dtype=torch.float64):
    """One GeneratorBlock forward and, with the loss sum(c out), the hand-written backward.  ``sd``: {key: tensor or array}.
    -> dict(out, u/v after, and with c: dx, dz, grads {parameter key: gradient})."""
    t = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    x, z, img = x.to(dtype), z.to(dtype), img.to(dtype)
    sn, learned = cfg["spectral"], cfg["n_in"] != cfg["n_out"]
    n_mid = min(cfg["n_in"], cfg["n_out"])
    res = {}
    W, SN = {}, {}
    for name in ("conv_0", "conv_1") + (("conv_s",) if learned else ()):
        if sn:
            wn, u, v, sigma = spectral(t[name + ".weight_orig"], t[name + ".weight_u"], t[name + ".weight_v"], train)
            W[name], SN[name] = wn, (u, v, sigma)
            res[name + ".weight_u"], res[name + ".weight_v"] = u, v
        else:
            W[name] = t[name + ".weight"]
    T, H, Wd = x.shape[2:]
    # Spade and its branch
    xh0, rstd0 = group_stats(x, 16)
    y = F.interpolate(img, size=(H, Wd), mode="bilinear", align_corners=True)
    y1p = F.conv2d(y, t["norm_0.conv.weight"], t["norm_0.conv.bias"], padding=1)
    y1 = lrelu(y1p)
    gam = F.conv2d(y1, t["norm_0.conv_gamma.weight"], t["norm_0.conv_gamma.bias"], padding=1)
    bet = F.conv2d(y1, t["norm_0.conv_beta.weight"], t["norm_0.conv_beta.bias"], padding=1)
    h0 = xh0 * (1 + gam.unsqueeze(2)) + bet.unsqueeze(2)
    a0 = lrelu(h0)
    y0 = F.conv3d(a0, W["conv_0"], t["conv_0.bias"], padding=1)
    # ADAIN
    xh1, rstd1 = group_stats(y0, n_mid)
    lin = z @ t["norm_1.linear.weight"].t() + t["norm_1.linear.bias"]
    gz = lin[:, :n_mid, None, None, None]
    h1 = gz * xh1 + lin[:, n_mid:, None, None, None]
    a1 = lrelu(h1)
    dx1 = F.conv3d(a1, W["conv_1"], t["conv_1.bias"], padding=1)
    if learned:
        xhs, rstds = group_stats(x, 16)
        nsw = t["norm_s.bn.weight"].view(1, -1, 1, 1, 1)
        xn = xhs * nsw + t["norm_s.bn.bias"].view(1, -1, 1, 1, 1)
        xs = F.conv3d(xn, W["conv_s"])
    else:
        xs = x
    res["out"] = xs + dx1
    if c is None:
        return res
    g = c.to(dtype)
    grads = {}

    def put_conv(name, dwn):
        if sn:
            grads[name + ".weight_orig"] = sn_project(dwn, W[name], *SN[name])
        else:
            grads[name + ".weight"] = dwn
    # conv_1, the LeakyReLU, ADAIN and its Linear
    d_a1, dwn, grads["conv_1.bias"] = conv_grads(a1, W["conv_1"], g, 1)
    put_conv("conv_1", dwn)
    d_h1 = d_a1 * lrelu_slope(h1)
    d_lin = torch.cat([(d_h1 * xh1).sum((2, 3, 4)), d_h1.sum((2, 3, 4))], 1)
    grads["norm_1.linear.weight"] = d_lin.t() @ z
    grads["norm_1.linear.bias"] = d_lin.sum(0)
    res["dz"] = d_lin @ t["norm_1.linear.weight"]
    d_y0 = norm_backward(d_h1 * gz, xh1, rstd1, n_mid)
    # conv_0, the LeakyReLU, Spade
    d_a0, dwn, grads["conv_0.bias"] = conv_grads(a0, W["conv_0"], d_y0, 1)
    res["scale"] = {"conv_0.bias": d_y0.abs().sum((0, 2, 3, 4))}
    put_conv("conv_0", dwn)
    d_h0 = d_a0 * lrelu_slope(h0)
    dgam, dbet = (d_h0 * xh0).sum(2), d_h0.sum(2)
    dx = norm_backward(d_h0 * (1 + gam.unsqueeze(2)), xh0, rstd0, 16)
    # Spade's branch
    dy1_g, grads["norm_0.conv_gamma.weight"], grads["norm_0.conv_gamma.bias"] = conv_grads(y1, t["norm_0.conv_gamma.weight"], dgam, 1)
    dy1_b, grads["norm_0.conv_beta.weight"], grads["norm_0.conv_beta.bias"] = conv_grads(y1, t["norm_0.conv_beta.weight"], dbet, 1)
    d_y1p = (dy1_g + dy1_b) * lrelu_slope(y1p)
    _, grads["norm_0.conv.weight"], grads["norm_0.conv.bias"] = conv_grads(y, t["norm_0.conv.weight"], d_y1p, 1)
    # the shortcut
    if learned:
        d_xn, dwn, _ = conv_grads(xn, W["conv_s"], g, 0)
        put_conv("conv_s", dwn)
        grads["norm_s.bn.weight"] = (d_xn * xhs).sum((0, 2, 3, 4))
        grads["norm_s.bn.bias"] = d_xn.sum((0, 2, 3, 4))
        dx = dx + norm_backward(d_xn * nsw, xhs, rstds, 16)
    else:
        dx = dx + g
    res["dx"], res["grads"] = dx, grads
    return res


def sgd_outputs(sd, x, z, img, c, cfg, dtype):
    """SGD_STEPS plain SGD steps on the loss sum(c out) in .train() mode: the loss before each step."""
    state = {k: torch.as_tensor(v).to(dtype).clone() for k, v in sd.items()}
    losses = []
    for _ in range(SGD_STEPS):
        r = block(state, x, z, img, cfg, c, train=True, dtype=dtype)
        losses.append(float((c.to(dtype) * r["out"]).sum()))
        for k, g in r["grads"].items():
            state[k] = state[k] - SGD_LR * g
        for k in state:
            if is_buffer(k):
                state[k] = r[k]
    return np.array(losses)


def load_golden():
    """The fixtures' recorded results: every tests/golden/gblock_train_*.npz merged."""
    out = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gblock_train_*.npz"))):
        with np.load(path) as a:
            out.update({k: a[k] for k in a.files})
    return out


def rel(got, ref, scale=None):
    """Relative L2 distance; ``scale``: the tensor whose norm divides instead of the reference's (see ZERO_GRADS)."""
    ref = torch.as_tensor(ref).double()
    den = ref if scale is None else torch.as_tensor(scale).double()
    return float((torch.as_tensor(got).double().reshape(ref.shape) - ref).norm() / den.norm().clamp_min(1e-300))


# conv_0's bias shifts every channel by a constant, which ADAIN's instance norm removes: its gradient is exactly zero, every computed value
# of it is pure cancellation, and a distance relative to the reference's norm means nothing.  Such a tensor is held to the same 1e-4 on
# the scale of what cancels: sum |d_y0| per channel, from the float64 oracle (block()["scale"]).
ZERO_GRADS = ("conv_0.bias",)


# ---------------------------------------------------------------------------------------------------------------- unit oracles
#                C    B  (T, H, W): a Latin square of the channel counts, the batches and the maps
UNIT_CASES = [(16, 1, (1, 4, 4)), (48, 2, (3, 5, 6)), (64, 3, (2, 8, 8)), (128, 1, (3, 5, 6)),
              (16, 2, (2, 8, 8)), (48, 3, (1, 4, 4)), (64, 1, (3, 5, 6)), (128, 2, (1, 4, 4)),
              (16, 3, (3, 5, 6)), (48, 1, (2, 8, 8)), (64, 2, (1, 4, 4)), (128, 3, (2, 8, 8))]
BIG_CASE = (16, 4, (16, 32, 32))   # 65536 rows of 16 channels: the 128-row workgroup form of rows_of


def unit_inputs(seed, C, B, thw, zeros=True):
    """g, act, x [B, T, H, W, C] channels-last fp32; ``zeros``: some exact zeros in act (the LeakyReLU's slope there is 0.2)."""
    rng = np.random.default_rng(seed)
    shp = (B,) + tuple(thw) + (C,)
    g, act, x = (torch.from_numpy(rng.standard_normal(shp).astype(np.float32)) for _ in range(3))
    if zeros:
        act[torch.from_numpy(rng.uniform(size=shp) < 0.1)] = 0.0
    return g, act, x


def modnorm_ref(mode, g, act, x, mod, add=None, slope_at_zero=0.2, plain_gamma=False, unbiased=False, t_mean=False):
    """float64 oracle of the modulated-norm backward on channels-last tensors; mode 0 Spade (mod = gamma [B, H, W, C]), 1 ADAIN (mod = lin
    [B, 2 C]).  -> (dx, dgamma, dbeta, S_dx, (S_dgamma, S_dbeta)): the S are the sums of absolute values behind each result, for the bounds.  The keyword arguments are the
    deliberate errors."""
    g, act, x, mod = g.double(), act.double(), x.double(), mod.double()
    B, T, H, W, C = x.shape
    ga = (g.float() * lrelu_slope(act, slope_at_zero).float()).double()   # fp32, as torch's leaky_relu_backward
    xc = x.permute(0, 4, 1, 2, 3)
    groups = 16 if mode == 0 else C
    xhat, rstd = group_stats(xc, groups, unbiased)
    xhat, rstd = xhat.permute(0, 2, 3, 4, 1), rstd.permute(0, 2, 3, 4, 1)
    if mode == 0:
        m = (mod if plain_gamma else 1 + mod).unsqueeze(1)
        dgamma, dbeta = (ga * xhat).sum(1), ga.sum(1)
        if t_mean:
            dgamma = dgamma / T
    else:
        m = mod[:, :C].view(B, 1, 1, 1, C)
        dgamma, dbeta = torch.cat([(ga * xhat).sum((1, 2, 3)), ga.sum((1, 2, 3))], 1), None
    gp = (ga * m).permute(0, 4, 1, 2, 3)
    xh = xhat.permute(0, 4, 1, 2, 3)
    cpg = C // groups
    m1 = gp.reshape(B, groups, -1).mean(-1).repeat_interleave(cpg, 1).view(B, 1, 1, 1, C)
    m2 = (gp * xh).reshape(B, groups, -1).mean(-1).repeat_interleave(cpg, 1).view(B, 1, 1, 1, C)
    dx = rstd * (ga * m - m1 - xhat * m2)
    S = rstd.abs() * ((ga * m).abs() + m1.abs() + (xhat * m2).abs())
    if add is not None:
        dx, S = dx + add.double(), S + add.double().abs()
    if mode == 0:
        S_maps = ((ga * xhat).abs().sum(1), ga.abs().sum(1))
    else:
        S_maps = (torch.cat([(ga * xhat).abs().sum((1, 2, 3)), ga.abs().sum((1, 2, 3))], 1), None)
    return dx, dgamma, dbeta, S, S_maps


def wgrad1_plan(cout, cin, rows):
    """(slices, slice length) of the 1x1x1 weight gradient: csrc/i2v_gblock_train.hip wgrad1_plan."""
    tiles = (cout // 16) * (cin // 16)
    S = min(max(-(-1024 // tiles), 1), max(-(-rows // 64), 1))
    L = -(-(-(-rows // S)) // 16) * 16
    return -(-rows // L), L


def bn_of(c):
    return 64 if c % 64 == 0 else 32 if c % 32 == 0 else 16


def wgrad_plan(cout, cin, ntap, rows):
    """(slices, slice length) of the trunk's weight gradient: csrc/i2v_train_conv.h wgrad_plan."""
    CP = -(-(4 if cin == 3 else cin) // 16) * 16
    tiles = ntap * (cout // bn_of(cout)) * (CP // bn_of(CP))
    S = min(max(-(-1024 // tiles), 1), max(-(-rows // 64), 1))
    L = -(-(-(-rows // S)) // 16) * 16
    return -(-rows // L), L


def sn_finish_ref(dwn, S_dwn, n, w, u, v, sigma, drop_projection=False):
    """(dW_orig, bound) of the spectral-norm finish from the float64 dW and its element-wise bound gamma(n) S: the projection's inner
    product inherits sum(bound |w|), the four fp32 operations behind it one rounding each."""
    sigma = float(sigma)
    b_dwn = gamma(n) * S_dwn + U * dwn.abs()
    proj = float((dwn * w).sum()) / sigma
    uv = torch.outer(u, v).view_as(dwn)
    ref = dwn / sigma if drop_projection else (dwn - proj * uv) / sigma
    b_proj = float((b_dwn * w.abs()).sum()) / abs(sigma) + U * abs(proj)
    bound = (b_dwn + b_proj * uv.abs() + gamma(5) * (dwn.abs() + abs(proj) * uv.abs())) / abs(sigma)
    return ref, bound
