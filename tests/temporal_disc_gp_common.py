"""Shared by tests/test_host_temporal_disc_gp.py, tests/test_gpu_temporal_disc_gp.py and tests/test_gpu_temporal_disc_gp_hygiene.py: the
gradient of the temporal discriminator's gradient penalty in float64 on the CPU, WRITTEN OUT BY HAND on the ``cache`` of
``temporal_disc_common.forward_oracle`` -- a tangent forward and a reverse pass over the pair (primal, tangent), no autograd -- so that the
ReLU masks and the pool's argmaxes can be given and single deliberate errors switched on; plus the unit oracles of the new kernels with
their bounds.  Nothing of the package is imported.

The method: P = mean_b pred_b, g = grad_x P, L_GP = (1 / n) sum_b |g_b|^2.  With v = (2 s / n) g held constant (s: the
scale, w_GP), s grad_theta L_GP = grad_theta Pdot, Pdot the directional derivative of P along v: a tangent forward with x' = v on the
primal's decisions and statistics, then one reverse pass over (primal, tangent) seeded with adjoint(Pdot) = 1, adjoint(P) = 0.  u and v of
the spectral norm are constants; sigma depends on weight_orig through the projection, applied once to the SUM of the two members' dWn.

GroupNorm per (sample, group) of m elements: xh = (x - mu) r, M(a) = mean(a), C(a) = mean(xh a), Pi(a) = a - M(a) - xh C(a), p = w yb',
q = w yb (yb, yb': the adjoints at the primal and at the tangent output):
  tangent   xh' = r Pi(x'), y' = w xh'
  xb'       = r Pi(p)
  xb        = r Pi(q) - r^2 [xh mean(p Pi(x')) + C(x') Pi(p) + C(p) Pi(x')]
  wb        = sum yb xh + sum yb' xh',   bb = sum yb

Bounds of the unit oracles, in the style of temporal_disc_common: |err| <= gamma(n) S + 2^-24 |ref|, n the length of the chain of fp32
roundings, S the sum of the absolute terms that pass through them.  The kernels read fp32 operands, form every sum (M, C, the five
channel sums, the group sums) in float64 -- error ~ 2^-53 m, nothing against 2^-24 -- and evaluate each output element in float64:
  GN tangent  out = fl(fl(r Pi(x')) * w) (+ res'): the float64 value of r Pi(x') is rounded once, the product once, the add once:
              n = 3, S = |r Pi(x') w| + |res'|.  tstats are float64: compared at 1e-12 relative to mean |x'| resp. mean |xh x'|.
  dxd         = fl(r Pi(p)), one rounding of a float64 expression whose three terms cancel: n = 1 on the terms,
              S = r (|p| + |M(p)| + |xh C(p)|)
  dx          = fl(r Pi(q) - r^2 [...]), one rounding: n = 1,
              S = r (|q| + |M(q)| + |xh C(q)|) + r^2 (|xh K| + |C(x')| (|p| + |M(p)| + |xh C(p)|) + |C(p)| (|x'| + |M(x')| + |xh C(x')|))
  dweight     one rounding of a float64 sum: n = 1, S = sum |yb xh| + sum |yb'| r (|x'| + |M(x')| + |xh C(x')|);  dbias: n = 1, S = sum |yb|
  (gamma(1) S covers the last-place error of the float64 arithmetic on cancelling terms many times over; the term 2^-24 |ref| is the
  rounding itself.)
  pool gather compared bit for bit.
  head        pdot: 16 fp32 adds and an exact scaling, then a float64 dot product rounded once: n = 17, S = sum |mean| |w|;
              dxd = fl(fl(s / n) * fl(w / 16)): n = 2 (the division s / n rounds once, the product once), S = |ref|;
              dweight = float64 sum over the batch of fl(s / n) times the fp32 pooled mean, rounded once: n = 18, S = (s / n) sum mean |x'|
              dx = 0 exactly."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv3d_input, conv3d_weight

import temporal_disc_common as tc
from temporal_disc_common import U, gamma  # noqa: F401

MUTATIONS = ("second_order_dropped", "tangent_relu_mask_dropped", "pool_gather_first_element", "gamma_without_tangent", "seed_one_over_n",
             "projection_one_member", "head_weight_dropped")
# every one of them shows in the module on fixture B (tests/test_host_temporal_disc_gp.py asserts it), so none needs its unit's gate
W_GP = 10.0


def _g16(a):
    return a.reshape(a.shape[0], 16, -1)


def gn_tangent(c, yd):
    """c: a conv entry of the cache (xhat, rstd, gw); yd: the tangent of the conv's output -> (tangent of the norm's output, entry)"""
    xh, a = _g16(c["xhat"]), _g16(yd)
    M, C = a.mean(2, keepdim=True), (xh * a).mean(2, keepdim=True)
    pi = a - M - xh * C
    xhd = (c["rstd"].reshape(-1, 16, 1) * pi).reshape(yd.shape)
    return xhd * c["gw"].view(1, -1, 1, 1, 1), dict(xd=yd, M=M, C=C, pi=pi, xhd=xhd)


def gn_dual_backward(c, t, yb, ybd, mutate=None):
    """-> (xb, xbd, dweight, dbias): the adjoints at the conv's output and at its tangent, and the norm's parameter gradients"""
    w = c["gw"].view(1, -1, 1, 1, 1)
    dw = (yb * c["xhat"]).sum((0, 2, 3, 4))
    if mutate != "gamma_without_tangent":
        dw = dw + (ybd * t["xhd"]).sum((0, 2, 3, 4))
    db = yb.sum((0, 2, 3, 4))
    xh, r = _g16(c["xhat"]), c["rstd"].reshape(-1, 16, 1)
    p, q = _g16(ybd * w), _g16(yb * w)

    def proj(a):
        return a - a.mean(2, keepdim=True) - xh * (xh * a).mean(2, keepdim=True)

    Cp = (xh * p).mean(2, keepdim=True)
    pip, piq = proj(p), proj(q)
    xbd = r * pip
    xb = r * piq
    if mutate != "second_order_dropped":
        K = (p * t["pi"]).mean(2, keepdim=True)
        xb = xb - r * r * (xh * K + t["C"] * pip + Cp * t["pi"])
    return xb.reshape(yb.shape), xbd.reshape(yb.shape), dw, db


def tangent_forward(cache, xd, mutate=None):
    """xd [N, 3, T, H, W]: the tangent clip -> tcache (per conv key the entries of gn_tangent plus ``a``: the tangent of the conv's input,
    ``out``: the tangent of the activation; ``pool``: the tangent of the pool's output; ``top``: the tangent of the last activation)"""
    zero = torch.zeros((), dtype=xd.dtype)
    T = {}

    def conv_norm(c, ad):
        yd = F.conv3d(ad, c["Wn"], stride=c["strides"], padding=c["pads"])
        out, e = gn_tangent(c, yd)
        e["a"] = ad
        T[c["key"]] = e
        return out, e

    def masked(mask, a):
        return a if mutate == "tangent_relu_mask_dropped" else torch.where(mask, a, zero)

    stem = cache["stem"]
    h, e = conv_norm(stem, xd)
    h = masked(stem["mask"], h)
    e["out"] = h
    if cache["pool"] is not None:
        idx = cache["pool"]["idx"]
        flat = h.reshape(*h.shape[:2], -1)
        if mutate == "pool_gather_first_element":   # the window's first element in (t, h, w) scan order, clamped into the map
            _, _, Tn, Hn, Wn_ = h.shape
            to, ho, wo = torch.meshgrid(torch.arange(idx.shape[2]), torch.arange(idx.shape[3]), torch.arange(idx.shape[4]), indexing="ij")
            first = ((to - 1).clamp_min(0) * Hn + (2 * ho - 1).clamp_min(0)) * Wn_ + (2 * wo - 1).clamp_min(0)
            idx = first.view(1, 1, *first.shape).expand_as(idx).contiguous()
        h = flat.gather(2, idx.reshape(*idx.shape[:2], -1)).reshape(idx.shape)
        T["pool"] = h
    for st in cache["steps"]:
        xin = h
        h1, e1 = conv_norm(st["c1"], xin)
        h1 = masked(st["c1"]["mask"], h1)
        e1["out"] = h1
        h2, e2 = conv_norm(st["c2"], h1)
        res = xin
        if st["cd"] is not None:
            res, ed = conv_norm(st["cd"], xin)
            ed["out"] = res
        h = masked(st["mask"], h2 + res)
        e2["out"] = h
    T["top"] = h
    return T


def dual_backward(cache, T, s=1.0, mutate=None):
    """The reverse pass over (primal, tangent) for Pdot = (s / n) sum_b fc . avg(a'_b) -> {state_dict key: gradient}"""
    dtype, grads = cache["dtype"], {}
    zero = torch.zeros((), dtype=dtype)
    N = cache["top"][0]
    grads["fc.weight"] = (s / N) * T["top"].mean((2, 3, 4)).sum(0, keepdim=True)
    if mutate == "head_weight_dropped":
        grads["fc.weight"] = torch.zeros_like(grads["fc.weight"])
    gd = (s * cache["fc"] / (16.0 * N)).view(1, -1, 1, 1, 1).expand(cache["top"]).clone()
    g = torch.zeros_like(gd)

    def conv_bwd(c, t, yb, ybd, need_dx=True):
        kw = dict(stride=c["strides"], padding=c["pads"])
        d0, d1 = conv3d_weight(c["x"], c["W"].shape, yb, **kw), conv3d_weight(t["a"], c["W"].shape, ybd, **kw)
        if c["u"] is None:
            grads[c["key"]] = (d0 + d1) / c["sigma"]
        else:
            def proj(d):
                return (d - (d * c["Wn"]).sum() * torch.outer(c["u"], c["v"]).view_as(d)) / c["sigma"]
            grads[c["key"]] = proj(d0) + d1 / c["sigma"] if mutate == "projection_one_member" else proj(d0 + d1)
        if not need_dx:
            return None, None
        return conv3d_input(c["x"].shape, c["Wn"], yb, **kw), conv3d_input(c["x"].shape, c["Wn"], ybd, **kw)

    def norm_conv_bwd(c, yb, ybd, need_dx=True):
        t = T[c["key"]]
        xb, xbd, dw, db = gn_dual_backward(c, t, yb, ybd, mutate)
        grads[c["nkey"] + ".weight"], grads[c["nkey"] + ".bias"] = dw, db
        return conv_bwd(c, t, xb, xbd, need_dx)

    for st in reversed(cache["steps"]):
        g, gd = torch.where(st["mask"], g, zero), torch.where(st["mask"], gd, zero)
        h1, h1d = norm_conv_bwd(st["c2"], g, gd)
        h1, h1d = torch.where(st["c1"]["mask"], h1, zero), torch.where(st["c1"]["mask"], h1d, zero)
        dx, dxd = norm_conv_bwd(st["c1"], h1, h1d)
        if st["cd"] is not None:
            rx, rxd = norm_conv_bwd(st["cd"], g, gd)
            dx, dxd = dx + rx, dxd + rxd
        else:
            dx, dxd = dx + g, dxd + gd
        g, gd = dx, dxd
    if cache["pool"] is not None:
        idx, shp = cache["pool"]["idx"], cache["pool"]["in_shape"]
        flat_idx = idx.reshape(*idx.shape[:2], -1)

        def scatter(a):
            return torch.zeros(*shp[:2], int(np.prod(shp[2:])), dtype=dtype).scatter_add_(2, flat_idx, a.reshape(*a.shape[:2], -1)).reshape(shp)
        g, gd = scatter(g), scatter(gd)
    stem = cache["stem"]
    g, gd = torch.where(stem["mask"], g, zero), torch.where(stem["mask"], gd, zero)
    norm_conv_bwd(stem, g, gd, need_dx=False)
    return grads


def penalty_oracle(sd, x, cfg, scale=1.0, decisions=None, mutate=None, training=True):
    """-> dict(l_gp, grads: {key: scale * d L_GP / d parameter}, T: the tangent cache, cache, g: the gradient at the clips, xd: the tangent
    clip (2 scale / n) g).  One forward (it iterates the spectral norm when ``training``), by hand throughout."""
    pred, _, cache = tc.forward_oracle(sd, x, cfg, training=training, decisions=decisions)
    n = pred.shape[0]
    _, g = tc.backward_oracle(cache, torch.full_like(pred, 1.0 / n))
    l_gp = g.pow(2).reshape(n, -1).sum(1).mean()
    xd = ((1.0 if mutate == "seed_one_over_n" else 2.0) * scale / n) * g
    T = tangent_forward(cache, xd, mutate)
    return dict(l_gp=l_gp, grads=dual_backward(cache, T, 1.0, mutate), T=T, cache=cache, g=g, xd=xd, pred=pred)


def penalty_autograd(sd, x, cfg, scale=1.0, decisions=None, training=True):
    """The same through torch's float64 double backward over ``forward_oracle`` (autograd-compatible, also with given decisions)
    -> (l_gp, {key: gradient or None})"""
    if training:   # torch iterates u and v under no_grad: they are constants of the graph, sigma = u . (W v) is not
        with torch.no_grad():
            sd = dict(sd, **tc.forward_oracle(sd, x, cfg, training=True, decisions=decisions)[2]["state"])
    leaves = {k: v.double().clone().requires_grad_(not k.endswith(("weight_u", "weight_v"))) for k, v in sd.items()}
    xr = x.double().clone().requires_grad_(True)
    pred, _, _ = tc.forward_oracle(leaves, xr, cfg, training=False, decisions=decisions)
    g = torch.autograd.grad(pred.mean(), xr, create_graph=True)[0]
    l_gp = g.pow(2).reshape(x.shape[0], -1).sum(1).mean()
    keys = [k for k, v in leaves.items() if v.requires_grad]
    out = torch.autograd.grad(scale * l_gp, [leaves[k] for k in keys], allow_unused=True)
    return l_gp.detach(), dict(zip(keys, out))


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- unit oracles

GN_CASES = [{"id": f"c{c}-{'x'.join(map(str, thw))}-b{b}", "c": c, "thw": thw, "batch": b, "seed": 71000 + 10 * i}
            for i, (c, thw, b) in enumerate(((16, (1, 4, 4), 1), (16, (2, 5, 7), 3), (48, (1, 4, 4), 3), (48, (2, 5, 7), 1), (16, (3, 8, 8), 3),
                                             (48, (3, 8, 8), 1),
                                             (48, (4, 41, 39), 1),      # 6396 positions: 4 slices in the tangent's statistics, 24 ragged ones in the backward
                                             (64, (16, 64, 64), 1)))]   # 65536 positions x 4 per group: the maximal slice count (32) in both passes


def gn_slices(positions, per_row):
    """csrc/i2v_res3d_trunk.h gn_slices, restated so that the tests can say which slice counts they ran"""
    return int(min(max(positions * per_row // 4096, 1), 32))


def gn_case_inputs(case):
    """-> (x, xd, resd, act, g, gd, w, b) fp32 [N, C, T, H, W] / [C]; ``act`` decides the mask (act > 0)"""
    shape, s = (case["batch"], case["c"]) + tuple(case["thw"]), case["seed"]
    x = tc.randn(s, shape) * 1.5 + 0.3
    w, b = 1.0 + 0.2 * tc.randn(s + 6, (case["c"],)), 0.1 * tc.randn(s + 7, (case["c"],))
    return x, tc.randn(s + 1, shape), tc.randn(s + 2, shape), tc.randn(s + 3, shape), tc.randn(s + 4, shape), tc.randn(s + 5, shape), w, b


def _gn_entry(x, w):
    x = x.double()
    _, xhat, rstd = tc.group_norm(x, w.double(), torch.zeros_like(w).double())
    return dict(xhat=xhat, rstd=rstd, gw=w.double())


def gn_tangent_oracle(x, xd, w, resd=None, mask=None, mutate=None):
    """-> (ref, bound, M [N, 16], C [N, 16]) in float64"""
    c = _gn_entry(x, w)
    out, e = gn_tangent(c, xd.double())
    S = out.abs()
    if resd is not None:
        out, S = out + resd.double(), S + resd.double().abs()
    if mask is not None and mutate != "tangent_relu_mask_dropped":
        out, S = out * mask, S * mask
    return out, gamma(3) * S + U * out.abs(), e["M"].reshape(-1, 16), e["C"].reshape(-1, 16)


def gn_dual_oracle(g, gd, x, xd, w, mask=None, mutate=None):
    """-> {name: (ref, bound)} for dx, dxd, dweight, dbias in float64"""
    c = _gn_entry(x, w)
    _, t = gn_tangent(c, xd.double())
    yb, ybd = g.double(), gd.double()
    if mask is not None:
        yb, ybd = yb * mask, ybd * mask
    xb, xbd, dw, db = gn_dual_backward(c, t, yb, ybd, mutate)
    wv = c["gw"].view(1, -1, 1, 1, 1)
    xh, r = _g16(c["xhat"]), c["rstd"].reshape(-1, 16, 1)
    p, q, a = _g16(ybd * wv), _g16(yb * wv), _g16(xd.double())

    def absproj(v):
        return v.abs() + v.mean(2, keepdim=True).abs() + (xh * (xh * v).mean(2, keepdim=True)).abs()

    Cp, K = (xh * p).mean(2, keepdim=True), (p * t["pi"]).mean(2, keepdim=True)
    S_xbd = r * absproj(p)
    S_xb = r * absproj(q) + r * r * ((xh * K).abs() + t["C"].abs() * absproj(p) + Cp.abs() * absproj(a))
    S_dw = (yb * c["xhat"]).abs().sum((0, 2, 3, 4)) + (_g16(ybd).abs() * r * absproj(a)).reshape(yb.shape).sum((0, 2, 3, 4))
    S_db = yb.abs().sum((0, 2, 3, 4))
    return {"dx": (xb, gamma(1) * S_xb.reshape(xb.shape) + U * xb.abs()), "dxd": (xbd, gamma(1) * S_xbd.reshape(xb.shape) + U * xbd.abs()),
            "dweight": (dw, gamma(1) * S_dw + U * dw.abs()), "dbias": (db, gamma(1) * S_db + U * db.abs())}


def head_dual_oracle(xd, w, s):
    """xd [N, C, 1, 4, 4], w [1, C] -> {name: (ref, bound)} for pdot [N, 1], dxd, dweight [1, C]; dx is zero exactly"""
    xd, w = xd.double(), w.double()
    n = xd.shape[0]
    mean, amean = xd.mean((2, 3, 4)), xd.abs().mean((2, 3, 4))
    pdot = mean @ w.t()
    S_p = amean @ w.abs().t()
    dxd = (s * w / (16.0 * n)).view(1, -1, 1, 1, 1).expand(xd.shape)
    dw = (s / n) * mean.sum(0, keepdim=True)
    S_w = (abs(s) / n) * amean.sum(0, keepdim=True)
    return {"pdot": (pdot, gamma(17) * S_p + U * pdot.abs()), "dxd": (dxd, gamma(2) * dxd.abs() + U * dxd.abs()),
            "dweight": (dw, gamma(18) * S_w + U * dw.abs())}


def pool_tangent_oracle(xd, argmax):
    """xd [N, C, T, H, W], argmax int64 [N, C, T, Ho, Wo] -> the gathered values, exact"""
    return xd.reshape(*xd.shape[:2], -1).gather(2, argmax.reshape(*argmax.shape[:2], -1)).reshape(argmax.shape)
