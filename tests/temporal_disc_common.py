"""Shared by tests/test_host_temporal_disc.py, tests/test_gpu_temporal_disc.py and tests/golden/make_golden_temporal_disc.py: a float64
restatement of the temporal discriminator (reference stage1_VAE/modules/resnet3D.py:222-301) in functional torch on the CPU -- forward with
spectral norm in training mode, and a BACKWARD WRITTEN OUT BY HAND (not autograd), so that the ReLU masks and the pool's argmaxes can be
given and single deliberate errors switched on -- plus the unit oracles with their bounds and the inputs of the fixtures.  Nothing of the
package is imported.

The gate is the project's (``i3d_units_common.gate``): |got - ref64| <= gamma(n) S + 2^-24 |ref64| element-wise, with n the length of the
summation chain and S the same sum over absolute products, and relative L2 <= 1e-4 per batch row.
  conv forward   n = kt kh kw Cin, S = conv(|x|, |w|)
  dgrad          n = (taps of the position's parity class) Cout, per position: along an axis of stride 2 one tap (window 3) or three
                 (window 7) for an even coordinate, two or four for an odd one, all taps at stride 1 (+1 where a residual is added,
                 which then joins S)
  wgrad          n = positions; the kernel adds quarter-slices, then slices: any order of n terms has error <= gamma(n) S
  projection     as in patch_disc_common: the bound of dWn, plus gamma(4) |p u v^T| for the float64 dot product rounded once and the two
                 products, all divided by sigma, plus one rounding for the division
  GroupNorm fwd  statistics are float64 sums of exact fp32 values (error ~ 2^-53 m, nothing against 2^-24); per element xhat is formed
                 in float64 and rounded once, then one fma with weight and bias, one add of the residual: n = 3,
                 S = |xhat w| + |b| + |res|
  GroupNorm bwd  dweight / dbias: float64 sums rounded once: n = 1, S = |ref|.  dx = rstd (dy w - s1 / m - xhat s2 / m) in float64
                 from fp32 operands, rounded once: n = 2 (the mask multiplies dy exactly), S = rstd (|dy w| + |s1| / m + |xhat s2| / m)
  max pool       compared bit for bit; its backward adds at most 2 x 2 x 3 = 12 windows: n = 12, S = sum |g|
  head           pooled mean: 16 fp32 adds and an exact scaling, then a float64 dot product rounded once: n = 17, S = sum |mean| |w|;
                 dx = g w / 16: n = 2; dweight: float64 sum over the batch of g times the fp32 pooled mean: n = 17, S = sum |g| mean|x|
  fmap loss, sum of squares: float64 sums of fp32 differences / squares: compared at 1e-12 relative (the fp32 subtraction is exact to
                 one rounding, which the float64 reference reproduces by subtracting the same fp32 values in fp32)
Spectral norm: W viewed as [Cout, Cin 27]; v <- normalize(W^T u), u <- normalize(W v) with eps 1e-12, sigma = u . (W v), the conv uses
W / sigma; dW_orig = (dWn - <dWn, Wn> u v^T) / sigma with the u, v AFTER the iteration."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv3d_input, conv3d_weight

from i3d_units_common import U, TOL_L2, gamma, gate, gate_bound, randn, rel_l2_rows  # noqa: F401  (the gate is reused by import)
from patch_disc_common import hinge_disc, hinge_disc_grads, power_iteration  # noqa: F401

FRAGILE_REL, FRAGILE_MAX = 1e-5, 4
SGD_LR, SGD_STEPS = 1e-3, 6
CFG_A = {"res_type_encoder": "resnet18", "use_max_pool": True, "spectral_norm": True, "channels": [16, 16, 16, 32, 32], "stride_t": [2, 2, 2, 2],
         "stride_s": [1, 1, 2, 2]}
CFG_B = {"res_type_encoder": "resnet18", "use_max_pool": True, "spectral_norm": True, "channels": [16, 32, 32, 48, 48], "stride_t": [2, 1, 2, 1],
         "stride_s": [1, 2, 1, 1]}
CFG_C = dict(CFG_B, use_max_pool=False)
CFG_SHIPPED = {"res_type_encoder": "resnet18", "use_max_pool": True, "spectral_norm": True, "channels": [64, 64, 128, 256, 512],
               "stride_t": [2, 2, 2, 2], "stride_s": [1, 1, 2, 2]}
SEED_A, SEED_A_DATA, SEED_B, SEED_B_DATA, SEED_C_DATA = 5100, 5101, 5200, 5201, 5301
MUTATIONS = ("taps_not_flipped", "wrong_parity", "projection_dropped", "u_before_iteration", "block1_spectral", "gn_no_mean_terms",
             "residual_one_branch", "downsample_without_stride_t")


def clips_a():
    """(fake, real) [2, 3, 12, 64, 64] fp32 of fixture A: drawn in float64 and rounded to fp32 once."""
    g = torch.Generator().manual_seed(SEED_A_DATA)
    real = torch.randn(2, 3, 12, 64, 64, generator=g, dtype=torch.float64)
    fake = 0.5 * torch.randn(2, 3, 12, 64, 64, generator=g, dtype=torch.float64) + 0.3
    return fake.float(), real.float()


def clips_a_eval(t):
    return randn(SEED_A_DATA + 10 + t, (2, 3, t, 64, 64))


def clips_b():
    return randn(SEED_B_DATA, (3, 3, 4, 32, 32))


def clips_c():
    return randn(SEED_C_DATA, (3, 3, 4, 16, 16))


def upstream_b():
    """The upstream gradients of fixture B: d_pred [3, 1] and one per feature map (shapes from the config at 4 x 32 x 32)."""
    shapes = [(3, 32, 2, 8, 8), (3, 32, 2, 4, 4), (3, 48, 1, 4, 4), (3, 48, 1, 4, 4)]
    return randn(SEED_B_DATA + 1, (3, 1)), [randn(SEED_B_DATA + 2 + i, s) for i, s in enumerate(shapes)]


def blocks(cfg):
    """The eight BasicBlocks: state-dict prefix, widths, strides, which convs are spectral-normed, whether a downsample branch exists."""
    out, inplanes = [], cfg["channels"][0]
    for l, planes in enumerate(cfg["channels"][1:]):
        ss, st = cfg["stride_s"][l], cfg["stride_t"][l]
        out.append(dict(prefix=f"layer.{l}.0.", cin=inplanes, cout=planes, st=st, ss=ss, sn=bool(cfg["spectral_norm"]),
                        ds=ss != 1 or inplanes != planes or st != 1, layer=l, last=False))
        out.append(dict(prefix=f"layer.{l}.1.", cin=planes, cout=planes, st=1, ss=1, sn=False, ds=False, layer=l, last=True))
        inplanes = planes
    return out


def state_keys(cfg):
    """{key: (shape, dtype)} of Discriminator(cfg).state_dict(), in the reference's order."""
    out = {"conv1.weight": ((cfg["channels"][0], 3, 3, 7, 7), torch.float32), "norm1.weight": ((cfg["channels"][0],), torch.float32),
           "norm1.bias": ((cfg["channels"][0],), torch.float32)}

    def conv(key, cin, cout, sn):
        if sn:
            out[key + ".weight_orig"] = ((cout, cin, 3, 3, 3), torch.float32)
            out[key + ".weight_u"] = ((cout,), torch.float32)
            out[key + ".weight_v"] = ((cin * 27,), torch.float32)
        else:
            out[key + ".weight"] = ((cout, cin, 3, 3, 3), torch.float32)

    def norm(key, c):
        out[key + ".weight"] = ((c,), torch.float32)
        out[key + ".bias"] = ((c,), torch.float32)

    for b in blocks(cfg):
        p = b["prefix"]
        conv(p + "conv1", b["cin"], b["cout"], b["sn"]); norm(p + "bn1", b["cout"])
        conv(p + "conv2", b["cout"], b["cout"], b["sn"]); norm(p + "bn2", b["cout"])
        if b["ds"]:
            conv(p + "downsample.0", b["cin"], b["cout"], True); norm(p + "downsample.1", b["cout"])
    out["fc.weight"] = ((1, cfg["channels"][4]), torch.float32)
    return out


def synthetic_state(cfg, seed):
    """A seeded state dict (numpy draws, platform-stable) for fixtures whose parameters are not stored: conv weights of fan-in scale, u and
    v of unit length, GroupNorm weights around 1 and biases around 0."""
    sd = {}
    for i, (k, (shape, _)) in enumerate(state_keys(cfg).items()):
        x = randn(seed + i, shape)
        if k.endswith(("weight_u", "weight_v")):
            x = x / x.norm()
        elif len(shape) == 5:
            x = x * float(np.sqrt(2.0 / (shape[1] * shape[2] * shape[3] * shape[4])))
        elif k == "fc.weight":
            x = x * float(np.sqrt(1.0 / shape[1]))
        elif k.endswith("bias"):
            x = 0.1 * x
        else:
            x = 1.0 + 0.2 * x
        sd[k] = x.float().contiguous()
    return sd


# ---------------------------------------------------------------------------------------------------------------- the network, by hand

def group_norm(x, w, b, eps=1e-5):
    """GroupNorm(16) on x [N, C, T, H, W] -> (y, xhat, rstd [N, 16])"""
    N, C = x.shape[:2]
    g = x.reshape(N, 16, -1)
    mean, var = g.mean(2, keepdim=True), g.var(2, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((g - mean) * rstd).reshape(x.shape)
    return xhat * w.view(1, -1, 1, 1, 1) + b.view(1, -1, 1, 1, 1), xhat, rstd.reshape(N, 16)


def group_norm_backward(dy, xhat, rstd, w, mutate=None):
    """dy at the norm's output -> (dx, dweight, dbias)"""
    N, C = dy.shape[:2]
    dw, db = (dy * xhat).sum((0, 2, 3, 4)), dy.sum((0, 2, 3, 4))
    dyw = (dy * w.view(1, -1, 1, 1, 1)).reshape(N, 16, -1)
    xh = xhat.reshape(N, 16, -1)
    m = dyw.shape[2]
    s1, s2 = dyw.sum(2, keepdim=True), (dyw * xh).sum(2, keepdim=True)
    inner = dyw if mutate == "gn_no_mean_terms" else dyw - s1 / m - xh * s2 / m
    return (rstd.reshape(N, 16, 1) * inner).reshape(dy.shape), dw, db


def dgrad_taps(dy, W, in_shape, strides, mutate=None):
    """Input gradient of conv3d(., W, strides, padding = k // 2) tap by tap: dx[i = o s - p + k] += dy[o] . W[:, :, k].  Equal to
    torch.nn.grad.conv3d_input (checked by the host test); ``mutate`` switches one deliberate error on."""
    N, Co = dy.shape[:2]
    ks, pads = W.shape[2:], [k // 2 for k in W.shape[2:]]
    big = torch.zeros(N, W.shape[1], *[n + 2 * k for n, k in zip(in_shape, ks)], dtype=dy.dtype)
    for kt in range(ks[0]):
        for kh in range(ks[1]):
            for kw in range(ks[2]):
                wt, wh, ww = kt, kh, kw
                if mutate == "taps_not_flipped":
                    wt, wh, ww = ks[0] - 1 - kt, ks[1] - 1 - kh, ks[2] - 1 - kw
                if mutate == "wrong_parity":   # the taps of the other parity class, along every strided axis
                    wt, wh, ww = [(k + 1) % n if s == 2 else k for k, n, s in zip((kt, kh, kw), ks, strides)]
                c = torch.einsum("nothw,oi->nithw", dy, W[:, :, wt, wh, ww])
                sl = [slice(k + n - p, k + n - p + s * o, s) for k, n, p, s, o in zip((kt, kh, kw), ks, pads, strides, dy.shape[2:])]
                big[:, :, sl[0], sl[1], sl[2]] += c
    return big[:, :, ks[0]: ks[0] + in_shape[0], ks[1]: ks[1] + in_shape[1], ks[2]: ks[2] + in_shape[2]]


def class_taps(in_shape, ks, strides):
    """Per input position [1, 1, T, H, W] the number of taps of its parity class: along an axis of window k, pad k // 2 and stride s the
    taps kk = (i + k // 2) mod s + s j < k."""
    out = torch.ones(1, 1, 1, 1, 1, dtype=torch.float64)
    for axis, (n, k, s) in enumerate(zip(in_shape, ks, strides)):
        kb = (torch.arange(n) + k // 2) % s
        cnt = ((k - kb + s - 1) // s).double()
        out = out * cnt.view([1, 1] + [n if a == axis else 1 for a in range(3)])
    return out


def _conv_params(sd, key, training, state, dtype, as_if_spectral=False):
    """-> dict(W, Wn, u, v, u0, sigma, key) of the conv under ``key``"""
    if key + ".weight" in sd:
        W = sd[key + ".weight"].to(dtype)
        sigma = torch.ones((), dtype=dtype)
        if as_if_spectral:
            sigma = torch.linalg.matrix_norm(W.reshape(W.shape[0], -1).double(), 2).to(dtype)
        return dict(W=W, Wn=W / sigma, u=None, v=None, u0=None, sigma=sigma, key=key + ".weight")
    W = sd[key + ".weight_orig"].to(dtype)
    u0, v0 = sd[key + ".weight_u"].to(dtype), sd[key + ".weight_v"].to(dtype)
    u, v, sigma = power_iteration(W.reshape(W.shape[0], -1), u0, v0, iterate=training)
    state[key + ".weight_u"], state[key + ".weight_v"] = u, v
    return dict(W=W, Wn=W / sigma, u=u, v=v, u0=u0, sigma=sigma, key=key + ".weight_orig")


def forward_oracle(sd, x, cfg, training, dtype=torch.float64, decisions=None, mutate=None):
    """sd: {state_dict key: tensor}; x [N, 3, T, H, W].  -> (pred [N, 1], [fmap0 .. fmap3], cache).  ``decisions``: {name: tensor} of ReLU
    masks (bool, per norm key) and of the pool's argmax ("pool": int64 [N, C, T, Ho, Wo], flat (t H + h) W + w) to use instead of this
    pass's own.  cache["state"] holds the updated u, v; cache["decisions"] the decisions taken; cache["margins"] the values they were
    taken on."""
    x = x.to(dtype)
    state, dec, margins, steps = {}, {}, {}, []
    given = decisions or {}

    def relu(name, h):
        mask = given.get(name, h > 0)
        dec[name], margins[name] = mask, h
        return torch.where(mask, h, torch.zeros((), dtype=dtype)), mask

    def conv_norm(ckey, nkey, xin, strides, pads, as_if=False):
        c = _conv_params(sd, ckey, training, state, dtype, as_if)
        y = F.conv3d(xin, c["Wn"], stride=strides, padding=pads)
        w, b = sd[nkey + ".weight"].to(dtype), sd[nkey + ".bias"].to(dtype)
        h, xhat, rstd = group_norm(y, w, b)
        c.update(x=xin, y=y, xhat=xhat, rstd=rstd, gw=w, nkey=nkey, strides=strides, pads=pads)
        return h, c

    h, stem = conv_norm("conv1", "norm1", x, (1, 2, 2), (1, 3, 3))
    h, stem["mask"] = relu("norm1", h)
    pool = None
    if cfg["use_max_pool"]:
        if "pool" in given:
            idx = given["pool"]
            out = h.reshape(*h.shape[:2], -1).gather(2, idx.reshape(*idx.shape[:2], -1)).reshape(idx.shape)
        else:
            out, idx = F.max_pool3d(h, 3, (1, 2, 2), 1, return_indices=True)
        pool = dict(idx=idx, in_shape=h.shape)
        dec["pool"], margins["pool"] = idx, h
        h = out
    fmaps = []
    for b in blocks(cfg):
        p, xin = b["prefix"], h
        as_if = mutate == "block1_spectral" and b["last"]
        h1, c1 = conv_norm(p + "conv1", p + "bn1", xin, (b["st"], b["ss"], b["ss"]), (1, 1, 1), as_if)
        h1, c1["mask"] = relu(p + "bn1", h1)
        h2, c2 = conv_norm(p + "conv2", p + "bn2", h1, (1, 1, 1), (1, 1, 1), as_if)
        cd, res = None, xin
        has_ds = b["ds"]
        if mutate == "downsample_without_stride_t":
            has_ds = b["ss"] != 1 or b["cin"] != b["cout"]
        if has_ds:
            res, cd = conv_norm(p + "downsample.0", p + "downsample.1", xin, (b["st"], b["ss"], b["ss"]), (1, 1, 1))
        elif b["ds"]:
            res = xin[:, :, ::b["st"]]          # (the mutation: an identity residual where the stride_t rule builds a branch)
        h, mask = relu(p + "bn2", h2 + res)
        steps.append(dict(block=b, c1=c1, c2=c2, cd=cd, mask=mask, x=xin))
        if b["last"]:
            fmaps.append(h)
    pooled = h.mean((2, 3, 4)) if h.shape[2:] == (1, 4, 4) else None
    assert pooled is not None, f"the network ends on a {tuple(h.shape[2:])} map"
    fc = sd["fc.weight"].to(dtype)
    pred = pooled @ fc.t()
    return pred, fmaps, dict(steps=steps, stem=stem, pool=pool, state=state, decisions=dec, margins=margins, pooled=pooled, fc=fc, top=h.shape,
                             dtype=dtype)


def _conv_backward(c, dy, grads, mutate, need_dx=True):
    """dy at the conv's output -> dx at its input; the weight gradient goes into ``grads``"""
    dWn = conv3d_weight(c["x"], c["W"].shape, dy, stride=c["strides"], padding=c["pads"])
    if c["u"] is None:
        grads[c["key"]] = dWn / c["sigma"]          # (sigma is 1 unless the as-if-spectral mutation is on)
    else:
        u = c["u0"] if mutate == "u_before_iteration" else c["u"]
        proj = 0.0 if mutate == "projection_dropped" else (dWn * c["Wn"]).sum() * torch.outer(u, c["v"]).view_as(dWn)
        grads[c["key"]] = (dWn - proj) / c["sigma"]
    if not need_dx:
        return None
    if mutate in ("taps_not_flipped", "wrong_parity"):
        return dgrad_taps(dy, c["Wn"], c["x"].shape[2:], c["strides"], mutate)
    return conv3d_input(c["x"].shape, c["Wn"], dy, stride=c["strides"], padding=c["pads"])


def _norm_conv_backward(c, g, grads, mutate, need_dx=True):
    dy, dw, db = group_norm_backward(g, c["xhat"], c["rstd"], c["gw"], mutate)
    grads[c["nkey"] + ".weight"], grads[c["nkey"] + ".bias"] = dw, db
    return _conv_backward(c, dy, grads, mutate, need_dx)


def backward_oracle(cache, d_pred, d_fmaps=None, mutate=None):
    """-> ({state_dict key: gradient}, dx [N, 3, T, H, W]) for the upstream gradients d_pred [N, 1] (or None) and d_fmaps (None, or a
    list of four tensors / None), by hand."""
    dtype, grads = cache["dtype"], {}
    zero = torch.zeros((), dtype=dtype)
    N = cache["top"][0]
    dp = torch.zeros(N, 1, dtype=dtype) if d_pred is None else d_pred.to(dtype)
    grads["fc.weight"] = dp.t() @ cache["pooled"]
    g = ((dp @ cache["fc"]) / 16.0).view(N, -1, 1, 1, 1).expand(cache["top"]).clone()
    for st in reversed(cache["steps"]):
        b = st["block"]
        if b["last"] and d_fmaps is not None and d_fmaps[b["layer"]] is not None:
            g = g + d_fmaps[b["layer"]].to(dtype)
        g = torch.where(st["mask"], g, zero)
        dh1 = _norm_conv_backward(st["c2"], g, grads, mutate)
        dh1 = torch.where(st["c1"]["mask"], dh1, zero)
        dx = _norm_conv_backward(st["c1"], dh1, grads, mutate)
        if mutate == "residual_one_branch":
            if st["cd"] is not None:
                _norm_conv_backward(st["cd"], g, grads, mutate)
        elif st["cd"] is not None:
            dx = dx + _norm_conv_backward(st["cd"], g, grads, mutate)
        elif dx.shape == g.shape:
            dx = dx + g
        else:                                         # (the identity residual of the downsample_without_stride_t mutation)
            dx[:, :, ::b["st"]] += g
        g = dx
    if cache["pool"] is not None:
        idx, shp = cache["pool"]["idx"], cache["pool"]["in_shape"]
        g = torch.zeros(*shp[:2], int(np.prod(shp[2:])), dtype=dtype).scatter_add_(2, idx.reshape(*idx.shape[:2], -1), g.reshape(*g.shape[:2], -1)).reshape(shp)
    g = torch.where(cache["stem"]["mask"], g, zero)
    dx = _norm_conv_backward(cache["stem"], g, grads, mutate)
    return grads, dx


def fmap_loss_oracle(f1, f2, metric="L1"):
    """-> (loss, [d loss / d f1[i]]) in float64 (sign(0) = 0)"""
    n = len(f1)
    d = [a.double() - b.double() for a, b in zip(f1, f2)]
    if metric == "L1":
        return sum(x.abs().mean() for x in d) / n, [torch.sign(x) / (x.numel() * n) for x in d]
    return sum((x ** 2).mean() for x in d) / n, [2 * x / (x.numel() * n) for x in d]


def generator_loss_oracle(sd, fake, real, cfg, w_coup_t=1, w_fmap_t=10):
    """loss.py:127-135 through the oracle -> ((coup_t, L_fmap_t, L_temp), gradient at fake, state after both forwards)"""
    pf, ff, cf = forward_oracle(sd, fake, cfg, training=True)
    sd2 = dict(sd, **cf["state"])
    _, fr, cr = forward_oracle(sd2, real, cfg, training=True)
    coup = -pf.mean()
    fm, dfm = fmap_loss_oracle(ff, fr)
    _, dx = backward_oracle(cf, torch.full_like(pf, -float(w_coup_t) / pf.numel()), [w_fmap_t * d for d in dfm])
    return (coup, fm, w_coup_t * coup + w_fmap_t * fm), dx, dict(sd2, **cr["state"])


def gradient_penalty_oracle(sd, real, cfg):
    """The value of loss.py:35-43 -> (L_GP, state after the forward)"""
    pred, _, c = forward_oracle(sd, real, cfg, training=True)
    _, dx = backward_oracle(c, torch.full_like(pred, 1.0 / pred.numel()))
    return dx.pow(2).reshape(dx.shape[0], -1).sum(1).mean(), dict(sd, **c["state"])


def decision_report(given, cache64):
    """How the given decisions differ from the float64 pass's own (which ran WITHOUT them): per name (differing units, differing units
    whose deciding margin exceeds FRAGILE_REL x the layer's rms).  A ReLU's margin is |h|; the pool's is the gap between the value float64
    chose and the value at the given position."""
    rep = {}
    for name, own in cache64["decisions"].items():
        h = cache64["margins"][name]
        rms = float(h.double().pow(2).mean().sqrt())
        if name == "pool":
            diff = given[name] != own
            flat = h.reshape(*h.shape[:2], -1)
            gap = (flat.gather(2, own.reshape(*own.shape[:2], -1)) - flat.gather(2, given[name].reshape(*own.shape[:2], -1))).abs().reshape(own.shape)
        else:
            diff = given[name] != own
            gap = h.abs()
        rep[name] = (int(diff.sum()), int((diff & (gap > FRAGILE_REL * rms)).sum()))
    return rep


# ---------------------------------------------------------------------------------------------------------------- unit oracles

def cl(x):
    """[N, C, T, H, W] -> channels-last [N, T, H, W, C] fp32 (3 channels: a zero fourth is appended)."""
    x = x.float().permute(0, 2, 3, 4, 1)
    if x.shape[-1] == 3:
        x = torch.cat([x, torch.zeros_like(x[..., :1])], dim=-1)
    return x.contiguous()


def uncl(y):
    """channels-last [N, T, H, W, C] -> [N, C, T, H, W]"""
    return y.permute(0, 4, 1, 2, 3)


def out_extent(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def conv_case_inputs(case):
    """(x [N, Cin, T, H, W], w [Cout, Cin, 3, k, k], g [N, Cout, To, Ho, Wo], act like g) fp32"""
    cin, cout, (t, h, w), b, k = case["cin"], case["cout"], case["thw"], case["batch"], case.get("k", 3)
    st, ss = case["st"], case["ss"]
    x = randn(case["seed"], (b, cin, t, h, w))
    wt = randn(case["seed"] + 1, (cout, cin, 3, k, k)) * float(np.sqrt(1.0 / (3 * k * k * cin)))
    oshape = (b, cout, out_extent(t, 3, st), out_extent(h, k, ss), out_extent(w, k, ss))
    return x, wt, randn(case["seed"] + 2, oshape), randn(case["seed"] + 3, oshape)


def conv_oracle(x, w, st, ss):
    k = w.shape[-1]
    x, w = x.double(), w.double()
    kw = dict(stride=(st, ss, ss), padding=(1, k // 2, k // 2))
    return F.conv3d(x, w, **kw), F.conv3d(x.abs(), w.abs(), **kw), int(np.prod(w.shape[1:]))


def dgrad_oracle(g, w, act, in_thw, st, ss, add=None, add_mask=None, mutate=None):
    """-> (ref [N, Cin, T, H, W], S, n [1, 1, T, H, W]: the chain length of each position's parity class)"""
    k = w.shape[-1]
    dy, w = g.double(), w.double()
    if act is not None:
        dy = dy * (act > 0)
    ref = dgrad_taps(dy, w, in_thw, (st, ss, ss), mutate)
    S = conv3d_input((g.shape[0], w.shape[1]) + tuple(in_thw), w.abs(), dy.abs(), stride=(st, ss, ss), padding=(1, k // 2, k // 2))
    n = class_taps(in_thw, (3, k, k), (st, ss, ss)) * w.shape[0]
    if add is not None:
        a = add.double() * (1.0 if add_mask is None else (add_mask > 0))
        ref, S, n = ref + a, S + a.abs(), n + 1
    return ref, S, n


def wgrad_oracle(g, x, w, act, st, ss, u=None, v=None, sigma=None, mutate=None, u0=None):
    """-> (dweight, bound) in float64.  With u, v, sigma: w is weight_orig and the conv ran on w / sigma (u0: the u from before the
    iteration, for the mutation that uses it)."""
    k = w.shape[-1]
    dy, x, w = g.double(), x.double(), w.double()
    if act is not None:
        dy = dy * (act > 0)
    kw = dict(stride=(st, ss, ss), padding=(1, k // 2, k // 2))
    n = dy.shape[0] * int(np.prod(dy.shape[2:]))
    dWn = conv3d_weight(x, w.shape, dy, **kw)
    S = conv3d_weight(x.abs(), w.shape, dy.abs(), **kw)
    bound = gamma(n) * S
    if sigma is not None:
        sg, Wn = float(sigma), w / float(sigma)
        p = (dWn * Wn).sum() * torch.outer(u.double(), v.double()).view_as(dWn)
        pa = (S * Wn.abs()).sum() * torch.outer(u.double().abs(), v.double().abs()).view_as(dWn)
        if mutate == "projection_dropped":
            p = p * 0
        if mutate == "u_before_iteration":
            p = (dWn * Wn).sum() * torch.outer(u0.double(), v.double()).view_as(dWn)
        dWn = (dWn - p) / sg
        bound = (bound + gamma(n + 4) * pa + gamma(4) * p.abs()) / sg + U * dWn.abs()
    return dWn, bound + U * dWn.abs()


CONV_CH = ((16, 16), (16, 32), (32, 48), (48, 48))
CONV_STRIDES = ((1, 1), (2, 1), (2, 2), (1, 2))
CONV_MAPS = ((1, 4, 4), (2, 5, 7), (3, 8, 8), (4, 5, 7))


def conv_cases():
    """Every (channels, strides) pair on two maps, rotated with the channel pair so that every map -- T in {1, 2, 3, 4}, H x W in {4 x 4,
    5 x 7, 8 x 8} -- meets every stride pair, and both batch sizes: odd extents under stride 2, a single frame under temporal stride 2,
    ragged last tiles."""
    cases, seed, i = [], 51000, 0
    for cin, cout in CONV_CH:
        for st, ss in CONV_STRIDES:
            for j in range(2):
                thw = CONV_MAPS[(i + i // 4 + 2 * j) % 4]
                b = (1, 3)[(i + j) % 2]
                seed += 10
                cases.append({"id": f"c{cin}-{cout}-st{st}-ss{ss}-{'x'.join(map(str, thw))}-b{b}", "cin": cin, "cout": cout, "st": st, "ss": ss, "thw": thw,
                              "batch": b, "seed": seed})
            i += 1
    return cases


STEM_CASES = [{"id": f"stem-{t}x{h}x{w}-b{b}", "cin": 3, "cout": 16, "st": 1, "ss": 2, "k": 7, "thw": (t, h, w), "batch": b, "seed": 52000 + 10 * i}
              for i, (t, h, w, b) in enumerate(((1, 16, 16, 1), (3, 10, 12, 2)))]


def rows_per_workgroup(rows, column_tiles):
    """The tile choice of the two GEMM kernels (csrc/i2v_disc3d.hip, rows_of), restated so that the tests can say which they ran."""
    return 128 if (rows + 127) // 128 * column_tiles >= 512 else 64


def big_cases():
    """Past the only tile-size threshold of the launch code (128-row tiles from 512 row tiles per column tile on), with a ragged tail:
    65 536 + positions, every column-tile width (16, 32, 64) of both GEMM kernels -- the forward's follows Cout, the input gradient's Cin."""
    big = (2, 181, 182)
    return [{"id": "big-conv-bn16", "kind": "conv", "cin": 16, "cout": 16, "st": 1, "ss": 1, "thw": big, "batch": 1, "seed": 53010},
            {"id": "big-conv-bn32", "kind": "conv", "cin": 16, "cout": 32, "st": 1, "ss": 1, "thw": big, "batch": 1, "seed": 53040},
            {"id": "big-conv-bn64", "kind": "conv", "cin": 16, "cout": 64, "st": 1, "ss": 1, "thw": big, "batch": 1, "seed": 53050},
            {"id": "big-dgrad-bn16-s1", "kind": "dgrad", "cin": 16, "cout": 16, "st": 1, "ss": 1, "thw": big, "batch": 1, "seed": 53020},
            {"id": "big-dgrad-bn16-s2", "kind": "dgrad", "cin": 16, "cout": 16, "st": 2, "ss": 2, "thw": (3, 183, 181), "batch": 1, "seed": 53030},
            {"id": "big-dgrad-bn32-s1", "kind": "dgrad", "cin": 32, "cout": 16, "st": 1, "ss": 1, "thw": big, "batch": 1, "seed": 53060},
            {"id": "big-dgrad-bn64-s2", "kind": "dgrad", "cin": 64, "cout": 16, "st": 2, "ss": 2, "thw": (3, 183, 181), "batch": 1, "seed": 53070}]


DGRAD_VARIANTS = ({"name": "plain", "act": False, "add": False, "add_mask": False}, {"name": "mask", "act": True, "add": False, "add_mask": False},
                  {"name": "add", "act": False, "add": True, "add_mask": False}, {"name": "mask-add-addmask", "act": True, "add": True, "add_mask": True})


def dgrad_cases():
    """The conv grid, each case with one named variant of the input-gradient kernel's options (every variant meets every stride pair and
    every channel pair); both stem maps in the frames' layout and in the 4-channel layout, with and without the mask."""
    cases = []
    for i, c in enumerate(conv_cases()):
        v = DGRAD_VARIANTS[(i // 2 + i // 8 + i % 2 * 2) % 4]
        cases.append(dict(c, id=f"{c['id']}-{v['name']}", act=v["act"], add=v["add"], add_mask=v["add_mask"], frames=False))
    for c in STEM_CASES:
        for frames in (True, False):
            for act in (False, True):
                cases.append(dict(c, id=f"{c['id']}-{'frames' if frames else 'cl4'}-{'mask' if act else 'plain'}", act=act, add=False, add_mask=False,
                                  frames=frames))
    return cases


def wgrad_cases():
    """Position counts that the slice plan turns into one, two and three slices, with ragged last slices (asserted by the GPU test)."""
    return [{"id": "one-slice", "cin": 16, "cout": 32, "st": 2, "ss": 2, "thw": (3, 8, 8), "batch": 1, "seed": 54010, "slices": 1},      # 32 positions
            {"id": "two-slices", "cin": 16, "cout": 16, "st": 1, "ss": 1, "thw": (2, 5, 7), "batch": 1, "seed": 54020, "slices": 2},     # 70 = 48 + 22
            {"id": "three-slices", "cin": 32, "cout": 48, "st": 1, "ss": 2, "thw": (4, 5, 7), "batch": 3, "seed": 54030, "slices": 3},   # 144 = 3 x 48
            {"id": "three-ragged", "cin": 48, "cout": 48, "st": 2, "ss": 1, "thw": (3, 5, 7), "batch": 2, "seed": 54040, "slices": 3},   # 140 = 48 + 48 + 44
            {"id": "stem", "cin": 3, "cout": 16, "st": 1, "ss": 2, "k": 7, "thw": (3, 10, 12), "batch": 2, "seed": 54050, "slices": 3}]  # 180 = 64 + 64 + 52
