"""Shared by tests/test_host_encoder_train.py, tests/test_gpu_encoder_train.py and tests/golden/make_golden_encoder_train.py: a float64
restatement of the motion encoder (reference stage1_VAE/modules/resnet3D.py:138-219) with its posterior head, the reparameterisation and
the KL term (loss.py:10-12) in functional torch on the CPU -- and a BACKWARD WRITTEN OUT BY HAND (not autograd), so that the ReLU masks can
be given and single deliberate errors switched on -- plus the oracles of the head's kernels with their bounds and the inputs of the
fixtures.  Nothing of the package is imported; the trunk's pieces (GroupNorm, the tap-by-tap input gradient, the conv backward) and the
gate are those of temporal_disc_common / i3d_units_common, by import.

The gate: |got - ref64| <= gamma(n) S + 2^-24 |ref64| element-wise, with n the length of the summation chain and S the same sum over
absolute products, and relative L2 <= 1e-4 per batch row.  The trunk's families keep the bounds stated in temporal_disc_common.  New here:
  head forward   mu, logvar: 16 C products and the bias, in any order: n = 16 C + 1, S = sum |emb| |w| + |b|
  sample         eps e^{lv / 2} + mu formed in float64 from the kernel's OWN fp32 mu and logvar and rounded once; the two float64
                 exponentials (device, host) may differ in the last place, far below 2^-24: n = 1, S = |eps| e^{lv / 2} + |mu|
  fold, KL grad  g_mu = d_mu + d_sample + k mu / N, g_lv = d_lv + d_sample eps e^{lv / 2} / 2 + k (e^lv - 1) / (2 N): float64 sums of fp32
                 operands rounded once: n = 1, S = the sum of the terms' magnitudes (with e^lv + 1 for the difference)
  head dgrad     d_emb = sum over the 2 z columns of g w, on the fp32 g of the fold (its rounding is the + 2): n = 2 z + 2,
                 S = sum S_g |w| with S_g the fold's S
  head wgrad     dW = sum over the N samples of g emb: n = N + 2, S = sum S_g |emb|
  head bias      float64 sum over the samples, rounded once, of the rounded g: n = 3, S = sum S_g
"""
import numpy as np
import torch
import torch.nn.functional as F

import temporal_disc_common as tc
from i3d_units_common import U, TOL_L2, gamma, gate, gate_bound, randn, rel_l2_rows  # noqa: F401  (the gate is reused by import)
from temporal_disc_common import FRAGILE_MAX, FRAGILE_REL, SGD_STEPS, cl, decision_report, uncl  # noqa: F401

CFG_A = {"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": 24, "channels": [16, 16, 32, 32, 48], "stride_s": [1, 2, 2, 1],
         "stride_t": [1, 2, 2, 1]}
CFG_B = {"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": 8, "channels": [16, 32, 32, 32, 32], "stride_s": [1, 1, 1, 1],
         "stride_t": [2, 1, 1, 1]}
CFG_SHIPPED = {"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": 64, "channels": [64, 128, 256, 512, 512], "stride_s": [1, 2, 2, 2],
               "stride_t": [1, 2, 2, 2]}
# the reference can BUILD this one (its forward then fails on the half-rate residual); only its list of keys is recorded
CFG_HALFRATE = {"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": 8, "channels": [16, 16, 32, 32, 32], "stride_s": [1, 1, 1, 1],
                "stride_t": [2, 1, 1, 1]}
# a small network on the smallest clip that the INFERENCE handle takes too (frames of 64 x 64, a power of two of frames behind the stem)
CFG_D = {"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": 8, "channels": [16, 16, 32, 32, 32], "stride_s": [2, 2, 2, 1],
         "stride_t": [2, 1, 1, 1]}
CLIP_D, SEED_D = (2, 3, 4, 64, 64), 6400
CLIP_A, CLIP_B, CLIP_B2, CLIP_SHIPPED = (3, 3, 6, 32, 32), (2, 3, 3, 8, 8), (2, 3, 2, 8, 8), (1, 3, 16, 64, 64)
SEED_A, SEED_B, SEED_SHIPPED = 6100, 6200, 6300
# The fixtures' loss is linear in the outputs with O(1) coefficients, so it has no minimum and its gradient does not shrink: at the
# discriminator tests' 1e-3 the steps overshoot and the reference's own float64 and fp32 sequences part by more than 1 after four steps,
# which would make the band of the SGD test vacuous; at 1e-4 they stay within the rounding of the loss value.
SGD_LR = 1e-4
KL_WEIGHT = 1.0   # the fixtures' loss weighs KL with 1, not with the configs' 1e-5, so that an error in its gradient is visible
MUTATIONS = ("kl_half_dropped", "eps_missing_in_dlogvar", "head_layout_swapped", "downsample_with_stride_t_term", "stem_stride_t_1",
             "taps_not_flipped", "residual_one_branch")


def blocks(cfg, mutate=None):
    """The eight BasicBlocks: state-dict prefix, widths, strides, whether a downsample branch exists (resnet3D.py:184: no stride_t term)."""
    out, inplanes = [], cfg["channels"][0]
    for l, planes in enumerate(cfg["channels"][1:]):
        ss, st = cfg["stride_s"][l], cfg["stride_t"][l]
        ds = ss != 1 or inplanes != planes
        if mutate == "downsample_with_stride_t_term":
            ds = ds or st != 1
        out.append(dict(prefix=f"layer.{l}.0.", cin=inplanes, cout=planes, st=st, ss=ss, ds=ds, layer=l, last=False))
        out.append(dict(prefix=f"layer.{l}.1.", cin=planes, cout=planes, st=1, ss=1, ds=False, layer=l, last=True))
        inplanes = planes
    return out


def state_keys(cfg, mutate=None):
    """{key: shape} of Encoder(cfg).state_dict(), in the reference's order."""
    c0, z = cfg["channels"][0], cfg["z_dim"]
    out = {"conv1.weight": (c0, 3, 3, 7, 7), "norm1.weight": (c0,), "norm1.bias": (c0,)}
    for b in blocks(cfg, mutate):
        p = b["prefix"]
        out[p + "conv1.weight"] = (b["cout"], b["cin"], 3, 3, 3)
        out[p + "bn1.weight"], out[p + "bn1.bias"] = (b["cout"],), (b["cout"],)
        out[p + "conv2.weight"] = (b["cout"], b["cout"], 3, 3, 3)
        out[p + "bn2.weight"], out[p + "bn2.bias"] = (b["cout"],), (b["cout"],)
        if b["ds"]:
            out[p + "downsample.0.weight"] = (b["cout"], b["cin"], 3, 3, 3)
            out[p + "downsample.1.weight"], out[p + "downsample.1.bias"] = (b["cout"],), (b["cout"],)
    c4 = cfg["channels"][4]
    out["conv_mu.weight"], out["conv_mu.bias"] = (z, c4, 4, 4), (z,)
    out["conv_var.weight"], out["conv_var.bias"] = (z, c4, 4, 4), (z,)
    return out


def synthetic_state(cfg, seed):
    """A seeded state dict (numpy draws, platform-stable; the fixtures store no parameters): conv weights of fan-in scale, GroupNorm
    weights around 1, biases around 0; conv_var small enough that e^logvar stays O(1)."""
    sd = {}
    for i, (k, shape) in enumerate(state_keys(cfg).items()):
        x = randn(seed + i, shape)
        if len(shape) >= 4:
            x = x * float(np.sqrt((0.5 if k.startswith("conv_var") else 2.0) / int(np.prod(shape[1:]))))
        elif k.endswith("bias"):
            x = 0.1 * x
        else:
            x = 1.0 + 0.2 * x
        sd[k] = x.float().contiguous()
    return sd


def inputs(cfg, clip, seed):
    """(x, eps, c_sample, c_mu, c_logvar) fp32: the clips, the reparameterisation's draw and the loss's coefficients."""
    n, z = clip[0], cfg["z_dim"]
    return (randn(seed + 500, clip), randn(seed + 501, (n, z)), randn(seed + 502, (n, z)), randn(seed + 503, (n, z)), randn(seed + 504, (n, z)))


def kl_value(mu, logvar):
    return -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=-1))


# ---------------------------------------------------------------------------------------------------------------- the network, by hand

def forward_oracle(sd, x, eps, cfg, dtype=torch.float64, decisions=None, mutate=None):
    """sd: {state_dict key: tensor}; x [N, 3, T, H, W]; eps [N, z].  -> (sample, mu, logvar, cache).  ``decisions``: {norm key: bool mask}
    of ReLU decisions to use instead of this pass's own; cache["decisions"] / ["margins"]: those taken and the values they were taken on."""
    x, eps = x.to(dtype), eps.to(dtype)
    dec, margins, steps = {}, {}, []
    given = decisions or {}

    def relu(name, h):
        mask = given.get(name, h > 0)
        dec[name], margins[name] = mask, h
        return torch.where(mask, h, torch.zeros((), dtype=dtype)), mask

    def conv_norm(ckey, nkey, xin, strides, pads):
        W = sd[ckey + ".weight"].to(dtype)
        y = F.conv3d(xin, W, stride=strides, padding=pads)
        w, b = sd[nkey + ".weight"].to(dtype), sd[nkey + ".bias"].to(dtype)
        h, xhat, rstd = tc.group_norm(y, w, b)
        return h, dict(W=W, Wn=W, u=None, v=None, u0=None, sigma=torch.ones((), dtype=dtype), key=ckey + ".weight", x=xin, y=y, xhat=xhat, rstd=rstd,
                       gw=w, nkey=nkey, strides=strides, pads=pads)

    h, stem = conv_norm("conv1", "norm1", x, (1 if mutate == "stem_stride_t_1" else 2, 2, 2), (1, 3, 3))
    h, stem["mask"] = relu("norm1", h)
    for b in blocks(cfg):
        p, xin = b["prefix"], h
        h1, c1 = conv_norm(p + "conv1", p + "bn1", xin, (b["st"], b["ss"], b["ss"]), (1, 1, 1))
        h1, c1["mask"] = relu(p + "bn1", h1)
        h2, c2 = conv_norm(p + "conv2", p + "bn2", h1, (1, 1, 1), (1, 1, 1))
        cd, res = None, xin
        if b["ds"]:
            res, cd = conv_norm(p + "downsample.0", p + "downsample.1", xin, (b["st"], b["ss"], b["ss"]), (1, 1, 1))
        h, mask = relu(p + "bn2", h2 + res)
        steps.append(dict(block=b, c1=c1, c2=c2, cd=cd, mask=mask, x=xin))
    assert h.shape[2:] == (1, 4, 4), f"the network ends on a {tuple(h.shape[2:])} map"
    emb = h[:, :, 0]                                             # [N, C, 4, 4]
    wm, bm, wv, bv = (sd[k].to(dtype) for k in ("conv_mu.weight", "conv_mu.bias", "conv_var.weight", "conv_var.bias"))
    N, C = emb.shape[:2]
    flat = emb.reshape(N, C, 16)
    if mutate == "head_layout_swapped":                          # the channels-last map's index p C + c read as c 16 + p
        flat = flat.permute(0, 2, 1).reshape(N, C, 16)
    mu = torch.einsum("ncp,jcp->nj", flat, wm.reshape(-1, C, 16)) + bm
    logvar = torch.einsum("ncp,jcp->nj", flat, wv.reshape(-1, C, 16)) + bv
    sample = eps * torch.exp(0.5 * logvar) + mu                  # resnet3D.py:203-206 with the given eps
    return sample, mu, logvar, dict(steps=steps, stem=stem, decisions=dec, margins=margins, flat=flat, wm=wm, wv=wv, mu=mu, logvar=logvar, eps=eps,
                                    top=h.shape, dtype=dtype, mutate_fwd=mutate)


def fold_oracle(mu, logvar, eps, d_sample, d_mu, d_logvar, kl_scale, mutate=None):
    """-> (g_mu, g_lv, S_mu, S_lv) in float64: the gradients at mu and logvar and the sums of their terms' magnitudes."""
    mu, logvar = mu.double(), logvar.double()
    n = mu.shape[0]
    zero = torch.zeros_like(mu)
    dm, dl = (zero if d_mu is None else d_mu.double()), (zero if d_logvar is None else d_logvar.double())
    ds = zero if d_sample is None else d_sample.double()
    e = torch.ones_like(mu) if (eps is None or mutate == "eps_missing_in_dlogvar") else eps.double()
    if d_sample is None:
        e = zero
    half = 1.0 if mutate == "kl_half_dropped" else 2.0
    t_s = ds * e * 0.5 * torch.exp(0.5 * logvar)
    g_mu = dm + ds + kl_scale * mu / n
    g_lv = dl + t_s + kl_scale * (torch.exp(logvar) - 1.0) / (half * n)
    S_mu = dm.abs() + ds.abs() + abs(kl_scale) * mu.abs() / n
    S_lv = dl.abs() + t_s.abs() + abs(kl_scale) * (torch.exp(logvar) + 1.0) / (half * n)
    return g_mu, g_lv, S_mu, S_lv


def backward_oracle(cache, d_sample=None, d_mu=None, d_logvar=None, kl_scale=0.0, mutate=None):
    """-> ({state_dict key: gradient}, dx [N, 3, T, H, W]) by hand, for the upstream gradients [N, z] (or None) plus kl_scale * KL."""
    dtype, grads = cache["dtype"], {}
    zero = torch.zeros((), dtype=dtype)
    g_mu, g_lv, _, _ = fold_oracle(cache["mu"], cache["logvar"], cache["eps"], d_sample, d_mu, d_logvar, kl_scale, mutate)
    g_mu, g_lv = g_mu.to(dtype), g_lv.to(dtype)
    flat, wm, wv = cache["flat"], cache["wm"], cache["wv"]
    N, C = flat.shape[:2]
    grads["conv_mu.weight"] = torch.einsum("nj,ncp->jcp", g_mu, flat).reshape(wm.shape)
    grads["conv_var.weight"] = torch.einsum("nj,ncp->jcp", g_lv, flat).reshape(wv.shape)
    grads["conv_mu.bias"], grads["conv_var.bias"] = g_mu.sum(0), g_lv.sum(0)
    d_flat = torch.einsum("nj,jcp->ncp", g_mu, wm.reshape(-1, C, 16)) + torch.einsum("nj,jcp->ncp", g_lv, wv.reshape(-1, C, 16))
    if cache["mutate_fwd"] == "head_layout_swapped":
        d_flat = d_flat.reshape(N, 16, C).permute(0, 2, 1)
    g = d_flat.reshape(cache["top"])
    for st in reversed(cache["steps"]):
        g = torch.where(st["mask"], g, zero)
        dh1 = tc._norm_conv_backward(st["c2"], g, grads, mutate)
        dh1 = torch.where(st["c1"]["mask"], dh1, zero)
        dx = tc._norm_conv_backward(st["c1"], dh1, grads, mutate)
        if mutate == "residual_one_branch":
            if st["cd"] is not None:
                tc._norm_conv_backward(st["cd"], g, grads, mutate)
        elif st["cd"] is not None:
            dx = dx + tc._norm_conv_backward(st["cd"], g, grads, mutate)
        else:
            dx = dx + g
        g = dx
    g = torch.where(cache["stem"]["mask"], g, zero)
    dx = tc._norm_conv_backward(cache["stem"], g, grads, mutate)
    return grads, dx


def loss_and_grads(sd, x, eps, coefs, cfg, dtype=torch.float64, decisions=None, mutate=None, kl_only=False):
    """The fixtures' loss sum(c_s sample) + sum(c_m mu) + sum(c_l logvar) + KL_WEIGHT KL (kl_only: the last term alone)
    -> (loss, (sample, mu, logvar), grads, dx, cache)"""
    cs, cm, clv = (c.to(dtype) for c in coefs)
    sample, mu, logvar, cache = forward_oracle(sd, x, eps, cfg, dtype, decisions, mutate)
    kl = kl_value(mu, logvar)
    if kl_only:
        loss = KL_WEIGHT * kl
        grads, dx = backward_oracle(cache, None, None, None, KL_WEIGHT, mutate)
    else:
        loss = (cs * sample).sum() + (cm * mu).sum() + (clv * logvar).sum() + KL_WEIGHT * kl
        grads, dx = backward_oracle(cache, cs, cm, clv, KL_WEIGHT, mutate)
    return loss, (sample, mu, logvar), grads, dx, cache


def sgd_losses(sd, x, eps, coefs, cfg, dtype):
    """The losses of SGD_STEPS plain SGD steps (lr SGD_LR) on the fixtures' loss, through the hand-written backward."""
    sd = {k: v.to(dtype).clone() for k, v in sd.items()}
    seq = []
    for _ in range(SGD_STEPS):
        loss, _, grads, _, _ = loss_and_grads(sd, x, eps, coefs, cfg, dtype)
        seq.append(float(loss))
        for k in sd:
            sd[k] = sd[k] - SGD_LR * grads[k]
    return seq


# ---------------------------------------------------------------------------------------------------------------- the head's unit oracles

HEAD_N, HEAD_C, HEAD_Z2 = (1, 3, 17), (16, 48, 64), (16, 48, 128)


def head_cases():
    """Every n in {1, 3, 17} with every C in {16, 48, 64} and every 2 z in {16, 48, 128} once each way round (a Latin square): a masked
    single row, a row tile with 13 masked rows, two row tiles; one, three and four K slices; one, three and eight column tiles."""
    cases = []
    for a, n in enumerate(HEAD_N):
        for b, c in enumerate(HEAD_C):
            z2 = HEAD_Z2[(a + b) % 3]
            cases.append({"id": f"n{n}-c{c}-z{z2 // 2}", "n": n, "c": c, "z": z2 // 2, "seed": 61000 + 100 * a + 10 * b})
    cases.append({"id": "n2-c32-z3", "n": 2, "c": 32, "z": 3, "seed": 61900})      # 2 z = 6: a masked column tile
    cases.append({"id": "n5-c16-z70", "n": 5, "c": 16, "z": 70, "seed": 61910})    # 2 z = 140: two chunks of the input gradient's staging
    return cases


def head_inputs(case):
    """(emb [n, 16, C] channels-last, w_mu, b_mu, w_var, b_var, eps, d_sample, d_mu, d_logvar) fp32"""
    n, c, z, s = case["n"], case["c"], case["z"], case["seed"]
    sc = float(np.sqrt(1.0 / (16 * c)))
    return (randn(s, (n, 16, c)), randn(s + 1, (z, c, 4, 4)) * sc, 0.1 * randn(s + 2, (z,)), randn(s + 3, (z, c, 4, 4)) * sc, 0.1 * randn(s + 4, (z,)),
            randn(s + 5, (n, z)), randn(s + 6, (n, z)), randn(s + 7, (n, z)), randn(s + 8, (n, z)))


def _flat(emb):
    return emb.double().permute(0, 2, 1)                         # [n, C, 16]


def head_forward_oracle(emb, w_mu, b_mu, w_var, b_var):
    """-> ((mu, S, n), (logvar, S, n))"""
    f, C = _flat(emb), emb.shape[-1]
    out = []
    for w, b in ((w_mu, b_mu), (w_var, b_var)):
        w3 = w.double().reshape(-1, C, 16)
        out.append((torch.einsum("ncp,jcp->nj", f, w3) + b.double(), torch.einsum("ncp,jcp->nj", f.abs(), w3.abs()) + b.double().abs(), 16 * C + 1))
    return out


def sample_oracle(eps, mu, logvar):
    """From the kernel's own fp32 mu and logvar -> (ref, S, n)"""
    t = eps.double() * torch.exp(0.5 * logvar.double())
    return t + mu.double(), t.abs() + mu.double().abs(), 1


def head_backward_oracle(emb, w_mu, w_var, g_mu, g_lv, S_mu, S_lv):
    """From the float64 fold -> {name: (ref, S, n)} for d_emb [n, 16, C], dw_mu, dw_var, db_mu, db_var"""
    f, C, N = _flat(emb), emb.shape[-1], emb.shape[0]
    wm, wv = w_mu.double().reshape(-1, C, 16), w_var.double().reshape(-1, C, 16)
    z2 = 2 * wm.shape[0]
    d = torch.einsum("nj,jcp->ncp", g_mu, wm) + torch.einsum("nj,jcp->ncp", g_lv, wv)
    dS = torch.einsum("nj,jcp->ncp", S_mu, wm.abs()) + torch.einsum("nj,jcp->ncp", S_lv, wv.abs())
    out = {"d_emb": (d.permute(0, 2, 1), dS.permute(0, 2, 1), z2 + 2)}
    for name, g, S in (("mu", g_mu, S_mu), ("var", g_lv, S_lv)):
        out["dw_" + name] = (torch.einsum("nj,ncp->jcp", g, f).reshape(w_mu.shape), torch.einsum("nj,ncp->jcp", S, f.abs()).reshape(w_mu.shape), N + 2)
        out["db_" + name] = (g.sum(0), S.sum(0), 3)
    return out
