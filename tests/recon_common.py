"""What the reconstruction-metric tests share: the float64 oracle of PSNR / SSIM / L1 / KL (the specification: a restatement of
pytorch_lightning 1.2.7's ``psnr`` and ``ssim``, which the reference's stage1_VAE/modules/loss.py calls), a seeded input synthesiser, the
derived gate and the deliberate errors the gate has to reject.  torch on the CPU only.

Argument order as the reference calls the two functions, ``psnr(seq_orig, seq_gen)`` / ``ssim(seq_orig, seq_gen)``: ``pred`` is the real clip,
``target`` the generated one.

The gate
--------
u = 2^-53, gamma(n) = n u / (1 - n u).  The kernel and the oracle both evaluate the SAME real-valued formula in float64 from inputs that
are exact in float64 (fp32 pixels; p - t, p^2, t^2, p t of fp32 values are exact or correctly rounded), in different orders.  Each is
within B of the exact value, so they are within 2 B of each other; every bound below is that 2 B.

* sums of non-negative terms (sum |p - t|, sum (p - t)^2 over n elements): any order of a float64 sum of n terms, each carrying at most
  three roundings of its own, is within gamma(n + 3) * sum |terms| = gamma(n + 3) * value.  Bound 2 gamma(n + 3) value; the means add u.
* PSNR = (2 ln R - ln MSE) * 10 / ln 10: R = max - min of fp32 values, rounded once (u); ln is good to one ulp (2 u |ln x| covers it);
  |d ln MSE| <= the relative bound of the MSE.  Bound 2 [ (10 / ln 10) (2 u (1 + 2 |ln R|) + gamma(n + 4) + 2 u |ln MSE|) + 4 u |PSNR| ].
* SSIM, per position.  Window weights: exp's argument carries three roundings of a value <= 5.6 (17 u absolute), exp one ulp, the sum
  of 11 and the division: a 1-D weight is within gamma(52) relatively, a product of two within gamma(105); a dot product of 121 terms
  adds gamma(121) (the separable form: twice gamma(52 + 11), which is less).  K = 256 covers either.  With a^2 = E[p^2], b^2 = E[t^2],
  q = a^2 + b^2 (all terms of those two sums are positive, so they are their own absolute sums; by Jensen sum w |p| <= a and
  sum w |p t| <= q / 2):
      |d mu_p| <= gamma(K) a,  |d E..| <= gamma(K) {a^2, b^2, q / 2}
      |d mu_p^2|, |d mu_t^2|, |d mu_p mu_t| <= (2 gamma(K) + 2 u) {a^2, b^2, q / 2}
      |d sigma..| <= (3 gamma(K) + 4 u) {a^2, b^2, q / 2}
  A1 = 2 mu_p mu_t + c1, B1 = mu_p^2 + mu_t^2 + c1:  |dA1|, |dB1| <= e1 = (2 gamma(K) + 2 u) q + 4 u B1
  A2 = 2 sigma_pt + c2,  B2 = sigma_p^2 + sigma_t^2 + c2:  |dA2|, |dB2| <= e2 = (3 gamma(K) + 4 u) q + 4 u B2
  (4 u B covers c1, c2 themselves and the additions).  |A1| <= B1 and |A2| <= B2 (AM-GM, Cauchy-Schwarz), so |ssim| <= 1 and with
  r = e1 / B1 + e2 / B2 the quotient A1 A2 / (B1 B2) moves by at most 2 r / (1 - r) + 3 u.  This is where the conditioning enters:
  B1 >= c1 and B2 >= c2 = (0.03 R)^2, which is why the inputs keep R >= 0.5 -- q / c2 stays below a few thousand.
  An image's sum over m positions: 2 sum(per-position bound) + 2 gamma(m) sum |ssim|; the scalar adds 2 gamma(N) over the rows and 2 u.
* KL: each term 1 + lv - mu^2 - exp(lv) carries at most six roundings of parts whose magnitudes sum to 1 + |lv| + mu^2 + exp(lv);
  bound 2 gamma(n + 8) * 0.5 / b * sum(1 + |lv| + mu^2 + exp(lv)) + 2 u |KL|.

``check_scalars`` asserts that the relative bound of every scalar output is below 1e-8: the fp32 form of the same formula differs from
float64 by 9e-8 .. 2.5e-6 on these input families, so a gate that loose could not tell the float64 kernel from an fp32 one."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -53
K_WINDOW = 256
REL_CEILING = 1e-8
SIGMAS = (0.02, 0.1, 0.5)

MUTATIONS = ("padded_mean", "sigma_1", "unnormalised", "psnr_range_pred", "ssim_range_1", "c_swapped", "fp32_sums")


def gamma(n):
    return n * U / (1.0 - n * U)


def window(sigma=1.5, size=11, normalise=True, dtype=torch.float64):
    """[1, size]: g / sum g, g_i = exp(-(d_i / sigma)^2 / 2), d = -(size - 1) / 2 .. (size - 1) / 2."""
    d = torch.arange((1 - size) / 2, (1 + size) / 2, 1, dtype=dtype)
    g = torch.exp(-((d / sigma) ** 2) / 2)
    return (g / g.sum() if normalise else g).unsqueeze(0)


def _images(x):
    return x.reshape(-1, *x.shape[-3:])


def _five(p, t, form, sigma, normalise, fp32):
    """The five window means of p, t, p^2, t^2, p t, [5][N, C, H', W'], and whether H', W' still carry the padding."""
    c = p.shape[1]
    g = window(sigma, normalise=normalise)
    k = torch.matmul(g.t(), g).expand(c, 1, 11, 11).contiguous()
    if form in ("reflect", "padded"):
        p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    x = torch.cat([p, t, p * p, t * t, p * t])
    out = F.conv2d(x.float(), k.float(), groups=c).double() if fp32 else F.conv2d(x, k, groups=c)
    if form == "reflect":
        out = out[..., 5:-5, 5:-5]
    return out.chunk(5)


def oracle(pred, target, data_range=None, mutate=None, form="valid"):
    """pred, target: fp32 [B, T, C, H, W] or [N, C, H, W].  -> dict of float64 values (``l1, mse, psnr, ssim, terms``, ``per_image`` [N, 3])
    and the bounds of the gate (``bound_*``).  ``form``: "valid" (the window inside the image) or "reflect" (pad by reflection, filter, crop
    the padding: pytorch_lightning's order).  ``mutate``: one of MUTATIONS."""
    assert mutate in (None,) + MUTATIONS and form in ("valid", "reflect")
    p, t = _images(pred).double(), _images(target).double()
    n_img, c, h, w = p.shape
    assert h >= 11 and w >= 11, "SSIM needs an 11 x 11 window inside the image"
    n, chw = p.numel(), c * h * w
    d = p - t
    l1_img, sq_img = d.abs().sum((1, 2, 3)), (d * d).sum((1, 2, 3))
    l1, mse = l1_img.sum() / n, sq_img.sum() / n
    if data_range is None:
        r_psnr = (p.max() - p.min()) if mutate == "psnr_range_pred" else (t.max() - t.min())
        r_ssim = torch.maximum(p.max() - p.min(), t.max() - t.min())
    else:
        r_psnr = r_ssim = torch.tensor(float(data_range), dtype=torch.float64)
    if mutate == "ssim_range_1":
        r_ssim = torch.tensor(1.0, dtype=torch.float64)
    k10 = 10.0 / math.log(10.0)
    psnr = (2 * torch.log(r_psnr) - torch.log(mse)) * k10
    c1, c2 = (0.01 * r_ssim) ** 2, (0.03 * r_ssim) ** 2
    if mutate == "c_swapped":
        c1, c2 = c2, c1
    mp, mt, epp, ett, ept = _five(p, t, "padded" if mutate == "padded_mean" else form, 1.0 if mutate == "sigma_1" else 1.5,
                                  mutate != "unnormalised", mutate == "fp32_sums")
    mpp, mtt, mpt = mp * mp, mt * mt, mp * mt
    spp, stt, spt = epp - mpp, ett - mtt, ept - mpt
    b1, b2 = mpp + mtt + c1, spp + stt + c2
    smap = ((2 * mpt + c1) * (2 * spt + c2)) / (b1 * b2)
    terms = smap[0].numel()
    ssim_img = smap.sum((1, 2, 3))
    ssim = ssim_img.sum() / smap.numel()
    out = {"l1": l1, "mse": mse, "psnr": psnr, "ssim": ssim, "terms": float(smap.numel()), "range_psnr": r_psnr, "range_ssim": r_ssim,
           "per_image": torch.stack([l1_img, sq_img, ssim_img], 1), "shape": (n_img, c, h, w), "ssim_map": smap}
    # ---- the gate's bounds (see the module docstring)
    gk = gamma(K_WINDOW)
    q = epp + ett
    e1 = (2 * gk + 2 * U) * q + 4 * U * b1
    e2 = (3 * gk + 4 * U) * q + 4 * U * b2
    r = e1 / b1 + e2 / b2
    per_pos = 2 * r / (1 - r) + 3 * U
    b_ssim_img = 2 * per_pos.sum((1, 2, 3)) + 2 * gamma(terms) * smap.abs().sum((1, 2, 3))
    out["bound_per_image"] = torch.stack([2 * gamma(chw + 3) * l1_img, 2 * gamma(chw + 3) * sq_img, b_ssim_img], 1)
    out["bound_l1"] = 2 * gamma(n + 4) * l1
    out["bound_mse"] = 2 * gamma(n + 4) * mse
    out["bound_psnr"] = 2 * (k10 * (2 * U * (1 + 2 * r_psnr.log().abs()) + gamma(n + 4) + 2 * U * mse.log().abs()) + 4 * U * psnr.abs())
    out["bound_ssim"] = (b_ssim_img.sum() + 2 * gamma(n_img) * ssim_img.abs().sum()) / smap.numel() + 2 * U * ssim.abs()
    return out


def per_image_curves(ref):
    """(psnr [N], ssim [N]) of an oracle result: the per-image PSNR uses the same R as the scalar."""
    _, c, h, w = ref["shape"]
    k10 = 10.0 / math.log(10.0)
    psnr = (2 * torch.log(ref["range_psnr"]) - torch.log(ref["per_image"][:, 1] / (c * h * w))) * k10
    return psnr, ref["per_image"][:, 2] / (c * (h - 10) * (w - 10))


def kl_oracle(mu, logvar):
    """(value, bound) of -0.5 * mean_b sum_d (1 + logvar - mu^2 - exp(logvar)) in float64."""
    mu, lv = mu.double(), logvar.double()
    value = -0.5 * torch.mean(torch.sum(1 + lv - mu.pow(2) - lv.exp(), axis=1))
    mass = (1 + lv.abs() + mu.pow(2) + lv.exp()).sum()
    return value, 2 * gamma(mu.numel() + 8) * 0.5 / mu.shape[0] * mass + 2 * U * value.abs()


# ---------------------------------------------------------------------------------------------------------------- inputs

def smooth_field(seed, shape):
    """tanh of a bilinearly upsampled 4 x 4 Gaussian grid per channel plane: [..., C, H, W] in (-1, 1)."""
    g = torch.Generator().manual_seed(seed)
    lead = int(torch.tensor(shape[:-3]).prod()) if len(shape) > 3 else 1
    grid = torch.randn(lead, shape[-3], 4, 4, generator=g)
    return torch.tanh(F.interpolate(grid, size=tuple(shape[-2:]), mode="bilinear", align_corners=True)).reshape(shape)


def pair(seed, shape, sigma, scale=1.0):
    """(real, generated) fp32: the smooth field and a noisy copy clamped to [-1, 1], both times ``scale`` (0.25 puts R near 0.5)."""
    real = smooth_field(seed, shape)
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 7919))
    gen = (real + sigma * noise).clamp(-1, 1)
    return (scale * real).float().contiguous(), (scale * gen).float().contiguous()


def families(seed, shape):
    """[(name, real, generated)]: the three noise levels at full range and the set with R near 0.5."""
    out = [(f"sigma{s}", *pair(seed + i, shape, s)) for i, s in enumerate(SIGMAS)]
    out.append(("range0.5", *pair(seed + 11, shape, 0.1, scale=0.25)))
    return out


# ---------------------------------------------------------------------------------------------------------------- gate

def gate(name, got, want, bound, verbose=True):
    """|got - want| <= bound elementwise (a NaN fails).  -> (ok, max measured / allowed, max measured, its allowed)."""
    got = torch.as_tensor(got, dtype=torch.float64).detach().cpu().reshape(-1)
    want, bound = want.detach().double().reshape(-1), torch.as_tensor(bound, dtype=torch.float64).reshape(-1)
    err = (got - want).abs()
    ok = bool((err <= bound).all())
    i = int(torch.nan_to_num(err / bound, nan=float("inf")).argmax())
    if verbose:
        print(f"  {name:<24} measured {float(err[i]):.3e}  allowed {float(bound[i]):.3e}  (rel. allowed {float(bound[i] / want[i].abs()):.2e})"
              f"{'' if ok else '  <-- FAIL'}")
    return ok, float(err[i] / bound[i]) if bound[i] > 0 else float("inf"), float(err[i]), float(bound[i])


SCALARS = ("l1", "mse", "psnr", "ssim")


def check_scalars(got, ref, verbose=True, what=""):
    """got: {l1, mse, psnr, ssim} (anything ``float64``-convertible).  Asserts the condition on the gate (relative bound < 1e-8) and returns
    {name: (ok, ratio, measured, allowed)}."""
    res = {}
    for k in SCALARS:
        rel = float(ref["bound_" + k] / ref[k].abs())
        assert rel < REL_CEILING, f"{what} {k}: the derived bound is {rel:.2e} relative, above {REL_CEILING:g}: fix the derivation or the input"
        res[k] = gate(f"{what} {k}".strip(), got[k], ref[k], ref["bound_" + k], verbose)
    return res


def all_ok(res):
    return all(v[0] for v in res.values())
