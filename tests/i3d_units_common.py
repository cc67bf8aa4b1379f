"""Shared by tests/test_host_i3d_units.py, tests/test_gpu_i3d_units.py and tests/golden/make_golden_i3d_units.py: the case lists of the
I3D unit tests, seeded inputs, plain torch float64 oracles of one conv unit, one max pool, the average pool, the time mean and one Mixed
block (written from the layer definitions: explicit ``F.pad`` with zeros, ``F.conv3d`` / ``F.max_pool3d`` in double; nothing of the
package's padding code is imported), the mutated oracles that show what the gate catches, and the gate itself.

Gate of every sum (conv, average pool, time mean), element-wise, derived and not tuned:

    |got - ref64| <= gamma(n) * S + 2^-24 * |ref64|,    gamma(n) = n u / (1 - n u),  u = 2^-24

the standard bound of a length-n fp32 dot product in ANY summation order (Higham, Accuracy and Stability of Numerical Algorithms,
eq. 3.5), S the same sum over absolute values, plus one rounding of the result.  Unit: n = padded K + 2 (K = taps x input channels
rounded up to the kernel's 16-wide chunks; + 2 for the fp32 rounding of the folded BatchNorm scale and of the shift),
S = |scale| * sum |x| |w| + |shift|.  Average pool: n = 49 kT + 1, S = mean |x|.  Time mean: n = T' + 1, S = mean |x|.  On top: the
project's relative L2 <= 1e-4 per batch row.  Max pools are compared bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

import dtfvd_common as dc
import fvd_common as fc

U = 2.0 ** -24
TOL_L2 = 1e-4
EPS = {"kin": 1e-3, "dt": 1e-5}
CLASSES = {"kin": 400, "dt": 18}      # the head with 400 and with 18 classes
WEIGHT_SEED = {"kin": 101, "dt": 102}
BRANCH = {"kin": ("branch_0", "branch_1.0", "branch_1.1", "branch_2.0", "branch_2.1", "branch_3.1"), "dt": ("b0", "b1a", "b1b", "b2a", "b2b", "b3b")}
BN_KEY = {"kin": "batch3d", "dt": "bn"}
BLOCKS = [m[0] for m in fc.MIXED]     # mixed_3b .. mixed_5c
UNIT_STEM, UNIT_2B, UNIT_2C, UNIT_MIXED, UNIT_HEAD = 0, 1, 2, 3, 57

_SD = {}


def state_dict(variant):
    """The seeded synthetic state_dict of one variant (numpy arrays), built once per process."""
    if variant not in _SD:
        _SD[variant] = (fc.i3d_state_dict if variant == "kin" else dc.dti3d_state_dict)(WEIGHT_SEED[variant], CLASSES[variant])
    return _SD[variant]


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------- units

def unit_spec(variant, unit):
    """(state_dict prefix, cin, cout, kernel, stride, has_bn) of unit index ``unit`` (the numbering of include/i2v_hip.h)."""
    cap = (lambda s: s) if variant == "kin" else (lambda s: s[0].upper() + s[1:])
    if unit == UNIT_STEM:
        return cap("conv3d_1a_7x7"), 3, 64, 7, 2, True
    if unit == UNIT_2B:
        return cap("conv3d_2b_1x1"), 64, 64, 1, 1, True
    if unit == UNIT_2C:
        return cap("conv3d_2c_3x3"), 64, 192, 3, 1, True
    if unit == UNIT_HEAD:
        return ("conv3d_0c_1x1" if variant == "kin" else "logits"), 1024, CLASSES[variant], 1, 1, False
    i, j = divmod(unit - UNIT_MIXED, 6)
    name, cin, o = fc.MIXED[i]
    cins = (cin, cin, o[1], cin, o[3], cin)
    return cap(name) + "." + BRANCH[variant][j], cins[j], o[j], 3 if j in (2, 4) else 1, 1, True


def mixed_unit(block, j):
    return UNIT_MIXED + 6 * BLOCKS.index(block) + j


def unit_params(variant, unit):
    """float64 tensors (weight [Co, Ci, k, k, k], scale [Co], shift [Co]) from the layer definition: eval-mode BatchNorm
    (x - mean) / sqrt(var + eps) * w + b, or the conv bias."""
    key, cin, cout, k, s, bn = unit_spec(variant, unit)
    sd = state_dict(variant)
    w = torch.from_numpy(sd[key + ".conv3d.weight"]).double()
    if bn:
        g, b, m, v = (torch.from_numpy(sd[f"{key}.{BN_KEY[variant]}.{n}"]).double() for n in ("weight", "bias", "running_mean", "running_var"))
        scale = g / torch.sqrt(v + EPS[variant])
        shift = b - m * scale
    else:
        scale = torch.ones(cout, dtype=torch.float64)
        shift = torch.from_numpy(sd[key + ".conv3d.bias"]).double()
    return w, scale, shift


def same_pads(variant, kernel, stride, size):
    """[(front, back)] per dimension (T, H, W) of "TF SAME" padding: k - (size % stride, or stride when that is 0) zeros in all, the
    smaller half in front.  The Kinetics modules look at size % stride in the time dimension only, the dynamic-texture ones in all."""
    pads = []
    for dim, (k, s, n) in enumerate(zip(kernel, stride, size)):
        r = n % s if (variant == "dt" or dim == 0) else 0
        total = max(k - (r if r else s), 0)
        pads.append((total // 2, total - total // 2))
    return pads


def _pad(x, pads, value=0.0):
    (t0, t1), (h0, h1), (w0, w1) = pads
    return F.pad(x, (w0, w1, h0, h1, t0, t1), value=value)


def padded_k(cin, k):
    return (k ** 3 * ((cin + 3) // 4 * 4) + 15) // 16 * 16


def unit_oracle(variant, unit, x, mutate=None):
    """One conv unit on x [B, cin, T, H, W] (any float dtype) in float64 -> (y, S, n): the output [B, cout, To, Ho, Wo], the bound
    magnitude |scale| * sum |x| |w| + |shift| and the bound length.  ``mutate`` names one deliberate error (see MUTATIONS)."""
    key, cin, cout, k, s, bn = unit_spec(variant, unit)
    w, scale, shift = unit_params(variant, unit)
    x = x.double()
    if mutate == "kinetics_rule":
        variant = "kin"
    pads = same_pads(variant, (k,) * 3, (s,) * 3, x.shape[2:])
    if mutate == "swap_front_back":
        pads = [(b, f) for f, b in pads]
    if mutate == "zero_last_cin_group":
        w = w.clone()
        w[:, -(4 if cin >= 8 else 1):] = 0
    swapped = mutate == "swap_hw_extent"
    if swapped:                         # the channels-last buffer [B][T][H][W][C] read as [B][T][W][H][C]
        B, C, T, H, W = x.shape
        x = x.permute(0, 2, 3, 4, 1).contiguous().view(B, T, W, H, C).permute(0, 4, 1, 2, 3)
        pads = [pads[0], pads[2], pads[1]]
    xp = _pad(x, pads)
    acc = F.conv3d(xp, w, stride=s)
    if mutate == "drop_border_tap":     # the first tap of every window in the last output column
        w1 = torch.zeros_like(w)
        w1[:, :, 0, 0, 0] = w[:, :, 0, 0, 0]
        acc[..., -1] -= F.conv3d(xp, w1, stride=s)[..., -1]
    y = acc * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    if unit != UNIT_HEAD:
        y = torch.relu(y)
    if swapped:                         # ... and the output written back through the same mistake
        B, Co, To, Wo, Ho = y.shape
        y = y.permute(0, 2, 3, 4, 1).contiguous().view(B, To, Ho, Wo, Co).permute(0, 4, 1, 2, 3)
    if mutate == "zero_last_cout":
        y = y.clone()
        y[:, -1] = 0
    if mutate == "zero_last_row":       # row M - 1 of the flattened [M][C] output: the last row of the last 128-position tile
        y = y.clone()
        y[-1, :, -1, -1, -1] = 0
    S = F.conv3d(xp.abs(), w.abs(), stride=s) * scale.abs().view(1, -1, 1, 1, 1) + shift.abs().view(1, -1, 1, 1, 1)
    return y, S, padded_k(cin, k) + 2


def unit_fp32(variant, unit, x):
    """The same unit in plain fp32 torch on the CPU: BatchNorm folded in double and rounded to fp32, fp32 conv3d, fp32 scale and shift."""
    key, cin, cout, k, s, bn = unit_spec(variant, unit)
    w, scale, shift = unit_params(variant, unit)
    xp = _pad(x.float(), same_pads(variant, (k,) * 3, (s,) * 3, x.shape[2:]))
    y = F.conv3d(xp, w.float(), stride=s) * scale.float().view(1, -1, 1, 1, 1) + shift.float().view(1, -1, 1, 1, 1)
    return y if unit == UNIT_HEAD else torch.relu(y)


# ---------------------------------------------------------------------------------------------------------------- pools, head

def maxpool_oracle(variant, x, kernel, stride, mutate=None):
    """Zero padding that takes part in the maximum, then MaxPool3d(ceil_mode=True): x [B, C, T, H, W] -> exact maxima, in x's dtype."""
    if mutate == "kinetics_rule":
        variant = "kin"
    pads = same_pads(variant, kernel, stride, x.shape[2:])
    if mutate == "swap_front_back":
        pads = [(b, f) for f, b in pads]
    xp = _pad(x, pads, value=float("-inf") if mutate == "neg_inf_padding" else 0.0)
    return F.max_pool3d(xp, kernel, stride, ceil_mode=mutate != "floor_mode")


def avgpool_oracle(x, kt):
    """AvgPool3d((kt, 7, 7), stride 1) on x [B, C, T, 7, 7] in float64 -> (y [B, C, T'], S, n)."""
    x = x.double()
    y = F.avg_pool3d(x, (kt, 7, 7), stride=1)[..., 0, 0]
    S = F.avg_pool3d(x.abs(), (kt, 7, 7), stride=1)[..., 0, 0]
    return y, S, 49 * kt + 1


def time_mean_oracle(x):
    """x [B, C, T'] -> (mean over T' [B, C], S, n)."""
    x = x.double()
    return x.mean(2), x.abs().mean(2), x.shape[2] + 1


def mixed_oracle(variant, block, x, first=None):
    """Mixed block on x [B, cin, T, H, W] in float64: the concatenation of the four branches, with (S, n) of the LAST conv of each
    branch.  ``first``: outputs of the first convs of branch 1 and 2 to use instead of the oracle's own (the GPU's, so that the bound
    stays per layer).  Returns [(y, S, n)] per branch."""
    u = [mixed_unit(block, j) for j in range(6)]
    t1 = unit_oracle(variant, u[1], x)[0] if first is None else first[0]
    t2 = unit_oracle(variant, u[3], x)[0] if first is None else first[1]
    pooled = maxpool_oracle(variant, x.double(), (3, 3, 3), (1, 1, 1))
    return [unit_oracle(variant, u[0], x), unit_oracle(variant, u[2], t1), unit_oracle(variant, u[4], t2), unit_oracle(variant, u[5], pooled)]


# ---------------------------------------------------------------------------------------------------------------- gate

def rel_l2_rows(got, ref):
    got, ref = got.double().reshape(got.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    return ((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).tolist()


def gate_bound(got, ref, bound):
    """(passes, worst |err| / bound, worst rel-L2 over the batch rows) for an element-wise bound.  A shape mismatch fails."""
    if tuple(got.shape) != tuple(ref.shape):
        return False, float("inf"), float("inf")
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    l2 = max(rel_l2_rows(got, ref))
    return bool(torch.isfinite(got).all()) and ratio <= 1.0 and l2 <= TOL_L2, ratio, l2


def gate(got, ref, S, n):
    """The gate of one sum of length n: |got - ref| <= gamma(n) S + u |ref| element-wise and rel-L2 <= 1e-4 per batch row."""
    return gate_bound(got, ref, gamma(n) * S + U * ref.abs())


# ---------------------------------------------------------------------------------------------------------------- inputs, cases

def randn(seed, shape, negative=False):
    """Seeded fp32 N(0, 1) values (O(1), never subnormal: |x| >= 2^-20 is enforced); ``negative``: -|x|."""
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    x = np.where(np.abs(x) < 2.0 ** -20, np.float32(2.0 ** -20), x).astype(np.float32)
    return torch.from_numpy(-np.abs(x) if negative else x)


def unit_input(case):
    """x [B, cin, T, H, W] fp32 of a unit case (the stem: 3 channels; the GPU test appends the 4th channel of its input layout)."""
    variant, unit, (B, T, H, W) = case["variant"], case["unit"], case["shape"]
    cin = unit_spec(variant, unit)[1]
    return randn(case["seed"], (B, cin, T, H, W))


M_LADDER = ((1, 2, 5, 5), (1, 2, 8, 8), (2, 1, 5, 13), (3, 3, 7, 6))   # M = 50, 128, 130, 378 against the 128-row tile
REST = (2, 3, 6, 5)
STEM_SHAPES = ((2, 9, 12, 9), (2, 8, 12, 9), (2, 2, 7, 16))


def _case(variant, unit, shape, seed):
    key = unit_spec(variant, unit)[0]
    return {"id": f"{variant}-{key}-{'x'.join(map(str, shape))}", "variant": variant, "unit": unit, "shape": tuple(shape), "seed": seed}


def unit_cases():
    cases, seed = [], 1000
    # the M ladder on one unit per column template: BN = 32 (480 -> 96), 64 (64 -> 64), 128 (256 -> 128)
    for unit in (mixed_unit("mixed_4b", 1), UNIT_2B, mixed_unit("mixed_3c", 0)):
        for shape in M_LADDER:
            cases.append(_case("kin", unit, shape, seed := seed + 1))
    rest = [mixed_unit(b, j) for b in ("mixed_3b", "mixed_4b", "mixed_4c", "mixed_5c") for j in (2, 4)]   # 3x3x3: cin 96, 16, 96, 16, 112, 24, 192, 48
    rest += [UNIT_2C, mixed_unit("mixed_4e", 2)]                                                         # 64 -> 192, 144 -> 288 (3x3x3)
    rest += [mixed_unit("mixed_3b", 3), mixed_unit("mixed_4c", 3), mixed_unit("mixed_4b", 1), mixed_unit("mixed_4c", 1),
             mixed_unit("mixed_4e", 1), mixed_unit("mixed_5c", 0)]                                       # 1x1: cout 16, 24, 96 (feeds 208), 112, 144, 384
    for variant in ("kin", "dt"):
        for unit in rest:
            cases.append(_case(variant, unit, REST, seed := seed + 1))
        for shape in ((2, 1, 1, 1), (2, 3, 1, 1)):                                                       # the head: 400 and 18 classes
            cases.append(_case(variant, UNIT_HEAD, shape, seed := seed + 1))
        for shape in STEM_SHAPES:
            cases.append(_case(variant, UNIT_STEM, shape, seed := seed + 1))
    return cases


MIXED_CASES = [{"id": f"{v}-{b}-{'x'.join(map(str, s))}", "variant": v, "block": b, "shape": s, "seed": 2000 + 10 * i + j + 100 * k}
               for k, v in enumerate(("kin", "dt")) for i, b in enumerate(("mixed_3b", "mixed_4b", "mixed_4c"))
               for j, s in enumerate(((2, 3, 5, 4), (1, 1, 7, 7)))]

POOLS = [((1, 3, 3), (1, 2, 2), (1, 7, 10)), ((1, 3, 3), (1, 2, 2), (1, 8, 14)),
         ((3, 3, 3), (2, 2, 2), (4, 6, 7)), ((3, 3, 3), (2, 2, 2), (5, 6, 7)),
         ((2, 2, 2), (2, 2, 2), (3, 14, 5)), ((2, 2, 2), (2, 2, 2), (4, 14, 5)),
         ((3, 3, 3), (1, 1, 1), (1, 5, 6)), ((3, 3, 3), (1, 1, 1), (2, 5, 6)), ((3, 3, 3), (1, 1, 1), (3, 5, 6))]


def pool_cases(channels=(64, 528), batch=2):
    cases, seed = [], 3000
    for variant in ("kin", "dt"):
        for kernel, stride, thw in POOLS:
            for C in channels:
                for negative in (False, True):
                    seed += 1
                    cases.append({"id": f"{variant}-k{''.join(map(str, kernel))}s{''.join(map(str, stride))}-{'x'.join(map(str, thw))}-c{C}-"
                                        f"{'neg' if negative else 'rnd'}", "variant": variant, "kernel": kernel, "stride": stride,
                                  "shape": (batch, C, *thw), "negative": negative, "seed": seed})
    return cases


def pool_input(case):
    return randn(case["seed"], case["shape"], case["negative"])


HEAD_CASES = [{"id": f"{v}-pool{kt}-t{t}", "variant": v, "length": length, "pool_t": kt, "shape": (3, t), "seed": 4000 + 10 * kt + t}
              for v, length, kt, ts in (("kin", None, 2, (2, 3, 5)), ("dt", 16, 2, (2, 3, 5)), ("dt", 32, 4, (4, 6))) for t in ts]

# deliberate errors the gate has to catch: name -> the kinds of case it applies to
MUTATIONS = {"drop_border_tap": "conv", "swap_front_back": "conv+pool", "swap_hw_extent": "conv", "zero_last_cin_group": "conv",
             "zero_last_cout": "conv", "zero_last_row": "conv", "neg_inf_padding": "pool", "floor_mode": "pool", "kinetics_rule": "conv+pool"}


# the thinned list of the committed fixture (tests/golden/i3d_units.npz): batch 1 and small maps, the oracles do not depend on either
def fixture_cases():
    units, seed = [], 5000
    for variant in ("kin", "dt"):
        for shape in ((1, 9, 12, 9), (1, 2, 7, 16)):
            units.append(_case(variant, UNIT_STEM, shape, seed := seed + 1))
        for unit in (mixed_unit("mixed_3b", 4), mixed_unit("mixed_3b", 3), UNIT_2B):
            units.append(_case(variant, unit, (1, 3, 6, 5), seed := seed + 1))
        units.append(_case(variant, UNIT_HEAD, (2, 3, 1, 1), seed := seed + 1))
    mixed = [{"id": f"{v}-mixed_3b-1x2x3x2", "variant": v, "block": "mixed_3b", "shape": (1, 2, 3, 2), "seed": 5100 + k}
             for k, v in enumerate(("kin", "dt"))]
    return units, mixed, pool_cases(channels=(4,), batch=1)
