"""Shared by tests/test_host_fid.py, tests/test_gpu_fid.py and tests/golden/make_golden_fid.py: a numpy-only, seeded synthesiser of the FID
Inception-v3 ``state_dict`` under torchvision's keys (94 BasicConv2d units and the 1008-class ``fc``: 23.9 M parameters, about 96 MB -- never
committed, always regenerated), and plain torch float64 oracles of one BasicConv2d, the three pools, the global average, the input stage,
every Mixed block and the trunk, written from the layer table of the issue.  Nothing of the package is imported.

Gate of one convolution, element-wise (``i3d_units_common.gate``, derived there): |got - ref64| <= gamma(n) S + 2^-24 |ref64| with
n = padded K + 1 (K = taps x stored input channels, rounded up to the kernel's 16-wide chunks; + 1 for the fp32 rounding of the folded
BatchNorm scale -- the rounding of the shift is covered by |shift| in S, the final fma by the 2^-24 |ref64| term) and
S = |scale| sum |x| |w| + |shift|; on top relative L2 <= 1e-4 per batch row.  ReLU is 1-Lipschitz, so the bound holds behind it.
Average pools: n = taps + 1 (the sum and the division), S = mean |x|.  Max pools are compared bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

from fvd_common import clips, load_fixture  # noqa: F401  (re-exported)
from i3d_units_common import U, TOL_L2, gamma, gate, gate_bound, randn, rel_l2_rows  # noqa: F401  (the gate is reused by import)

BN_EPS = 1e-3
FID_FILE = "pt_inception-2015-12-05-6726825d.pth"
POOL_MAX_S2, POOL_MAX_S1, POOL_AVG = 0, 1, 2
BLOCK_CHANNELS = (64, 192, 768, 2048)

STEM = (("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)), ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
        ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)), ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0)))
# name -> (kind, cin, parameter: pool_features / channels_7x7 / the pool of an E block)
MIXED = (("Mixed_5b", "A", 192, 32), ("Mixed_5c", "A", 256, 64), ("Mixed_5d", "A", 288, 64), ("Mixed_6a", "B", 288, None),
         ("Mixed_6b", "C", 768, 128), ("Mixed_6c", "C", 768, 160), ("Mixed_6d", "C", 768, 160), ("Mixed_6e", "C", 768, 192),
         ("Mixed_7a", "D", 768, None), ("Mixed_7b", "E", 1280, POOL_AVG), ("Mixed_7c", "E", 2048, POOL_MAX_S1))
BLOCK_NAMES = [m[0] for m in MIXED]

_1, _0 = (1, 1), (0, 0)


def block_units(kind, cin, par):
    """{suffix: (cin, cout, kernel, stride, padding)} of one block kind, in torchvision's order."""
    if kind == "A":
        return {"branch1x1": (cin, 64, _1, 1, _0), "branch5x5_1": (cin, 48, _1, 1, _0), "branch5x5_2": (48, 64, (5, 5), 1, (2, 2)),
                "branch3x3dbl_1": (cin, 64, _1, 1, _0), "branch3x3dbl_2": (64, 96, (3, 3), 1, _1), "branch3x3dbl_3": (96, 96, (3, 3), 1, _1),
                "branch_pool": (cin, par, _1, 1, _0)}
    if kind == "B":
        return {"branch3x3": (cin, 384, (3, 3), 2, _0), "branch3x3dbl_1": (cin, 64, _1, 1, _0), "branch3x3dbl_2": (64, 96, (3, 3), 1, _1),
                "branch3x3dbl_3": (96, 96, (3, 3), 2, _0)}
    if kind == "C":
        c7 = par
        return {"branch1x1": (cin, 192, _1, 1, _0), "branch7x7_1": (cin, c7, _1, 1, _0), "branch7x7_2": (c7, c7, (1, 7), 1, (0, 3)),
                "branch7x7_3": (c7, 192, (7, 1), 1, (3, 0)), "branch7x7dbl_1": (cin, c7, _1, 1, _0), "branch7x7dbl_2": (c7, c7, (7, 1), 1, (3, 0)),
                "branch7x7dbl_3": (c7, c7, (1, 7), 1, (0, 3)), "branch7x7dbl_4": (c7, c7, (7, 1), 1, (3, 0)),
                "branch7x7dbl_5": (c7, 192, (1, 7), 1, (0, 3)), "branch_pool": (cin, 192, _1, 1, _0)}
    if kind == "D":
        return {"branch3x3_1": (cin, 192, _1, 1, _0), "branch3x3_2": (192, 320, (3, 3), 2, _0), "branch7x7x3_1": (cin, 192, _1, 1, _0),
                "branch7x7x3_2": (192, 192, (1, 7), 1, (0, 3)), "branch7x7x3_3": (192, 192, (7, 1), 1, (3, 0)),
                "branch7x7x3_4": (192, 192, (3, 3), 2, _0)}
    return {"branch1x1": (cin, 320, _1, 1, _0), "branch3x3_1": (cin, 384, _1, 1, _0), "branch3x3_2a": (384, 384, (1, 3), 1, (0, 1)),
            "branch3x3_2b": (384, 384, (3, 1), 1, (1, 0)), "branch3x3dbl_1": (cin, 448, _1, 1, _0), "branch3x3dbl_2": (448, 384, (3, 3), 1, _1),
            "branch3x3dbl_3a": (384, 384, (1, 3), 1, (0, 1)), "branch3x3dbl_3b": (384, 384, (3, 1), 1, (1, 0)),
            "branch_pool": (cin, 192, _1, 1, _0)}


def block_branches(kind, par):
    """[(steps in front, last steps)] per branch in concatenation order: a step is a unit suffix or a pool kind (int); every last step
    contributes one channel slice of the output."""
    if kind == "A":
        return [([], ["branch1x1"]), (["branch5x5_1"], ["branch5x5_2"]), (["branch3x3dbl_1", "branch3x3dbl_2"], ["branch3x3dbl_3"]),
                ([POOL_AVG], ["branch_pool"])]
    if kind == "B":
        return [([], ["branch3x3"]), (["branch3x3dbl_1", "branch3x3dbl_2"], ["branch3x3dbl_3"]), ([], [POOL_MAX_S2])]
    if kind == "C":
        return [([], ["branch1x1"]), (["branch7x7_1", "branch7x7_2"], ["branch7x7_3"]),
                (["branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4"], ["branch7x7dbl_5"]), ([POOL_AVG], ["branch_pool"])]
    if kind == "D":
        return [(["branch3x3_1"], ["branch3x3_2"]), (["branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3"], ["branch7x7x3_4"]), ([], [POOL_MAX_S2])]
    return [([], ["branch1x1"]), (["branch3x3_1"], ["branch3x3_2a", "branch3x3_2b"]),
            (["branch3x3dbl_1", "branch3x3dbl_2"], ["branch3x3dbl_3a", "branch3x3dbl_3b"]), ([par], ["branch_pool"])]


def units():
    """[(torchvision key, cin, cout, kernel, stride, padding)] of all 94 BasicConv2d units, in torchvision's state_dict order."""
    out = list(STEM)
    for name, kind, cin, par in MIXED:
        out += [(f"{name}.{s}", *v) for s, v in block_units(kind, cin, par).items()]
    return out


UNITS = {u[0]: u[1:] for u in units()}
_SD = {}


def fid_state_dict(seed):
    """Seeded weights under torchvision's keys, cached per seed: conv weights N(0, 2 / fan_in) (the ReLU-preserving scale: activations stay
    O(1) through 47 conv layers), BatchNorm weight in [0.8, 1.2], bias and running_mean N(0, 0.1^2), running_var in [0.5, 1.5],
    ``num_batches_tracked`` and the checkpoint's 1008-class ``fc`` (ignored by the trunk)."""
    if seed not in _SD:
        rng = np.random.default_rng(seed)
        sd = {}
        for key, cin, cout, (kh, kw), _, _ in units():
            sd[key + ".conv.weight"] = (rng.standard_normal((cout, cin, kh, kw)) * np.sqrt(2.0 / (cin * kh * kw))).astype(np.float32)
            sd[key + ".bn.weight"] = rng.uniform(0.8, 1.2, cout).astype(np.float32)
            sd[key + ".bn.bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            sd[key + ".bn.running_mean"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            sd[key + ".bn.running_var"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
            sd[key + ".bn.num_batches_tracked"] = np.asarray(0, dtype=np.int64)
        sd["fc.weight"] = (rng.standard_normal((1008, 2048)) * 0.02).astype(np.float32)
        sd["fc.bias"] = np.zeros(1008, dtype=np.float32)
        _SD[seed] = sd
    return _SD[seed]


def torch_state_dict(seed):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in fid_state_dict(seed).items()}


def holder_keys(seed=0):
    """[[key, shape]] of the holder's state_dict: every unit's entries, without ``fc.*``."""
    return [[k, list(np.shape(v))] for k, v in fid_state_dict(seed).items() if not k.startswith("fc.")]


def save_fid_file(path, seed):
    torch.save(torch_state_dict(seed), path)


def unit_params(sd, key):
    """(weight [Co, Ci, kh, kw] float64, (bn weight, bias, running_mean, running_var) float32 numpy) of unit ``key``."""
    return torch.from_numpy(sd[key + ".conv.weight"]).double(), tuple(sd[f"{key}.bn.{n}"] for n in ("weight", "bias", "running_mean", "running_var"))


# ---------------------------------------------------------------------------------------------------------------- oracles

def padded_k(cin, kh, kw):
    return (kh * kw * ((cin + 3) // 4 * 4) + 15) // 16 * 16


def conv_oracle(x, w, bn, stride=1, padding=(0, 0), eps=BN_EPS, mutate=None):
    """One BasicConv2d on x [N, cin, H, W] in float64 -> (y, S, n): relu(bn(conv(x))) with eval-mode BatchNorm
    (x - mean) / sqrt(var + eps) * weight + bias.  ``mutate``: "bn_eps" (1e-5), "swap_kernel" (a (1, k) window applied as (k, 1))."""
    x, w = x.double(), torch.as_tensor(w).double()
    g, b, m, v = (torch.as_tensor(np.asarray(t)).double() for t in bn)
    if mutate == "bn_eps":
        eps = 1e-5
    wm, pad = w, tuple(padding)
    if mutate == "swap_kernel" and w.shape[2] != w.shape[3]:
        wm, pad = w.transpose(2, 3), (padding[1], padding[0])
    scale = g / torch.sqrt(v + eps)
    shift = b - m * scale
    y = torch.relu(F.conv2d(x, wm, stride=stride, padding=pad) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    S = F.conv2d(x.abs(), w.abs(), stride=stride, padding=tuple(padding)) * scale.abs().view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
    return y, S, padded_k(w.shape[1], w.shape[2], w.shape[3]) + 1


def unit_oracle(sd, key, x, mutate=None):
    cin, cout, kernel, stride, padding = UNITS[key]
    w, bn = unit_params(sd, key)
    return conv_oracle(x, w, bn, stride, padding, mutate=mutate)


def pool_oracle(x, kind, mutate=None):
    """(y, S, n) of one 3 x 3 pool; the max pools are exact (S None, n 0).  ``mutate``: "zero_pad_max" (zeros take part in pool (b)),
    "ceil_mode" (pool (a)), "count_pad" (pool (c) divides by 9 everywhere)."""
    if kind == POOL_MAX_S2:
        return F.max_pool2d(x, 3, 2, ceil_mode=mutate == "ceil_mode"), None, 0
    if kind == POOL_MAX_S1:
        return (F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 1) if mutate == "zero_pad_max" else F.max_pool2d(x, 3, 1, 1)), None, 0
    x = x.double()
    inc = mutate == "count_pad"
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=inc), F.avg_pool2d(x.abs(), 3, 1, 1, count_include_pad=inc), 10


def global_avg_oracle(x):
    """AdaptiveAvgPool2d((1, 1)) on x [N, C, H, W] in float64 -> (y [N, C], S, n)."""
    x = x.double()
    return x.mean((2, 3)), x.abs().mean((2, 3)), x.shape[2] * x.shape[3] + 1


def input_oracle(frames, resize=True, normalize=False, align_corners=False):
    """InceptionV3.forward's input stage on frames [N, 3, H, W] in float64."""
    x = frames.double()
    if resize:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=align_corners)
    return 2 * x - 1 if normalize else x


def _step(sd, name, step, h, mutate):
    if isinstance(step, int):
        m = {"avg_count_pad": "count_pad", "zero_pad_max": "zero_pad_max"}.get(mutate)
        return pool_oracle(h.double(), step, m)
    m = {"bn_eps": "bn_eps", "swap_1x7_7x1": "swap_kernel"}.get(mutate)
    return unit_oracle(sd, f"{name}.{step}", h, m)


def mixed_oracle(sd, block, x, mutate=None, first=None):
    """Mixed block ``block`` (a name of BLOCK_NAMES) on x [N, cin, H, W] in float64 -> [(y, S, n)] per channel slice, in concatenation
    order (a max pool slice: S None, exact).  ``first``: per branch the input of its last step(s) to use instead of the oracle's own (the
    GPU's intermediates, so that the bound stays per layer; None for a branch without steps in front).  ``mutate``: one deliberate error
    ("bn_eps", "avg_count_pad", "zero_pad_max", "e2_avg", "swap_1x7_7x1", "cat_order")."""
    name, kind, cin, par = MIXED[BLOCK_NAMES.index(block)]
    if mutate == "e2_avg" and kind == "E":
        par = POOL_AVG
    out = []
    for bi, (pre, lasts) in enumerate(block_branches(kind, par)):
        h = x.double()
        if first is not None and pre:
            h = first[bi].double()
        else:
            for step in pre:
                h = _step(sd, name, step, h, mutate)[0]
        out += [_step(sd, name, step, h, mutate) for step in lasts]
    if mutate == "cat_order":
        out[0], out[1] = out[1], out[0]
    return out


def mixed_cat(slices):
    return torch.cat([s[0].double() for s in slices], 1)


def trunk_oracle(sd, x, mutate=None, last=3):
    """The output blocks 0..last of x [N, 3, H, W] (behind the input stage) in float64: [N, 64, ., .], [N, 192, ., .], [N, 768, ., .] and
    [N, 2048, 1, 1]."""
    m = "bn_eps" if mutate == "bn_eps" else None
    h, blocks = x.double(), []
    for key in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        h = unit_oracle(sd, key, h, m)[0]
    h = F.max_pool2d(h, 3, 2)
    blocks.append(h)
    if last >= 1:
        for key in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
            h = unit_oracle(sd, key, h, m)[0]
        h = F.max_pool2d(h, 3, 2)
        blocks.append(h)
    if last >= 2:
        for name in BLOCK_NAMES[:8]:
            h = mixed_cat(mixed_oracle(sd, name, h, mutate))
        blocks.append(h)
    if last >= 3:
        for name in BLOCK_NAMES[8:]:
            h = mixed_cat(mixed_oracle(sd, name, h, mutate))
        blocks.append(h.mean((2, 3), keepdim=True))
    return blocks


def frechet_stats(act):
    act = np.asarray(act, dtype=np.float64)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def to_cl(x, pad4=False):
    """[N, C, H, W] -> contiguous channels-last [N, H, W, C]; ``pad4``: a zero 4th channel behind 3."""
    y = x.permute(0, 2, 3, 1)
    if pad4:
        y = torch.cat([y, torch.zeros_like(y[..., :1])], -1)
    return y.contiguous()


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- cases

# (kernel, stride, padding) of every conv shape of the network
CONV_KINDS = (((3, 3), 2, (0, 0)), ((3, 3), 1, (0, 0)), ((3, 3), 1, (1, 1)), ((1, 1), 1, (0, 0)), ((5, 5), 1, (2, 2)), ((1, 7), 1, (0, 3)),
              ((7, 1), 1, (3, 0)), ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0)))
CONV_CIN = (3, 16, 48, 80)
CONV_COUT = (32, 48, 96, 192)      # 48 is ragged against every column tile, 192 uses more than one (128 and 384: appended in conv_cases)
CONV_MAPS = ((5, 7), (8, 16), (9, 17), (17, 33))   # below one position tile, exactly 128, one past it, ragged multi-tile (at stride 1, pad "same")
CONV_BATCH = (1, 3)


def conv_cases():
    """A pruned cross product: every kind on two maps (stride 2 on an odd and an even extent) with the other axes cycling, so that every
    value of every axis occurs several times; slices on a third of the cases."""
    cases, seed, i = [], 11000, 0
    for ki, (kernel, stride, padding) in enumerate(CONV_KINDS):
        for mi in range(4):
            hw = CONV_MAPS[(ki + mi) % 4]
            if mi >= 2 and stride == 1 and ki not in (2, 3):
                continue
            cin, cout, b = CONV_CIN[(i + ki) % 4], CONV_COUT[(i // 2 + mi) % 4], CONV_BATCH[i % 2]
            seed += 1
            cases.append({"id": f"k{kernel[0]}x{kernel[1]}s{stride}p{padding[0]}{padding[1]}-c{cin}-{cout}-{hw[0]}x{hw[1]}-b{b}"
                                + ("-slice" if i % 3 == 0 else ""), "kernel": kernel, "stride": stride, "padding": padding, "cin": cin, "cout": cout,
                          "hw": hw, "batch": b, "seed": seed, "slices": i % 3 == 0})
            i += 1
    # Cout 128 and 384 are the widths that take the 128-column tile (and its second weight piece per thread): a 1x1, a 1x7 and a stride-2
    # 3x3 window on a multi-tile map, one of them through channel slices
    for kernel, stride, padding, cin, cout, hw, b, sl in (((1, 1), 1, (0, 0), 48, 128, (9, 17), 3, False), ((1, 7), 1, (0, 3), 16, 128, (17, 33), 1, True),
                                                          ((3, 3), 2, (0, 0), 80, 384, (17, 33), 3, False)):
        seed += 1
        cases.append({"id": f"k{kernel[0]}x{kernel[1]}s{stride}p{padding[0]}{padding[1]}-c{cin}-{cout}-{hw[0]}x{hw[1]}-b{b}" + ("-slice" if sl else ""),
                      "kernel": kernel, "stride": stride, "padding": padding, "cin": cin, "cout": cout, "hw": hw, "batch": b, "seed": seed, "slices": sl})
    return cases


def conv_params(case):
    rng = np.random.default_rng(case["seed"] + 100000)
    cin, cout, (kh, kw) = case["cin"], case["cout"], case["kernel"]
    w = (rng.standard_normal((cout, cin, kh, kw)) * np.sqrt(2.0 / (cin * kh * kw))).astype(np.float32)
    bn = (rng.uniform(0.8, 1.2, cout).astype(np.float32), (rng.standard_normal(cout) * 0.1).astype(np.float32),
          (rng.standard_normal(cout) * 0.1).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32))
    return torch.from_numpy(w), bn


def conv_input(case):
    return randn(case["seed"], (case["batch"], case["cin"], *case["hw"]))


MAXPOOL_MAPS = ((7, 9), (8, 10), (3, 3), (17, 16))     # odd / even extents, the smallest map of pool (a), a multi-block one
AVGPOOL_MAPS = ((1, 1), (1, 5), (2, 2), (5, 6), (17, 17))
# block -> (batch, map) of the Mixed test: the network's channel counts on small maps
MIXED_CASES = [(n, 2, {"A": (5, 6), "B": (7, 9), "C": (5, 6), "D": (7, 9), "E": (3, 4)}[k]) for n, k, _, _ in MIXED]
MUTATIONS = ("bn_eps", "avg_count_pad", "zero_pad_max", "e2_avg", "swap_1x7_7x1", "cat_order")
