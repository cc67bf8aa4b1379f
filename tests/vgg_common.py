"""Shared by tests/test_host_vgg.py, tests/test_gpu_vgg.py and tests/golden/make_golden_vgg.py: a numpy-only, seeded synthesiser of
torchvision's VGG-16 ``state_dict`` (the thirteen ``features.N`` convolutions: 14.7 M parameters, about 59 MB -- never committed, always
regenerated) and of non-negative LPIPS ``lin`` weights, and plain torch float64 oracles of one convolution, the max pool, the input
stage, the trunk, LPIPS and the diversity pair mean, written from the layer definitions.  Nothing of the package is imported.

Gate of one convolution, element-wise (``i3d_units_common.gate``, derived there): |got - ref64| <= gamma(n) S + 2^-24 |ref64| with
n = 9 x (input channels as stored: 3 -> 4) + 1 (the bias add) and S = sum |x| |w| + |b|; on top relative L2 <= 1e-4 per batch row.
ReLU is 1-Lipschitz, so the bound of the sum holds behind it."""
import numpy as np
import torch
import torch.nn.functional as F

from fvd_common import clips, load_fixture  # noqa: F401  (re-exported)
from i3d_units_common import U, TOL_L2, gamma, gate, gate_bound, randn, rel_l2_rows  # noqa: F401  (the gate is reused by import)

# torchvision vgg16().features: (index, cin, cout) of every conv; a MaxPool2d(2, 2) sits at 4, 9, 16, 23 (and 30, unused)
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512), (19, 512, 512),
         (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
POOL_AFTER = (2, 7, 14, 21)
TAP_AFTER = (2, 7, 14, 21, 28)
TAPS = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
CHNS = (64, 128, 256, 512, 512)
# the reference module's slices: slice k holds the torchvision indices of SLICES[k] (vgg16.py:16-25)
SLICES = (range(0, 4), range(4, 9), range(9, 16), range(16, 23), range(23, 30))
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

_SD = {}


def vgg_state_dict(seed):
    """torchvision keys ``features.N.weight`` N(0, 2 / fan_in) and ``features.N.bias`` N(0, 0.1^2), float32, cached per seed."""
    if seed not in _SD:
        rng = np.random.default_rng(seed)
        sd = {}
        for idx, cin, cout in CONVS:
            sd[f"features.{idx}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9))).astype(np.float32)
            sd[f"features.{idx}.bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        _SD[seed] = sd
    return _SD[seed]


def lin_state_dict(seed):
    """``lin{k}.model.1.weight`` [1, C, 1, 1]: non-negative (|N(0, 1)| / C), as the trained LPIPS weights are."""
    rng = np.random.default_rng(seed)
    return {f"lin{k}.model.1.weight": (np.abs(rng.standard_normal((1, c, 1, 1))) / c).astype(np.float32) for k, c in enumerate(CHNS)}


def holder_keys():
    """The reference ``vgg16().state_dict()`` key list: slice{k}.{torchvision index}.{weight,bias}."""
    keys = []
    for idx, _, _ in CONVS:
        k = next(i for i, r in enumerate(SLICES) if idx in r)
        keys += [f"slice{k + 1}.{idx}.weight", f"slice{k + 1}.{idx}.bias"]
    return keys


def lpips_keys():
    return (["scaling_layer.shift", "scaling_layer.scale"] + ["net." + k for k in holder_keys()] + [f"lin{k}.model.1.weight" for k in range(5)])


def save_torchvision_file(path, seed):
    torch.save({k: torch.from_numpy(v) for k, v in vgg_state_dict(seed).items()}, path)


def save_lin_file(path, seed):
    torch.save({k: torch.from_numpy(v) for k, v in lin_state_dict(seed).items()}, path)


# ---------------------------------------------------------------------------------------------------------------- oracles

def padded_k(cin):
    return 9 * (4 if cin == 3 else cin)


def conv_oracle(x, w, b, mutate=None):
    """relu(conv2d(x, w, padding=1) + b) on x [N, cin, H, W] in float64 -> (y, S, n).  ``mutate`` names one deliberate error."""
    x, w, b = x.double(), torch.as_tensor(w).double(), torch.as_tensor(b).double()
    wm = w
    if mutate == "swap_dhdw":
        wm = w.transpose(2, 3)
    if mutate == "transposed_kernel":        # [cout][cin] read as [cin][cout] (needs cin = cout)
        wm = w.transpose(0, 1)
    acc = F.conv2d(x, wm, padding=1)
    if mutate == "drop_border_tap":          # tap (0, 0) of every window in the last output column
        w1 = torch.zeros_like(w)
        w1[:, :, 0, 0] = w[:, :, 0, 0]
        acc[..., -1] -= F.conv2d(x, w1, padding=1)[..., -1]
    bias = b.view(1, -1, 1, 1)
    if mutate == "missing_bias":
        y = torch.relu(acc)
    elif mutate == "relu_before_bias":
        y = torch.relu(acc) + bias
    else:
        y = torch.relu(acc + bias)
    S = F.conv2d(x.abs(), w.abs(), padding=1) + bias.abs()
    return y, S, padded_k(w.shape[1]) + 1


def maxpool_oracle(x, mutate=None):
    return F.max_pool2d(x, 2, 1 if mutate == "pool_stride1" else 2)


def input_oracle(frames, mode, size=None, align_corners=False):
    """The input stage on frames [N, 3, H, W] in float64 (the constants are the fp32 values the modules hold).  ``mode`` "lpips":
    (x - shift) / scale; "diversity": ((x + 1) / 2 - mean) / std, then F.interpolate(size, bilinear, align_corners)."""
    x = frames.double()
    c = lambda v: torch.tensor(v, dtype=torch.float32).double().view(1, 3, 1, 1)  # noqa: E731
    if mode == "lpips":
        return (x - c(LPIPS_SHIFT)) / c(LPIPS_SCALE)
    y = ((x + 1) / 2 - c(IMAGENET_MEAN)) / c(IMAGENET_STD)
    return F.interpolate(y, size=size, mode="bilinear", align_corners=align_corners)


def trunk_oracle(sd, x):
    """The five taps [N, C, H', W'] of x [N, 3, H, W] (already normalised) in float64."""
    h, taps = x.double(), []
    for idx, _, _ in CONVS:
        h = torch.relu(F.conv2d(h, torch.from_numpy(sd[f"features.{idx}.weight"]).double(), torch.from_numpy(sd[f"features.{idx}.bias"]).double(),
                                padding=1))
        if idx in TAP_AFTER:
            taps.append(h)
        if idx in POOL_AFTER:
            h = F.max_pool2d(h, 2, 2)
    return taps


def lpips_layer_oracle(f0, f1, lin, eps=1e-10):
    """One layer of LPIPS.forward on taps [N, C, H, W] in float64 -> [N]."""
    f0, f1 = f0.double(), f1.double()
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + eps)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + eps)
    return (((n0 - n1) ** 2) * lin.double().view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_oracle(sd, lin, x0, x1):
    t0, t1 = trunk_oracle(sd, input_oracle(x0, "lpips")), trunk_oracle(sd, input_oracle(x1, "lpips"))
    return sum(lpips_layer_oracle(a, b, torch.from_numpy(lin[f"lin{k}.model.1.weight"]).flatten()) for k, (a, b) in enumerate(zip(t0, t1)))


def lpips_score_rule(per_image, batch=10):
    """The reference CLI's rule (eval_synthesis_quality.py:85-89): the mean over floor(n / 10) batch means, the ragged tail dropped."""
    per_image = np.asarray(per_image, dtype=np.float64)
    nb = per_image.shape[0] // batch
    return float(np.mean([per_image[i * batch:(i + 1) * batch].mean() for i in range(nb)]))


def pair_mean(fmaps, r, t):
    """metrics/Diversity/VGG.py:36-43 for one video: fmaps = five taps of the R * T images [R * T, C, H, W] -> the list of the
    R (R - 1) * 5 terms ((f[i] - f[j]) ** 2).mean() in the reference's order."""
    div = []
    for i in range(r):
        for j in range(r):
            if i != j:
                for fm in fmaps:
                    f = fm.reshape(r, t, *fm.shape[1:])
                    div.append(float(((f[i] - f[j]) ** 2).mean()))
    return div


def diversity_oracle(sd, videos, align_corners=False):
    """compute_vgg_diversity on videos [N, R, T, 3, H, W] in [-1, 1], float64: the mean over the N R (R - 1) 5 terms."""
    n, r, t = videos.shape[:3]
    div = []
    for video in videos.double():
        x = input_oracle(video.reshape(-1, *video.shape[2:]), "diversity", (224, 224), align_corners)
        div += pair_mean(trunk_oracle(sd, x), r, t)
    return float(np.mean(div))


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

CONV_SHAPES = ((5, 7), (8, 16), (9, 17), (17, 33), (13, 21))   # below one tile, one tile, one past it in both, 3 x 3 tiles ragged, ragged
CONV_BATCH = (1, 3)
CONV_CIN = (3, 16, 48, 64)       # the 4-channel instantiation; one chunk; an odd chunk count; four chunks
CONV_COUT = (64, 128)


def conv_cases():
    cases, seed = [], 7000
    for cin in CONV_CIN:
        for cout in CONV_COUT:
            for hw in CONV_SHAPES:
                for b in CONV_BATCH:
                    seed += 1
                    cases.append({"id": f"c{cin}-{cout}-{hw[0]}x{hw[1]}-b{b}", "cin": cin, "cout": cout, "hw": hw, "batch": b, "seed": seed})
    return cases


def conv_params(case):
    rng = np.random.default_rng(case["seed"] + 100000)
    w = (rng.standard_normal((case["cout"], case["cin"], 3, 3)) * np.sqrt(2.0 / (9 * case["cin"]))).astype(np.float32)
    b = (rng.standard_normal(case["cout"]) * 0.1).astype(np.float32)
    return torch.from_numpy(w), torch.from_numpy(b)


def conv_input(case):
    return randn(case["seed"], (case["batch"], case["cin"], *case["hw"]))


MUTATIONS = ("drop_border_tap", "swap_dhdw", "transposed_kernel", "missing_bias", "relu_before_bias")
