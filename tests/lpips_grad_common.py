"""Shared by tests/test_host_lpips_grad.py, tests/test_gpu_lpips_grad.py and tests/golden/make_golden_lpips_grad.py: plain torch float64
oracles of the LPIPS backward pass (the input gradient of one 3x3 convolution, the max-pool backward, the LPIPS head backward, the
trunk with the ReLU masks and pool arg-max GIVEN), the deliberate errors the gates have to catch, and the case lists.  ``vgg_common`` is
imported unchanged; nothing of the package is imported.

Input gradient of a convolution.  y = conv2d(x, w, padding=1) with w [Cout, Cin, 3, 3] has dL/dx = conv2d(g, w.transpose(0, 1).flip(2, 3),
padding=1): the same convolution with the kernel transposed and the taps flipped (``test_host_lpips_grad`` checks the identity against
autograd).  Each output element is a dot product of length K = 9 Cout, so the gate is the one of the forward (``i3d_units_common.gate``):

    |got - ref64| <= gamma(n) S + 2^-24 |ref64|,   n = 9 Cout,   S = sum |g| |w| (+ |add| when a tap gradient is added)

and relative L2 <= 1e-4 per batch row.  A ReLU mask multiplies both sides by 0 or 1: the bound holds behind it.  The first-layer form
(64 -> 3, divided by ScalingLayer's scale, one more rounding) has n = 9 * 64 + 1 and S / scale.

LPIPS head.  For one position with feature vectors f0, f1 over c channels, s = |f|, n = f / (s + eps), d = n0 - n1 and the image's
value sum_p sum_c lin d^2 / P weighted by u:

    dn0 = 2 u / P * lin * d,  dn1 = -dn0,      df = dn / (s + eps) - f (f . dn) / (s (s + eps)^2)

(the second term is the derivative of 1 / (sqrt(sum f^2) + eps); at s = 0 it is dropped -- torch's sqrt backward gives NaN there, see
``head_backward_oracle``).  The kernel forms every product and both sums over c in float64 from exact fp32 inputs and rounds the result
to fp32 once, so the true error is about 2^-24 |df|.  The bound that is asserted is the formula on absolute values -- what ANY order of
the c-long sums in fp32 could lose -- times gamma(c + 8) (c terms of the dot product, and 8 for the products, the divisions, the square
root and the final rounding of the closed form):

    |got - ref64| <= gamma(c + 8) * (|dn| / (s + eps) + |f| (|f| . |dn|) / (s (s + eps)^2)),   |dn| = 2 |u| / P * lin * (|n0| + |n1|)

On top: relative L2 <= 1e-4 per image.

End to end.  The gradient of a ReLU network is discontinuous where a pre-activation crosses zero, so an oracle that chose its own
masks could differ from the GPU by a whole path at a unit whose pre-activation is at rounding level.  ``trunk_masked`` therefore takes
the masks (activation > 0) and the pool arg-max (first maximum in row-major order) from GIVEN activations -- the GPU's saved ones --
and is a smooth float64 function of the input; the test separately bounds where the given masks may differ from float64's own
(|pre-activation| <= 1e-5 x the layer's rms, at most 4 units per case).  Fed its own activations it is plain float64 autograd."""
import numpy as np
import torch
import torch.nn.functional as F

import vgg_common as vc
from vgg_common import U, TOL_L2, gamma, gate, gate_bound, randn, rel_l2_rows  # noqa: F401

EPS = 1e-10
FRAGILE_REL, FRAGILE_MAX = 1e-5, 4
SEED_W, SEED_LIN = 41, 42          # the weights of tests/golden/make_golden_vgg.py


# ---------------------------------------------------------------------------------------------------------------- conv input gradient

def dgrad_oracle(g, w, add=None, ymask=None, scale=None, mutate=None, other=None):
    """Input gradient of conv2d(., w, padding=1) for the output gradient g [N, Cout, H, W] in float64 -> (ref [N, Cin, H, W], S, n).
    ``add``: a tensor added to the sum; ``ymask``: the result is kept where ymask > 0; ``scale`` [Cin]: divided by it (the first-layer
    form).  ``mutate`` names one deliberate error; ``other``: the wrong activation of "mask_wrong_activation"."""
    g, w = g.double(), torch.as_tensor(w).double()
    wt = w.transpose(0, 1).flip(2, 3)
    wm = wt
    if mutate == "taps_not_flipped":
        wm = w.transpose(0, 1)
    if mutate == "kernel_not_transposed":      # [cout][cin] read as [cin][cout] (needs cin = cout)
        wm = w.flip(2, 3)
    acc = F.conv2d(g, wm, padding=1)
    if mutate == "drop_border_tap":            # tap (0, 0) of every window in the last output column
        w1 = torch.zeros_like(wt)
        w1[:, :, 0, 0] = wt[:, :, 0, 0]
        acc[..., -1] -= F.conv2d(g, w1, padding=1)[..., -1]
    S = F.conv2d(g.abs(), wt.abs(), padding=1)
    n = 9 * w.shape[0]
    if add is not None:
        acc, S = acc + add.double(), S + add.double().abs()
    if ymask is not None:
        m = ((other if mutate == "mask_wrong_activation" else ymask) > 0).double()
        acc = acc * m
    if scale is not None:
        sc = torch.tensor(scale, dtype=torch.float32).double().view(1, -1, 1, 1)
        acc, S, n = acc / sc, S / sc, n + 1
    return acc, S, n


DGRAD_MUTATIONS = ("taps_not_flipped", "kernel_not_transposed", "mask_wrong_activation", "drop_border_tap")
DGRAD_SHAPES = ((5, 7), (8, 16), (9, 17), (17, 33))   # below one tile, one tile, one past it in both, 3 x 3 tiles ragged
DGRAD_BATCH = (1, 3)
DGRAD_CIN = (64, 128)            # one and two 64-wide output tiles of the backward kernel
DGRAD_COUT = (16, 48, 64)        # one chunk, an odd chunk count, four chunks


def dgrad_cases():
    cases, seed = [], 17000
    for cin in DGRAD_CIN:
        for cout in DGRAD_COUT:
            for hw in DGRAD_SHAPES:
                for b in DGRAD_BATCH:
                    for mask in (0, 1):
                        for add in (0, 1):
                            seed += 1
                            cases.append({"id": f"c{cin}-{cout}-{hw[0]}x{hw[1]}-b{b}-m{mask}a{add}", "cin": cin, "cout": cout, "hw": hw, "batch": b,
                                          "mask": mask, "add": add, "seed": seed})
    return cases


def first_cases():
    return [{"id": f"first-{hw[0]}x{hw[1]}-b{b}-{'frames' if fr else 'cl'}", "cin": 3, "cout": 64, "hw": hw, "batch": b, "frames": fr,
             "mask": 0, "add": 0, "seed": 17900 + 10 * i + 2 * b + fr}
            for i, hw in enumerate(DGRAD_SHAPES) for b in DGRAD_BATCH for fr in (0, 1)]


def dgrad_inputs(case):
    """(g [N, cout, H, W], w [cout, cin, 3, 3], add or None, y or None, a second activation for the wrong-mask mutation), fp32."""
    cin, cout, (h, w), b = case["cin"], case["cout"], case["hw"], case["batch"]
    rng = np.random.default_rng(case["seed"] + 100000)
    wt = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
    g = randn(case["seed"], (b, cout, h, w))
    add = randn(case["seed"] + 200000, (b, cin, h, w)) if case["add"] else None
    y = torch.relu(randn(case["seed"] + 300000, (b, cin, h, w))) if case["mask"] else None
    other = torch.relu(randn(case["seed"] + 400000, (b, cin, h, w)))
    return g, wt, add, y, other


# ---------------------------------------------------------------------------------------------------------------- pool backward

POOL_SHAPES = [(n, c, h, w) for (h, w) in ((6, 10), (7, 9), (5, 4), (2, 3), (17, 33)) for n, c in ((2, 4), (1, 64), (1, 512))]


def pool_backward_torch(y, g):
    """torch's own MaxPool2d(2, 2) backward in fp32 (CPU): the gradient goes to the first maximum in row-major order."""
    y = y.clone().requires_grad_(True)
    F.max_pool2d(y, 2, 2).backward(g)
    return y.grad


def pool_input(kind, shape, seed):
    """Pool inputs [N, C, H, W]: "rnd", "neg" (all negative), "ties" (every window all-equal), "ties12" (equal maxima at positions 1, 2)."""
    n, c, h, w = shape
    if kind in ("rnd", "neg"):
        return randn(seed, shape, kind == "neg")
    base = randn(seed, (n, c, (h + 1) // 2, (w + 1) // 2))
    y = base.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :h, :w].clone()       # all four equal
    if kind == "ties12":                                                                # (0, 1) = (1, 0) = max, the other two below it
        y[:, :, 0::2, 0::2] -= 1.0
        y[:, :, 1::2, 1::2] -= 0.5
    return y.contiguous()


# ---------------------------------------------------------------------------------------------------------------- LPIPS head backward

def head_backward_oracle(f0, f1, lin, u, eps=EPS):
    """Closed form of the head's backward on taps [N, C, H, W] in float64, u [N]: (df0, df1, B0, B1) with B the formula on absolute
    values (the module docstring).  s = 0: the second term is dropped (finite; autograd gives NaN there)."""
    f0, f1, lin, u = f0.double(), f1.double(), lin.double().view(1, -1, 1, 1), u.double().view(-1, 1, 1, 1)
    P = f0.shape[2] * f0.shape[3]
    s0, s1 = torch.sqrt((f0 ** 2).sum(1, keepdim=True)), torch.sqrt((f1 ** 2).sum(1, keepdim=True))
    n0, n1 = f0 / (s0 + eps), f1 / (s1 + eps)
    dn = 2 * u / P * lin * (n0 - n1)
    dn_abs = 2 * u.abs() / P * lin.abs() * (n0.abs() + n1.abs())

    def side(f, s, d, d_abs):
        second = torch.where(s > 0, (f * d).sum(1, keepdim=True) / (s * (s + eps) ** 2).clamp_min(1e-300), torch.zeros_like(s))
        second_abs = torch.where(s > 0, (f.abs() * d_abs).sum(1, keepdim=True) / (s * (s + eps) ** 2).clamp_min(1e-300), torch.zeros_like(s))
        return d / (s + eps) - f * second, d_abs / (s + eps) + f.abs() * second_abs
    df0, B0 = side(f0, s0, dn, dn_abs)
    df1, B1 = side(f1, s1, -dn, dn_abs)
    return df0, df1, B0, B1


def head_backward_autograd(f0, f1, lin, u):
    """The same through autograd of ``vgg_common.lpips_layer_oracle`` (NaN at an all-zero feature vector)."""
    a, b = f0.double().clone().requires_grad_(True), f1.double().clone().requires_grad_(True)
    (vc.lpips_layer_oracle(a, b, lin) * u.double()).sum().backward()
    return a.grad, b.grad


def head_gate(got, ref, B, c):
    return gate_bound(got, ref, gamma(c + 8) * B + U * ref.abs())


HEAD_CASES = [{"id": f"c{c}-p{p[0] * p[1]}-n{n}", "c": c, "hw": p, "n": n, "seed": 18000 + c + 7 * p[0] * p[1] + n}
              for c in (64, 128, 256, 512) for p in ((1, 1), (3, 5), (16, 16)) for n in (1, 3)]


def head_inputs(case):
    """(f0, f1 [N, C, H, W] post-ReLU fp32 with ONE all-zero feature vector in f0 when there is more than one position, lin, u)."""
    c, (h, w), n = case["c"], case["hw"], case["n"]
    f0, f1 = torch.relu(randn(case["seed"], (n, c, h, w))), torch.relu(randn(case["seed"] + 50000, (n, c, h, w)))
    if h * w > 1:
        f0[0, :, 0, 1] = 0
    lin = torch.from_numpy(vc.lin_state_dict(9)[f"lin{vc.CHNS.index(c)}.model.1.weight"]).flatten()
    u = torch.tensor([0.7 + 0.9 * i * (-1) ** i for i in range(n)], dtype=torch.float64)     # non-uniform, one negative
    return f0, f1, lin, u


# ---------------------------------------------------------------------------------------------------------------- trunk, masks given

def windows(t):
    """[N, C, H, W] -> [N, C, H // 2, W // 2, 4]: the 2 x 2 windows of MaxPool2d(2, 2) in floor mode, row-major inside a window."""
    n, c, h, w = t.shape
    ho, wo = h // 2, w // 2
    return t[:, :, :2 * ho, :2 * wo].reshape(n, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, ho, wo, 4)


def trunk_masked(sd, x, acts=None):
    """The trunk of ``vgg_common.trunk_oracle`` on x [N, 3, H, W] (normalised, float64, may require grad) -> (taps, pre-activations,
    activations).  ``acts``: thirteen given post-ReLU activations [N, C, H', W'] whose masks (> 0) and pool arg-max (first maximum in
    row-major order) replace the oracle's own; None: relu and max_pool2d themselves."""
    h, taps, pres, own = x, [], [], []
    for l, (idx, _, _) in enumerate(vc.CONVS):
        pre = F.conv2d(h, torch.from_numpy(sd[f"features.{idx}.weight"]).double(), torch.from_numpy(sd[f"features.{idx}.bias"]).double(), padding=1)
        pres.append(pre)
        h = torch.relu(pre) if acts is None else pre * (acts[l] > 0).double()
        own.append(h)
        if idx in vc.TAP_AFTER:
            taps.append(h)
        if idx in vc.POOL_AFTER:
            if acts is None:
                h = F.max_pool2d(h, 2, 2)
            else:
                arg = windows(acts[l]).argmax(-1, keepdim=True)       # the FIRST maximal value (torch.argmax's rule)
                h = windows(h).gather(-1, arg)[..., 0]
    return taps, pres, own


def lpips_masked(sd, lin, x0, x1, acts0=None, acts1=None):
    """LPIPS per image [N] in float64 of frames x0, x1 (which may require grad), the trunk through ``trunk_masked``."""
    c = lambda v: torch.tensor(v, dtype=torch.float32).double().view(1, 3, 1, 1)  # noqa: E731
    t0 = trunk_masked(sd, (x0 - c(vc.LPIPS_SHIFT)) / c(vc.LPIPS_SCALE), acts0)
    t1 = trunk_masked(sd, (x1 - c(vc.LPIPS_SHIFT)) / c(vc.LPIPS_SCALE), acts1)
    val = sum(vc.lpips_layer_oracle(a, b, torch.from_numpy(lin[f"lin{k}.model.1.weight"]).flatten()) for k, (a, b) in enumerate(zip(t0[0], t1[0])))
    return val, t0, t1


def fragile_units(pres, acts):
    """Where given masks differ from float64's own: (number of differing units, the worst |pre-activation| / layer rms among them)."""
    count, worst = 0, 0.0
    for pre, a in zip(pres, acts):
        diff = (pre.detach() > 0) != (a > 0)
        k = int(diff.sum())
        if k:
            count += k
            worst = max(worst, float(pre.detach().abs()[diff].max() / pre.detach().pow(2).mean().sqrt()))
    return count, worst


def fp32_activations(sd, x):
    """The thirteen post-ReLU activations of plain fp32 torch on the CPU (x normalised)."""
    h, acts = x.float(), []
    for idx, _, _ in vc.CONVS:
        h = torch.relu(F.conv2d(h, torch.from_numpy(sd[f"features.{idx}.weight"]), torch.from_numpy(sd[f"features.{idx}.bias"]), padding=1))
        acts.append(h)
        if idx in vc.POOL_AFTER:
            h = F.max_pool2d(h, 2, 2)
    return acts


E2E_SIZES = ((16, 16), (32, 32), (24, 40), (20, 36))      # the last two floor odd maps (24 x 40 -> 3 x 5 -> 1 x 2; 20 x 36 -> 5 x 9 -> 2 x 4 -> 1 x 2)
E2E_BATCH = (2, 3)
E2E_WHICH = ("target", "input", "both")


def e2e_cases():
    # seeds at which plain fp32 torch and float64 agree on every ReLU mask of all thirteen layers (test_host_lpips_grad checks it): about
    # one input in ten has a unit whose pre-activation is at rounding level (bases 19000 and 19100 each had one), and there the
    # gradient is not defined to better than one path
    return [{"id": f"{h}x{w}-n{n}-{which}", "hw": (h, w), "n": n, "which": which, "seed": 19200 + 10 * i + n}
            for i, (h, w) in enumerate(E2E_SIZES) for n in E2E_BATCH for which in E2E_WHICH]


def e2e_frames(case):
    """(x0, x1 [N, 3, H, W] fp32 in [-1, 1]: x1 a perturbed copy of x0, as a generated frame is of its real one; weights [N] of the outputs)."""
    (h, w), n = case["hw"], case["n"]
    a = torch.from_numpy(vc.clips(case["seed"], n, 1, h, w))[:, 0].contiguous()
    b = (0.7 * a + 0.3 * torch.from_numpy(vc.clips(case["seed"] + 1, n, 1, h, w))[:, 0]).contiguous()
    return a, b, e2e_weights(n)


def e2e_weights(n):
    return torch.tensor([1.0 + 0.5 * i for i in range(n)], dtype=torch.float64)


def lpips_frames(x):
    c = lambda v: torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1)  # noqa: E731
    return (x - c(vc.LPIPS_SHIFT)) / c(vc.LPIPS_SCALE)


def to_nchw(t):
    """channels-last [N, H, W, C] (device or host) -> host [N, C, H, W]."""
    return t.detach().cpu().permute(0, 3, 1, 2)


# the committed fixture tests/golden/vgg_lpips_grad.npz (make_golden_lpips_grad.py): 2 pairs per size, seeds as below
GOLDEN = {"32x32": {"h": 32, "w": 32, "seed": 161}, "24x40": {"h": 24, "w": 40, "seed": 163}}
GOLDEN_N = 2


def golden_frames(tag):
    g = GOLDEN[tag]
    a = torch.from_numpy(vc.clips(g["seed"], GOLDEN_N, 1, g["h"], g["w"]))[:, 0].contiguous()
    b = (0.7 * a + 0.3 * torch.from_numpy(vc.clips(g["seed"] + 1, GOLDEN_N, 1, g["h"], g["w"]))[:, 0]).contiguous()
    return a, b, e2e_weights(GOLDEN_N)
