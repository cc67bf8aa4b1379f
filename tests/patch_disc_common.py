"""Shared by tests/test_host_patch_disc.py, tests/test_gpu_patch_disc.py and tests/golden/make_golden_patch_disc.py: a float64 restatement
of the patch discriminator (reference stage1_VAE/modules/patch_disc.py) in functional torch on the CPU -- forward with spectral norm in
training mode and ActNorm's data init, and a BACKWARD WRITTEN OUT BY HAND (not autograd), so that the LeakyReLU masks can be given and
single deliberate errors can be switched on -- plus the unit oracles with their bounds, the case lists and the inputs of the fixture.
Nothing of the package is imported.

The gate is the project's (``i3d_units_common.gate``): |got - ref64| <= gamma(n) S + 2^-24 |ref64| element-wise, with n the length of the
summation chain and S the same sum over absolute products, and relative L2 <= 1e-4 per batch row.
  conv forward   n = 16 Cin (+2 for the bias and ActNorm's add, +1 for its scale), S = conv(|x|, |w|) + |b|
  dgrad          n = 4 Cout at stride 2 (the taps of the pixel's parity), 16 Cout at stride 1; the mask and the scale multiply the
                 operand before the sum: one rounding each on the products, +2
  wgrad          n = positions (+2 as above); the kernel adds quarter-slices, then slices: any order of n terms has error <= gamma(n) S
  projection     dW = (dWn - p u v^T) / sigma with p = <dWn, Wn>: the bound of dWn, plus gamma(4) |p u v^T| for the float64 dot product
                 rounded once and the two products, all divided by sigma, plus one more rounding for the division
Spectral norm: W viewed as [Cout, Cin 16]; v <- normalize(W^T u), u <- normalize(W v) with eps 1e-12, sigma = u . (W v), the conv uses
W / sigma; dW_orig = (dWn - <dWn, Wn> u v^T) / sigma with the u, v AFTER the iteration (they are constants of the forward)."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from i3d_units_common import U, TOL_L2, gamma, gate, gate_bound, randn, rel_l2_rows  # noqa: F401  (the gate is reused by import)

FRAGILE_REL, FRAGILE_MAX = 1e-5, 4
SEED_MODULE, SEED_DATA = 4100, 4101
FIXTURE_CFG = {"in_channels": 3, "ndf": 16, "n_layers": 3, "use_actnorm": True, "spectral_norm": True}
EVAL_SHAPES = {"e24x40": (3, 24, 40, 4110), "e32": (2, 32, 32, 4111)}
SGD_LR, SGD_STEPS = 1e-3, 6
ISSUE_LOSSES = (0.885574, 0.661411, 0.547179, 0.467544, 0.401750, 0.344783)   # the reference in float64, as the issue records them
MUTATIONS = ("dgrad_not_flipped", "dgrad_wrong_parity", "projection_dropped", "u_before_iteration", "biased_std", "mask_wrong_side_of_scale")


def spec(ndf, n_layers):
    """The convs of NLayerDiscriminator.main: index in the Sequential, channels, stride, index of the ActNorm behind it (or None)."""
    layers, mult = [dict(key=0, cin=3, cout=ndf, stride=2, norm=None, last=False)], 1
    for n in range(1, n_layers + 1):
        prev, mult = mult, min(2 ** n, 8)
        k = 2 + 3 * (n - 1)
        layers.append(dict(key=k, cin=ndf * prev, cout=ndf * mult, stride=2 if n < n_layers else 1, norm=k + 1, last=False))
    layers.append(dict(key=2 + 3 * n_layers, cin=ndf * mult, cout=1, stride=1, norm=None, last=True))
    return layers


def state_keys(ndf=64, n_layers=3):
    """{key: (shape, dtype)} of NLayerDiscriminator(config).state_dict() with spectral norm and ActNorm."""
    out = {}
    for l in spec(ndf, n_layers):
        m = f"main.{l['key']}."
        out[m + "bias"] = ((l["cout"],), torch.float32)
        out[m + "weight_orig"] = ((l["cout"], l["cin"], 4, 4), torch.float32)
        out[m + "weight_u"] = ((l["cout"],), torch.float32)
        out[m + "weight_v"] = ((l["cin"] * 16,), torch.float32)
        if l["norm"] is not None:
            a = f"main.{l['norm']}."
            out[a + "loc"] = ((1, l["cout"], 1, 1), torch.float32)
            out[a + "scale"] = ((1, l["cout"], 1, 1), torch.float32)
            out[a + "initialized"] = ((), torch.uint8)
    return out


def train_inputs():
    """(fake, real) [4, 3, 32, 32] fp32 of the fixture's training step and of the loss sequence: drawn in float64 (the draw that gives
    the issue's loss sequence) and rounded to fp32 once, so that the reference and the GPU see the same numbers."""
    g = torch.Generator().manual_seed(SEED_DATA)
    real = torch.randn(4, 3, 32, 32, generator=g, dtype=torch.float64)
    fake = 0.5 * torch.randn(4, 3, 32, 32, generator=g, dtype=torch.float64) + 0.3
    return fake.float(), real.float()


def eval_inputs(tag):
    n, h, w, seed = EVAL_SHAPES[tag]
    return randn(seed, (n, 3, h, w))


def slope(mask):
    """LeakyReLU(0.2)'s derivative for a boolean mask, in float64 (torch.where on two Python scalars would give fp32)."""
    one = torch.ones((), dtype=torch.float64)
    return torch.where(mask, one, 0.2 * one)


def hinge_disc(fake, real):
    return (torch.relu(1.0 - real).mean() + torch.relu(1.0 + fake).mean()) / 2


def hinge_disc_grads(fake, real):
    """d loss / d fake, d loss / d real of the 'disc' hinge (relu'(0) = 0, torch's rule)."""
    n = fake.numel()
    return (1.0 + fake > 0).to(fake.dtype) / (2 * n), -(1.0 - real > 0).to(real.dtype) / (2 * n)


# ---------------------------------------------------------------------------------------------------------------- the network in float64

def power_iteration(W2, u, v, iterate=True, eps=1e-12):
    """-> (u', v', sigma) of torch.nn.utils.spectral_norm's forward (one iteration in training mode, none in eval mode)."""
    if iterate:
        v = F.normalize(W2.t() @ u, dim=0, eps=eps)
        u = F.normalize(W2 @ v, dim=0, eps=eps)
    return u, v, torch.dot(u, W2 @ v)


def actnorm_init(y, biased=False):
    """loc, scale [C] from the conv output y [N, C, H, W] (patch_disc.py:28-47)."""
    flat = y.permute(1, 0, 2, 3).reshape(y.shape[1], -1)
    return -flat.mean(1), 1.0 / (flat.std(1, unbiased=not biased) + 1e-6)


def forward_oracle(sd, x, layers, training, init=False, masks=None, mutate=None):
    """sd: {state_dict key: tensor}; x [N, 3, H, W].  -> (pred [N, 1, Ho, Wo] float64, cache).  ``masks``: per conv but the last the
    LeakyReLU mask [N, C, H, W] (bool) to use instead of the float64 one.  cache["state"] holds the updated u, v, loc, scale."""
    x = x.double()
    state, steps = {}, []
    for i, l in enumerate(layers):
        m = f"main.{l['key']}."
        b = sd[m + "bias"].double()
        if m + "weight" in sd:               # spectral_norm: False -- the same net with sigma = 1 and no u, v
            W = sd[m + "weight"].double()
            u0 = u = v = None
            sigma = torch.ones((), dtype=torch.float64)
        else:
            W = sd[m + "weight_orig"].double()
            u0, v0 = sd[m + "weight_u"].double(), sd[m + "weight_v"].double()
            u, v, sigma = power_iteration(W.reshape(W.shape[0], -1), u0, v0, iterate=training)
            state[m + "weight_u"], state[m + "weight_v"] = u, v
        Wn = W / sigma
        y = F.conv2d(x, Wn, b, stride=l["stride"], padding=1)
        st = dict(x=x, W=W, Wn=Wn, u=u, v=v, u0=u0, sigma=sigma, y=y, layer=l)
        h = y
        if l["norm"] is not None:
            a = f"main.{l['norm']}."
            loc, scale = sd[a + "loc"].double().reshape(-1), sd[a + "scale"].double().reshape(-1)
            if init:
                loc, scale = actnorm_init(y, biased=mutate == "biased_std")
            state[a + "loc"], state[a + "scale"] = loc.reshape(1, -1, 1, 1), scale.reshape(1, -1, 1, 1)
            st["loc"], st["scale"] = loc, scale
            h = scale.view(1, -1, 1, 1) * (y + loc.view(1, -1, 1, 1))
        st["h"] = h
        if not l["last"]:
            mask = h > 0 if masks is None else masks[i]
            st["mask"] = mask
            h = torch.where(mask, h, 0.2 * h)
        st["a"] = h
        steps.append(st)
        x = h
    return x, dict(steps=steps, state=state)


def dgrad_taps(dy, Wn, in_hw, stride, mutate=None):
    """Input gradient of conv2d(., Wn, stride, padding=1) tap by tap: dx[n, :, ho s - 1 + kh, wo s - 1 + kw] += dy[n, :, ho, wo] . Wn[:, :, kh, kw].
    Equal to torch.nn.grad.conv2d_input (checked by the host test); ``mutate`` switches one deliberate error on."""
    N, Co, Ho, Wo = dy.shape
    Hi, Wi = in_hw
    pad = torch.zeros(N, Wn.shape[1], Hi + 4, Wi + 4, dtype=dy.dtype)
    for kh in range(4):
        for kw in range(4):
            wh, ww = kh, kw
            if mutate == "dgrad_not_flipped":
                wh, ww = 3 - kh, 3 - kw
            if mutate == "dgrad_wrong_parity" and stride == 2:
                wh, ww = kh ^ 1, kw ^ 1
            c = torch.einsum("nohw,oi->nihw", dy, Wn[:, :, wh, ww])
            pad[:, :, kh + 1: kh + 1 + stride * Ho: stride, kw + 1: kw + 1 + stride * Wo: stride] += c
    return pad[:, :, 2: 2 + Hi, 2: 2 + Wi]


def backward_oracle(cache, d_pred, mutate=None):
    """-> ({state_dict key: gradient}, dx [N, 3, H, W]) for the upstream gradient d_pred, by hand."""
    g, grads = d_pred.double(), {}
    for st in reversed(cache["steps"]):
        l = st["layer"]
        m = f"main.{l['key']}."
        dh = g
        if not l["last"]:
            mask = st["mask"]
            if mutate == "mask_wrong_side_of_scale" and l["norm"] is not None:
                mask = (st["y"] + st["loc"].view(1, -1, 1, 1)) > 0
            dh = g * slope(mask)
        dy = dh
        if l["norm"] is not None:
            a = f"main.{l['norm']}."
            grads[a + "scale"] = (dh * (st["y"] + st["loc"].view(1, -1, 1, 1))).sum((0, 2, 3)).reshape(1, -1, 1, 1)
            grads[a + "loc"] = (dh * st["scale"].view(1, -1, 1, 1)).sum((0, 2, 3)).reshape(1, -1, 1, 1)
            dy = dh * st["scale"].view(1, -1, 1, 1)
        grads[m + "bias"] = dy.sum((0, 2, 3))
        dWn = conv2d_weight(st["x"], st["W"].shape, dy, stride=l["stride"], padding=1)
        if st["u"] is None:
            grads[m + "weight"] = dWn
        else:
            u = st["u0"] if mutate == "u_before_iteration" else st["u"]
            proj = 0.0 if mutate == "projection_dropped" else (dWn * st["Wn"]).sum() * torch.outer(u, st["v"]).view_as(dWn)
            grads[m + "weight_orig"] = (dWn - proj) / st["sigma"]
        g = dgrad_taps(dy, st["Wn"], st["x"].shape[2:], l["stride"], mutate)
    return grads, g


# ---------------------------------------------------------------------------------------------------------------- unit oracles

def cl(x):
    """[N, C, H, W] -> channels-last [N, H, W, C] fp32 (3 channels: a zero fourth is appended)."""
    x = x.float().permute(0, 2, 3, 1)
    if x.shape[-1] == 3:
        x = torch.cat([x, torch.zeros_like(x[..., :1])], dim=-1)
    return x.contiguous()


def uncl(y):
    """channels-last [N, H, W, C] -> [N, C, H, W]"""
    return y.permute(0, 3, 1, 2)


def conv_inputs(case):
    cin, cout, (h, w), b = case["cin"], case["cout"], case["hw"], case["batch"]
    x = randn(case["seed"], (b, cin, h, w))
    wt = randn(case["seed"] + 1, (cout, cin, 4, 4)) * float(np.sqrt(1.0 / (16 * cin)))
    bias, loc = 0.1 * randn(case["seed"] + 2, (cout,)), 0.2 * randn(case["seed"] + 3, (cout,))
    scale = 1.0 + 0.3 * randn(case["seed"] + 4, (cout,))
    scale[0] = -scale[0].abs()          # one negative scale
    return x, wt, bias, loc, scale


def conv_oracle(x, w, bias, loc, scale, stride, lrelu):
    """-> (out, pre, S, n) in float64"""
    x, w, bias = x.double(), w.double(), bias.double()
    pre = F.conv2d(x, w, bias, stride=stride, padding=1)
    S = F.conv2d(x.abs(), w.abs(), bias.abs(), stride=stride, padding=1)
    n, out = 16 * x.shape[1] + 1, pre
    if loc is not None:
        lc, sc = loc.double().view(1, -1, 1, 1), scale.double().view(1, -1, 1, 1)
        out, S, n = sc * (pre + lc), sc.abs() * (S + lc.abs()), n + 2
    if lrelu:
        out = torch.where(out > 0, out, 0.2 * out)
        n += 1
    return out, pre, S, n


CONV_STRIDE2 = ((9, 13), (8, 8), (33, 17))
CONV_STRIDE1 = ((4, 4), (6, 7), (8, 8))
CONV_CH = ((3, 16), (3, 48), (16, 16), (16, 128), (64, 48), (64, 128))
EPILOGUES = ("bias", "bias_lrelu", "actnorm_lrelu")


def conv_cases():
    cases, seed = [], 41000
    for cin, cout in CONV_CH:
        for stride, shapes in ((2, CONV_STRIDE2), (1, CONV_STRIDE1)):
            for hw in shapes:
                for b in (1, 3):
                    seed += 10
                    cases.append({"id": f"c{cin}-{cout}-s{stride}-{hw[0]}x{hw[1]}-b{b}", "cin": cin, "cout": cout, "stride": stride, "hw": hw, "batch": b,
                                  "seed": seed, "epilogue": EPILOGUES[(seed // 10) % 3]})
    return cases


def big_cases():
    """Shapes past the threshold at which the two GEMM kernels take their 128-row tile (at least 512 row tiles of 128 per column tile:
    65 536 positions with one column tile), one per column-tile width that the module tests do not reach: 16 and 32 columns.  The 64-column
    forms and the frames form run in the 128 x 128 module test."""
    return [
        {"id": "big-conv-c3-16", "kind": "conv", "cin": 3, "cout": 16, "stride": 2, "hw": (512, 512), "batch": 1, "seed": 47010, "epilogue": "bias_lrelu"},
        {"id": "big-conv-c3-32", "kind": "conv", "cin": 3, "cout": 32, "stride": 2, "hw": (512, 512), "batch": 1, "seed": 47020, "epilogue": "actnorm_lrelu"},
        {"id": "big-conv-c16-16-s1", "kind": "conv", "cin": 16, "cout": 16, "stride": 1, "hw": (257, 257), "batch": 1, "seed": 47030, "epilogue": "bias"},
        {"id": "big-dgrad-c16-s2", "kind": "dgrad", "cin": 16, "cout": 16, "stride": 2, "hw": (256, 257), "batch": 1, "seed": 47040},
        {"id": "big-dgrad-c32-s2", "kind": "dgrad", "cin": 32, "cout": 16, "stride": 2, "hw": (257, 256), "batch": 1, "seed": 47050},
        {"id": "big-dgrad-c16-s1", "kind": "dgrad", "cin": 16, "cout": 16, "stride": 1, "hw": (256, 257), "batch": 1, "seed": 47060},
        {"id": "big-dgrad-c32-s1", "kind": "dgrad", "cin": 32, "cout": 32, "stride": 1, "hw": (257, 256), "batch": 1, "seed": 47070},
    ]


def rows_per_workgroup(rows, column_tiles):
    """The tile choice of the two GEMM kernels (csrc/i2v_train_conv.h, rows_of), restated so that the tests can say which they ran."""
    return 128 if (rows + 127) // 128 * column_tiles >= 512 else 64


def dgrad_inputs(case):
    """(g [N, Cout, Ho, Wo], w, act (the layer's activation, for the mask) , scale) for the conv of ``case`` seen from its output."""
    cin, cout, (h, w), b, s = case["cin"], case["cout"], case["hw"], case["batch"], case["stride"]
    ho, wo = (h - 2) // s + 1, (w - 2) // s + 1
    g = randn(case["seed"] + 5, (b, cout, ho, wo))
    wt = randn(case["seed"] + 1, (cout, cin, 4, 4)) * float(np.sqrt(1.0 / (16 * cin)))
    act = randn(case["seed"] + 6, (b, cout, ho, wo))
    scale = 1.0 + 0.3 * randn(case["seed"] + 4, (cout,))
    scale[0] = -scale[0].abs()
    return g, wt, act, scale


def masked(g, act, scale):
    """The gradient at the conv output from the one at the activation, in float64, and its absolute value"""
    dy = g.double()
    if act is not None:
        dy = dy * slope(act > 0)
    if scale is not None:
        dy = dy * scale.double().view(1, -1, 1, 1)
    return dy


def dgrad_oracle(g, w, act, scale, in_hw, stride, mutate=None):
    """-> (ref [N, Cin, H, W], S, n)"""
    dy, w = masked(g, act, scale), w.double()
    ref = dgrad_taps(dy, w, in_hw, stride, mutate)
    S = conv2d_input((g.shape[0], w.shape[1]) + tuple(in_hw), w.abs(), dy.abs(), stride=stride, padding=1)
    return ref, S, (4 if stride == 2 else 16) * w.shape[0] + 2


def wgrad_oracle(g, x, w, act, scale, stride, u=None, v=None, sigma=None, mutate=None):
    """-> (dweight, dbias, bound of dweight, bound of dbias) in float64.  With u, v, sigma: w is weight_orig and the conv ran on w / sigma."""
    dy, x, w = masked(g, act, scale), x.double(), w.double()
    n = dy.shape[0] * dy.shape[2] * dy.shape[3] + 2
    dWn = conv2d_weight(x, w.shape, dy, stride=stride, padding=1)
    S = conv2d_weight(x.abs(), w.shape, dy.abs(), stride=stride, padding=1)
    db, Sb = dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
    bound = gamma(n) * S
    if sigma is not None:
        sg, Wn = float(sigma), w / float(sigma)
        p = (dWn * Wn).sum() * torch.outer(u.double(), v.double()).view_as(dWn)
        pa = (S * Wn.abs()).sum() * torch.outer(u.double().abs(), v.double().abs()).view_as(dWn)
        if mutate == "projection_dropped":
            p = p * 0
        dWn = (dWn - p) / sg
        bound = (bound + gamma(n + 4) * pa + gamma(4) * p.abs()) / sg + U * dWn.abs()
    return dWn, db, bound + U * dWn.abs(), gamma(n) * Sb + U * db.abs()


def wgrad_cases():
    """Position counts that the slice plan turns into one slice, exactly several and a ragged last one (asserted by the GPU test)."""
    return [
        {"id": "one-slice", "cin": 64, "cout": 128, "stride": 1, "hw": (4, 4), "batch": 1, "seed": 42010, "project": 1},        # 9 positions
        {"id": "even-slices", "cin": 16, "cout": 16, "stride": 2, "hw": (16, 16), "batch": 2, "seed": 42020, "project": 0},     # 128 = 2 x 64
        {"id": "ragged", "cin": 16, "cout": 48, "stride": 2, "hw": (9, 13), "batch": 3, "seed": 42030, "project": 1},           # 72 = 64 + 8
        {"id": "image", "cin": 3, "cout": 16, "stride": 2, "hw": (33, 17), "batch": 1, "seed": 42040, "project": 1},            # 128
        {"id": "wide", "cin": 64, "cout": 48, "stride": 1, "hw": (8, 8), "batch": 3, "seed": 42050, "project": 0},              # 147
    ]


HEAD_CASES = [{"id": f"head-c{c}-{h}x{h}-b{b}", "cin": c, "hw": (h, h), "batch": b, "seed": 43000 + c + 10 * h + b}
              for c in (128, 512) for h in (4, 7) for b in (1, 2)]
POWER_SHAPES = ((16, 48), (128, 1024), (512, 4096), (1, 8192))


def fragile_units(given_mask, h64):
    """Units whose given mask differs from float64's own, and how many of them lie outside |h| <= 1e-5 rms(h)."""
    diff = given_mask != (h64 > 0)
    rms = float(h64.pow(2).mean().sqrt())
    return int(diff.sum()), int((diff & (h64.abs() > FRAGILE_REL * rms)).sum())
