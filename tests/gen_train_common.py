"""Shared by tests/test_host_gen_train.py, tests/test_gpu_gen_train.py, tests/test_gpu_gen_train_hygiene.py and
tests/golden/make_golden_gen_train.py: the module cases, seeded parameters and inputs, a float64 restatement of the Generator chain
(decoder.py:55-120) on ``gblock_train_common.block`` with hand-written backwards of ``fc``, the up-samplings and the image head, float64
oracles of the new units with the deliberate errors the gates must catch, and the gates.

Gates.  The module, per tensor: relative L2 <= TOL_L2 = 1e-4, the project's gate, provided the reference's own fp32 run stays a factor four
inside it against its float64 run.  The frames do (about 1e-6).  Most gradients inherently cannot: a case has 0.4 to 6 million LeakyReLU
inputs per layer, an fp32 forward moves each by about 1e-6 of its scale, so in every large layer about one input changes its sign against
float64; its slope flips between 1 and 0.2, which is 0.8 / sqrt(N) = 6e-4 of that layer's gradient, and every gradient upstream inherits
it.  No seed avoids this (five were tried: 3e-4 to 3e-3), and an exact-fp32 implementation draws its own flips.  Such a tensor's gate is
four times the reference's fp32 distance: make_golden_gen_train.py measures the distance per compared tensor, the fixtures record it
(``<case>.d32.<tensor>``, case c included) and gate_of() applies the rule; REF_FP32 holds the worst figure per case.  The per-block
``conv_0.bias`` gradients are zero by construction (ADAIN's instance norm removes a constant): they are held on the scale of what cancels,
as gblock_train_common.ZERO_GRADS.  The units, element-wise, |got - ref64| <= gamma(n) S + u |ref64| with S the same sum over absolute
values:
  fc forward, dW, db      float64 sums rounded once: n = 1
  fc dz                   float64 partials per slice added in slice order: n = the slice count
  up-sampling forward     bit-exact
  up-sampling backward    n = ut us us - 1 on the box sum of |g|
  head y, dx, dW          n = 27 nf + 4 on the sum of absolute products; db: n = 1 on sum |gy| (gy = g (1 - y y) in fp32, as torch forms it)"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

import gblock_train_common as gc
from i3d_units_common import U, gamma, gate  # noqa: F401

TOL_L2 = 1e-4
SGD_STEPS = 4
SGD_LR = 2e-5          # measured when the fixtures were made (make_golden_gen_train.py --check prints the fp32 / float64 distance per step)
IMG_SCALE = 0.35       # conv_img.weight ~ N(0, IMG_SCALE^2 / fan_in): keeps the 99th percentile of |pre-tanh| below 2 (--check prints it)
N_DIRECTIONS = 4
# the worst relative L2 distance of the reference's own fp32 run from its float64 run over the compared tensors (--check, these seeds)
REF_FP32 = {"a": (8.60e-4, "g_3.norm_0.conv_beta.bias"), "b": (6.33e-3, "g_4.norm_0.conv_beta.bias"), "c": (3.97e-3, "g_3.norm_0.conv.bias")}
FULL_GRADS = ("fc.bias", "conv_img.weight", "conv_img.bias")   # stored in full in the fixtures, besides every block's conv_0.bias

BLOCKS = ("head_0", "g_0", "g_1", "g_2", "g_3", "g_4")
#         nf 16, z_dim 8: the smallest maps the chain allows
CASES = {
    "a": dict(nf=16, z_dim=8, spectral=True, upsample_s=[1, 1], upsample_t=[1, 1], B=3, img=(32, 32), seed=41),
    "b": dict(nf=16, z_dim=8, spectral=True, upsample_s=[2, 1], upsample_t=[1, 2], B=1, img=(64, 64), seed=42),
    "c": dict(nf=16, z_dim=8, spectral=False, upsample_s=[1, 2], upsample_t=[2, 1], B=2, img=(64, 64), seed=43),
}
FIXTURES = ("a", "b")


def dic_of(case):
    """The reference's constructor argument."""
    return {"channel_factor": case["nf"], "z_dim": case["z_dim"], "spectral_norm": case["spectral"], "upsample_s": list(case["upsample_s"]),
            "upsample_t": list(case["upsample_t"])}


def block_cfgs(case):
    nf = case["nf"]
    chans = [(16, 16), (16, 16), (16, 8), (8, 4), (4, 2), (2, 1)]
    return {name: dict(n_in=a * nf, n_out=b * nf, spectral=case["spectral"], z_dim=case["z_dim"]) for name, (a, b) in zip(BLOCKS, chans)}


def factors(case):
    return [(2, 2), (2, 2), (2, 2)] + list(zip(case["upsample_t"], case["upsample_s"]))


def out_shape(case):
    T, H = 1, 4
    for ut, us in factors(case):
        T, H = T * ut, H * us
    return (case["B"], T, 3, H, H)


def param_shapes(case):
    """{state_dict key: shape} of Generator.state_dict() (any order)."""
    nf, z = case["nf"], case["z_dim"]
    out = {"fc.weight": (256 * nf, z), "fc.bias": (256 * nf,), "conv_img.weight": (3, nf, 3, 3, 3), "conv_img.bias": (3,)}
    for name, cfg in block_cfgs(case).items():
        out.update({f"{name}.{k}": s for k, s in gc.param_shapes(cfg).items()})
    return out


def synthetic_state(case):
    """Seeded fp32 parameters (numpy), the blocks' in the manner of gblock_train_common.synthetic_state (weights ~ N(0, 1.5^2 / fan_in),
    unit u / v, GroupNorm weights around 1, biases 0.2 N(0, 1)); fc like a weight; conv_img on IMG_SCALE."""
    rng = np.random.default_rng(case["seed"])
    sd = {}
    for k, shp in sorted(param_shapes(case).items()):
        a = rng.standard_normal(shp)
        if gc.is_buffer(k):
            a = a / np.linalg.norm(a)
        elif k.endswith("bn.weight"):
            a = 1.0 + 0.3 * a
        elif k.endswith(".bias"):
            a = 0.2 * a
        elif k == "conv_img.weight":
            a = a * (IMG_SCALE / np.sqrt(np.prod(shp[1:])))
        else:
            a = a * (1.5 / np.sqrt(np.prod(shp[1:])))
        sd[k] = a.astype(np.float32)
    return sd


def inputs(case):
    """img [B, 3, h, w], motion [B, z_dim] and the loss coefficients c of the frames' shape, fp32."""
    rng = np.random.default_rng(case["seed"] + 1000)
    img = rng.uniform(-1, 1, (case["B"], 3) + tuple(case["img"])).astype(np.float32)
    z = rng.standard_normal((case["B"], case["z_dim"])).astype(np.float32)
    c = rng.standard_normal(out_shape(case)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (img, z, c))


def direction(key, i, shape):
    """The i-th seeded unit direction of the parameter ``key`` (float64)."""
    seed = [int.from_bytes(key.encode(), "little") % (2 ** 63), i]
    d = np.random.default_rng(seed).standard_normal(shape)
    return d / np.linalg.norm(d)


def is_zero_grad(key):
    return key.endswith("." + gc.ZERO_GRADS[0])


# ---------------------------------------------------------------------------------------------------------------- unit oracles (float64)
def upsample(x, ut, us):
    return x.repeat_interleave(ut, 2).repeat_interleave(us, 3).repeat_interleave(us, 4)


def upsample_backward(g, ut, us, mean=False):
    """The adjoint of the nearest up-sampling: the box SUM (``mean``: the deliberate error)."""
    B, C, T, H, W = g.shape
    box = g.reshape(B, C, T // ut, ut, H // us, us, W // us, us)
    return box.mean((3, 5, 7)) if mean else box.sum((3, 5, 7))


def fc_ref(z, w, b, g=None):
    """-> (out, S_out) or, with g, (dw, db, dz, S_dw, S_db, S_dz)."""
    z, w, b = z.double(), w.double(), b.double()
    if g is None:
        return z @ w.t() + b, z.abs() @ w.abs().t() + b.abs()
    g = g.double()
    return g.t() @ z, g.sum(0), g @ w, g.abs().t() @ z.abs(), g.abs().sum(0), g.abs() @ w.abs()


def head_forward_ref(x, w, b):
    """x [B, nf, T, H, W] fp32 -> (y [B, T, 3, H, W], S of the pre-activation, a = lrelu(x) as fp32 forms it, pre)."""
    a = gc.lrelu(x.float()).double()
    w, b = w.double(), b.double()
    pre = F.conv3d(a, w, b, padding=1)
    S = F.conv3d(a.abs(), w.abs(), b.abs(), padding=1)
    return torch.tanh(pre).transpose(1, 2), S.transpose(1, 2), a, pre


def head_backward_ref(x, w, g, y, slope_at_zero=0.2, no_tanh_grad=False, no_flip=False):
    """g, y [B, T, 3, H, W] fp32 (y: the frames the backward starts from) -> dict(dx, dw, db and their S).  gy = g (1 - y y) in fp32, as
    torch forms it; everything behind it in float64.  The keyword arguments are the deliberate errors."""
    a32 = gc.lrelu(x.float())
    a, w = a32.double(), w.double()
    g32, y32 = g.float(), y.float()
    gy = (g32 if no_tanh_grad else g32 * (1 - y32 * y32)).double().transpose(1, 2)    # [B, 3, T, H, W]
    slope = gc.lrelu_slope(a, slope_at_zero)
    wt = w if not no_flip else w.flip((2, 3, 4))
    d_a, dw, db = gc.conv_grads(a, wt, gy, 1)
    S_a, S_w, S_b = gc.conv_grads(a.abs(), w.abs(), gy.abs(), 1)
    return dict(dx=d_a * slope, dw=dw, db=db, S_dx=S_a * slope, S_dw=S_w, S_db=S_b)


# ---------------------------------------------------------------------------------------------------------------- the module oracle
def generator(sd, img, z, case, c=None, train=True, dtype=torch.float64):
    """The Generator forward and, with the loss sum(c frames), the hand-written backward.  ``sd``: {key: tensor or array}.
    -> dict(out [B, T, 3, H, W], pre, the blocks' u / v after, and with c: dz (= dz_fc + the blocks' dz_blocks), grads, scale)."""
    t = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    img, z = img.to(dtype), z.to(dtype)
    cfgs, B = block_cfgs(case), z.shape[0]
    sub = {name: {k[len(name) + 1:]: v for k, v in t.items() if k.startswith(name + ".")} for name in BLOCKS}
    steps = [(1, 1)] + factors(case)
    res, xs = {}, []
    x = (z @ t["fc.weight"].t() + t["fc.bias"]).reshape(B, -1, 1, 4, 4)
    for name, (ut, us) in zip(BLOCKS, steps):
        x = upsample(x, ut, us)
        xs.append(x)
        if c is None:
            r = gc.block(sub[name], x, z, img, cfgs[name], None, train, dtype)
            for k in r:
                if gc.is_buffer(k):
                    res[f"{name}.{k}"] = r[k]
            x = r["out"]
        else:   # (block() runs its forward again with the backward: the forward chain needs the outputs only)
            x = gc.block(sub[name], x, z, img, cfgs[name], None, train, dtype)["out"]
    a = gc.lrelu(x)
    pre = F.conv3d(a, t["conv_img.weight"], t["conv_img.bias"], padding=1)
    y = torch.tanh(pre)
    res["out"], res["pre"] = y.transpose(1, 2), pre
    if c is None:
        return res
    grads, scale = {}, {}
    gy = c.to(dtype).transpose(1, 2) * (1 - y * y)
    d_a, grads["conv_img.weight"], grads["conv_img.bias"] = gc.conv_grads(a, t["conv_img.weight"], gy, 1)
    g = d_a * gc.lrelu_slope(x)
    dz_blocks = torch.zeros_like(z)
    for name, (ut, us), xin in reversed(list(zip(BLOCKS, steps, xs))):
        r = gc.block(sub[name], xin, z, img, cfgs[name], g, train, dtype)
        for k in r:
            if gc.is_buffer(k):
                res[f"{name}.{k}"] = r[k]
        grads.update({f"{name}.{k}": v for k, v in r["grads"].items()})
        scale.update({f"{name}.{k}": v for k, v in r["scale"].items()})
        dz_blocks = dz_blocks + r["dz"]
        g = upsample_backward(r["dx"], ut, us)
    g = g.reshape(B, -1)
    grads["fc.weight"], grads["fc.bias"] = g.t() @ z, g.sum(0)
    res["dz_fc"], res["dz_blocks"] = g @ t["fc.weight"], dz_blocks
    res["dz"] = res["dz_fc"] + dz_blocks
    res["grads"], res["scale"] = grads, scale
    return res


def load_golden():
    """The fixtures' recorded results: every tests/golden/gen_train_*.npz merged."""
    out = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_train_*.npz"))):
        with np.load(path) as a:
            out.update({k: a[k] for k in a.files})
    for key in sorted({k.split("@")[0] for k in out if "@" in k}):      # an array too large for one file, cut along its second axis
        n = sum(1 for k in out if k.startswith(key + "@"))
        out[key] = np.concatenate([out.pop(f"{key}@{i}") for i in range(n)], axis=1)
    return out


def summary(key, grad):
    """What a fixture keeps of a large gradient: (float64 norm, its inner products with the N_DIRECTIONS seeded directions)."""
    g = np.asarray(torch.as_tensor(grad).detach().double().cpu())
    return float(np.linalg.norm(g)), np.array([float((g * direction(key, i, g.shape)).sum()) for i in range(N_DIRECTIONS)])


def check_summary(key, grad, golden, tag, tol):
    """A gradient against its fixture summary: a unit direction sees at most the whole distance, so each inner product and the norm lie
    within tol x the reference's norm.  -> the worst of them over that norm."""
    norm, proj = summary(key, grad)
    ref_norm, ref_proj = float(golden[f"{tag}.n.{key}"]), golden[f"{tag}.p.{key}"]
    worst = max(abs(norm - ref_norm), float(np.abs(proj - ref_proj).max())) / ref_norm
    assert worst <= tol, (key, worst)
    return worst


def gate_of(golden, tag, tensor):
    """The relative-L2 gate of one compared tensor (``out``, ``dz``, ``g.<key>``) of a case: TOL_L2 where the reference's own fp32 run
    stays a factor four inside it, else four times the reference's fp32 distance (the module docstring says why)."""
    d32 = float(golden[f"{tag}.d32.{tensor}"])
    return TOL_L2 if d32 <= TOL_L2 / 4 else 4 * d32


rel = gc.rel
