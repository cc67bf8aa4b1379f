"""Shared by tests/test_host_flow_train_units.py and tests/test_gpu_flow_train_units.py: the case matrix of the cINN TRAINING kernels
(csrc/i2v_flow_train.hip: ``chain_gemm<MODE, VEC>``, ``dw_gemm``, ``actnorm_grad``, ``fwd_link``, ``bwd_link``, ``adam_kernel``), a
reference of every kernel as a unit in float64 with a derived element-wise bound, a plain torch emulation of the whole pass built from
the same units (fp32: what the bounds are measured against on the CPU; float64: pinned to autograd through ``oracle/flow_ref``), and
the deliberate errors (``MUTATIONS``) that show what the gate catches.

A pass (forward + backward) keeps every intermediate in ``saved`` (layout: ``i2v_flow_train_saved_layout``).  ``Run`` holds those
regions by name, whether they come from the GPU or from the emulation, and ``check_units`` recomputes every unit in float64 FROM THE
RUN'S OWN INPUTS of that unit, so no error is carried from one unit to the next, and the LeakyReLU / InvLeakyRelu masks are read from the
saved values themselves: there is no kink problem at unit level.

Bounds, u = 2^-24.  All are dot-product bounds of any summation order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5)
with the counted extra roundings; ``TINY`` = 2^-126 per term is added where an operand may be subnormal (MFMA may flush subnormals).

* forward Linear  act = lrelu(W in + b): (R + 3) u (sum_k |W||in| + |b|), R the reduction length (R products and additions with the bias:
  R + 1; the LeakyReLU's constant 0.01f and its product: 2).  The bound is NOT scaled by the slope: an fp32 value on the other side of
  the kink than the float64 one differs from it by less than the unscaled bound (both lie within it of 0).
* dX  dpre[l-1] = m (W^T dY): (R + 2) u sum |W||dY|, m = 1 where the saved act[l-1] > 0, else 0.01.  dcin = sum_net W0^T dpre[0] is ONE
  reduction of length 2 H.
* dW, db: (B + 2) u sum_b |dY||X|, (B + 2) u sum_b |dY|.
* ActNorm: d_loc = scale sum_b g, d_scale = sum_b g (x + loc) + (sum_b d_logdet) / scale: (B + 4) u times the sum of the absolute terms
  (x + loc, the product, B additions, the quotient and the last addition).
* Coupling y = x e^s + t: C_EXP u |x| e^s + w |x e^s| + w |y|, w = UL u (below).  C_EXP = 4: ROCm's HIP math documentation states a maximum error of 1 ulp
  for the device expf and for logf; twice that is allotted, 2 ulp <= 4 u relative.
* ActNorm forward v = scale (y + loc) from the saved block input: |scale| w |y + loc| + w |v|; InvLeakyRelu (x 0.9f below 0): + 2 w |v|,
  unscaled for the same reason as above.  Shuffle, half swap, the copies into ``cin`` and its zero pad: exact (bound 0).
* Log-det, as a whole: sum_st sum_c s + sum_fl sum_c log|scale|.  A = the sum of the absolute terms.  (6 + C_EXP + 2 (S + 1)) u A: the
  64-lane butterfly adds in 6 levels, logf, and per link at most two additions onto running sums (S + 1 links).
* bwd_link  dout0 = dy x e^s + d_logdet: (C_EXP u + 2 w) |dy x e^s| + w |result|; part[32:] = dy e^s: (C_EXP u + w) |.|;
  gan = (part + dcin[:32]) x (1 | 0.9): w |sum| + 2 w |.|; d_x = gan scale, and dy of a block end = gan scale gathered: w |.|.
* Adam (``adam_one``), per element from the SAME fp32 state and the fp32 scalars the kernel is given, w = UL u per counted rounding:
  g' = g + wd p (2 roundings: dg = 2 w (|g| + |wd p|)), m' = m + (g' - m)(1 - b1) (3: dm = (1 - b1) dg + 2 w (1 - b1)(|g'| + |m|) + w |m'|),
  v' = v b2 + (1 - b2) g' g' (4: dv = 2 (1 - b2)|g'| dg + 2 w (1 - b2) g'^2 + w b2 v + w v'), q = sqrt(V) / bc2 (sqrtf and the division are
  correctly rounded in the default build: one rounding each: dq = (dV / sqrt(V) + w sqrt(V)) / bc2 + w q), D = q + eps: dD = dq + w D,
  r = m' / D: dr = dm / D + |m'| dD / D^2 + w |r|, p' = p - a r: dp = a dr + w a |r| + w |p'|.  vmax' = max(vmax, v') carries dv.

UL = 2: every counted rounding of a link and of Adam is charged one ulp (2 u relative at most), not the half ulp of a correctly
rounded operation.  A bound that charges half an ulp per rounding is attained: plain fp32 torch then uses up to 0.76 of it, and the
host test asks that the emulation stay within half of every bound, so that the GPU (other contraction into FMAs, other order) has room.
The GEMM bounds need no such factor: their (R + c) u sum |.| is the worst case over R roundings per term.

Gate: every element |got - ref64| <= bound + u |ref64|; a value that is not finite fails.

What cannot be checked as a unit (``d_embed`` is summed over the half-steps; ``part`` and ``dcin`` of the later half-steps are
overwritten) is checked end to end: float64 autograd through ``oracle/flow_ref``'s leaf functions composed in the order the flags
select, per-tensor rel-L2 <= 1e-4, on samples whose every LeakyReLU / InvLeakyRelu input is >= 1e-5 away from 0 in the float64
oracle (the rule of tests/test_gpu_flow_train.py)."""
import contextlib
import types

import numpy as np
import torch
import torch.nn.functional as F

import flow_train_common as fc
import flow_units_common as fu
from flow_units_common import NFL, block_cond

U = 2.0 ** -24
TINY = 2.0 ** -126
S = 2 * NFL
C_EXP = 4.0
UL = 2.0                 # what one counted rounding of a link is charged, in u
TOL_L2 = 1e-4
KINK_MARGIN = 1e-5
POOL_FACTOR = 16         # candidates drawn per sample of a batch: 1 / 8 of them must qualify, which gives the two batches a case uses
LAYOUT_FIELDS = ("KP", "step_sz", "o_cin", "o_act", "o_out", "o_dpre", "o_dout", "o_xin", "o_gan", "o_part", "o_dcin", "total")

MUTATIONS = (
    "dw_drop_last_sample",      # dW without the last sample
    "dw_ragged_block0",         # dW of a first layer with ragged K > 64: columns >= 64 taken from column block 0
    "db_drop_sample",           # db without one sample
    "dscale_no_dlogdet",        # d_scale without the d_logdet / scale term
    "dx_mask_wrong_layer",      # the dX mask taken from layer l instead of l - 1
    "dcin_drop_tnet",           # dX of the first layer with the t-net segment dropped
    "cin_drop_last_embed",      # the embedding column E - 1 dropped from cin
    "cond_offset_32",           # the 'normal' offset 32 used in 'cond' mode
    "logdet_missing_channel",   # the log-det missing one channel
    "dout0_no_dlogdet",         # dout(st, 0) without d_logdet
    "no_unswap",                # the un-swap omitted
    "accumulate_overwrites",    # accumulate = 1 overwriting instead of adding
    "adam_tail_not_updated",    # the last element of a tensor whose numel is no multiple of 4 not updated
    "adam_vmax_not_maxed",      # vmax = v instead of max(vmax, v)
    "adam_bc2_wrong_step",      # bc2_sqrt of the neighbouring step
)
ADAM_MUTATIONS = tuple(m for m in MUTATIONS if m.startswith("adam_"))


# ---------------------------------------------------------------------------------------------------------------- the case matrix

def _case(group, hidden, depth, E, control=0, flags=(False, False, "lrelu"), B=17):
    c = dict(group=group, hidden=hidden, depth=depth, E=E, control=control, skip_an=flags[0], skip_sh=flags[1], act=flags[2], B=B)
    c["id"] = (f"{group}-h{hidden}-d{depth}-e{E}-c{control}-b{B}" + ("-noan" if flags[0] else "") + ("-nosh" if flags[1] else "") +
               ("-noact" if flags[2] != "lrelu" else ""))
    return c


def cases():
    out = []
    for hidden in (128, 256, 384, 512):
        for B in (17, 65):
            out.append(_case("hidden", hidden, 2, 64, B=B))
    for hidden in (128, 384):
        for depth in (1, 3):
            out.append(_case("depth", hidden, depth, 64))
    for E in (1, 15, 16, 17, 93, 94, 95, 97, 128):
        for control in (0, 1, 2):
            out.append(_case("embed", 128, 2, E, control))
    for flags in fu.FLAG_SETS:
        out.append(_case("flags", 128, 2, 64, flags=flags))
    for B in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130):
        out.append(_case("batch", 128, 2, 94, 1, B=B))
    return out


CASES = cases()


def group(name):
    return [c for c in CASES if c["group"] == name]


def cond(case, st):
    return block_cond(case["control"], st // 2)


def kin(case, st):
    return case["E"] if cond(case, st) else 32 + case["E"]


def kp(case):
    return (32 + case["E"] + 3) // 4 * 4


def expressible(case):
    """``flow_ref.flow_forward`` (and so ``oracle_grads`` / ``kink_margins``) covers the default flags and control 0 / 1"""
    return case["control"] in (0, 1) and not case["skip_an"] and not case["skip_sh"] and case["act"] == "lrelu"


def branches(case):
    """What a pass of the case runs: the ledger entries"""
    out = set()
    for st in range(S):
        k = kin(case, st)
        out.add(("chain0", "vec" if k % 16 == 0 else "novec"))
        out.add(("cin", "cond" if cond(case, st) else "normal"))
    out |= {("chain0", "vec"), ("chain1", "one_segment"), ("chain1", "two_segments"), ("dw", "first"), ("dw", "middle"), ("dw", "last"),
            ("link", "actnorm" if not case["skip_an"] else "no_actnorm"), ("link", "shuffle" if not case["skip_sh"] else "no_shuffle"),
            ("link", "act" if case["act"] == "lrelu" else "no_act")}
    return out


LEDGER_WANT = {("chain0", "vec"), ("chain0", "novec"), ("chain1", "one_segment"), ("chain1", "two_segments"), ("dw", "first"), ("dw", "middle"),
               ("dw", "last"), ("cin", "cond"), ("cin", "normal"), ("link", "actnorm"), ("link", "no_actnorm"), ("link", "shuffle"),
               ("link", "no_shuffle"), ("link", "act"), ("link", "no_act")}


def regions(case, B, L):
    """(name, offset in floats, shape) of every region of ``saved`` under the layout L ({field: value})"""
    H, D, KP = case["hidden"], case["depth"], L["KP"]
    for st in range(S):
        base = st * L["step_sz"]
        yield ("xs", st), base, (B, 64)
        yield ("cin", st), base + L["o_cin"], (B, KP)
        for net in range(2):
            for l in range(D + 1):
                yield ("act", st, net, l), base + L["o_act"] + (net * (D + 1) + l) * B * H, (B, H)
                yield ("dpre", st, net, l), base + L["o_dpre"] + (net * (D + 1) + l) * B * H, (B, H)
            yield ("out", st, net), base + L["o_out"] + net * B * 32, (B, 32)
            yield ("dout", st, net), base + L["o_dout"] + net * B * 32, (B, 32)
    for fl in range(NFL):
        yield ("xin", fl), L["o_xin"] + fl * B * 64, (B, 64)
        yield ("gan", fl), L["o_gan"] + fl * B * 64, (B, 64)
    yield ("part",), L["o_part"], (B, 64)
    yield ("dcin",), L["o_dcin"], (B, KP)


# ---------------------------------------------------------------------------------------------------------------- parameters, inputs

def params(case, dt):
    return {k: (v.to(dt) if v.is_floating_point() else v) for k, v in fu.tensors(fu.state_dict(case)).items()}


def lin_key(st, net, l):
    return f"sub_layers.{st // 2}.coupling.{'st'[net]}.{st & 1}.main.{2 * l}"


def lin(P, st, net, l):
    k = lin_key(st, net, l)
    return P[k + ".weight"], P[k + ".bias"]


def actnorm(P, fl):
    return P[f"sub_layers.{fl}.norm_layer.loc"].reshape(1, 64), P[f"sub_layers.{fl}.norm_layer.scale"].reshape(1, 64)


def shuffle_idx(P, fl):
    return P[f"sub_layers.{fl}.shuffle.forward_shuffle_idx"], P[f"sub_layers.{fl}.shuffle.backward_shuffle_idx"]


def grad_keys(case):
    """state_dict keys of the tensors a backward writes"""
    keys = [lin_key(st, net, l) + s for st in range(S) for net in range(2) for l in range(case["depth"] + 2) for s in (".weight", ".bias")]
    if not case["skip_an"]:
        keys += [f"sub_layers.{fl}.norm_layer.{n}" for fl in range(NFL) for n in ("loc", "scale")]
    return keys


def composed_forward(sd, x, e, case):
    """``oracle/flow_ref``'s leaf functions in the order the case's flags select -> (zt [B, 64], logdet [B])"""
    from oracle import flow_ref
    h, ld = x, torch.zeros(x.shape[0], dtype=x.dtype)
    for fl in range(NFL):
        p = f"sub_layers.{fl}."
        if not case["skip_an"]:
            h, l = flow_ref.actnorm_forward(sd, p + "norm_layer.", h)
            ld = ld + l
        if case["act"] == "lrelu":
            h = flow_ref.inv_lrelu_forward(h)
        h, l = flow_ref.coupling_forward(sd, p + "coupling.", h, e, "cond" if block_cond(case["control"], fl) else "normal", case["depth"])
        ld = ld + l
        if not case["skip_sh"]:
            h = h[:, sd[p + "shuffle.forward_shuffle_idx"]]
    return h, ld


def autograd_ref(case, x, e, d_zt, d_ld, dt=torch.float64, composed=None):
    """Autograd through the oracle in ``dt`` -> (zt [B, 64], logdet [B], {"x", "embed", state_dict key: gradient}): ``oracle_grads`` where
    ``flow_ref.flow_forward`` expresses the case, else the composed forward"""
    sd_np = fu.state_dict(case)
    if expressible(case) if composed is None else not composed:
        zt, ld, _, grads = fc.oracle_grads(sd_np, x, e, dt, NFL, bool(case["control"]), d_zt, d_ld, depth=case["depth"])
        return zt, ld, grads
    with torch.enable_grad():
        sd = {k: (v.clone().to(dt).requires_grad_(True) if v.is_floating_point() else v) for k, v in fu.tensors(sd_np).items()}
        xg, eg = x.detach().clone().to(dt).requires_grad_(True), e.detach().clone().to(dt).requires_grad_(True)
        zt, ld = composed_forward(sd, xg, eg, case)
        ((zt * d_zt.to(dt)).sum() + (ld * d_ld.to(dt)).sum()).backward()
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.grad is not None}
    grads["x"], grads["embed"] = xg.grad, eg.grad
    return zt.detach(), ld.detach(), grads


@contextlib.contextmanager
def _recording(rec):
    """Every LeakyReLU / InvLeakyRelu input of the oracle into ``rec``, the way ``flow_train_common.kink_margins`` instruments it"""
    from oracle import flow_ref
    orig_f, orig_inv = flow_ref.F, flow_ref.inv_lrelu_forward

    def lrelu(h, slope):
        rec.append(h.detach())
        return F.leaky_relu(h, slope)

    def inv(h, alpha=0.9):
        rec.append(h.detach())
        return orig_inv(h, alpha)
    flow_ref.F, flow_ref.inv_lrelu_forward = types.SimpleNamespace(linear=F.linear, leaky_relu=lrelu), inv
    try:
        yield
    finally:
        flow_ref.F, flow_ref.inv_lrelu_forward = orig_f, orig_inv


def margins(case, x, e, composed=None):
    """Per sample, the smallest |input| of any LeakyReLU / InvLeakyRelu of the float64 oracle.  A case without any such input (depth
    and activation leave at least the s- / t-nets' LeakyReLUs, so there is always one) would give +inf."""
    if expressible(case) if composed is None else not composed:
        return fc.kink_margins(fu.state_dict(case), x, e, NFL, bool(case["control"]), depth=case["depth"])[0]
    rec = []
    with _recording(rec), torch.no_grad():
        composed_forward(params(case, torch.float64), x.double(), e.double(), case)
    return torch.stack([h.abs().min(1).values for h in rec]).min(0).values


_POOLS = {}


def pool(case):
    """(x, e, kept, drawn): ``POOL_FACTOR`` B candidates (at least 64) of the geometry's seeded stream, kept when >= KINK_MARGIN away from
    every kink in the float64 oracle.  The rule looks at the oracle alone."""
    key = (fu.geometry_key(case), case["B"])
    if key not in _POOLS:
        n = max(64, POOL_FACTOR * case["B"])
        x, e = fu.candidates(case, n)
        keep = (margins(case, x, e) >= KINK_MARGIN).nonzero().flatten()
        _POOLS[key] = (x[keep].contiguous(), e[keep].contiguous(), int(len(keep)), n)
    return _POOLS[key]


OWN_FP32 = 1e-5          # the standing check of tests/test_gpu_flow_train.py: the reference's own fp32 gradients against float64
_INPUTS = {}


def inputs(case, which=0):
    """(x, e, d_zt, d_logdet) of a case: the first B kink-free samples (``which`` = 1: the next B, for the second backward of the
    accumulation check) and seeded normal cotangents.  The first-layer bias gradients of these short, sign-coherent flows are sums that
    cancel, and with some cotangents the oracle's own fp32 autograd is then 1 .. 3e-5 from float64 on such a tensor although no kink
    is near.  The 1e-4 gate is a statement about points where the reference itself is good to 1e-5, so the cotangents are the first
    of up to 16 seeded draws at which the oracle's fp32 run is within HALF of ``OWN_FP32`` of its float64 run on every tensor -- a rule
    that looks at the oracle alone, decided on the CPU; the tests assert ``own`` <= OWN_FP32."""
    return reference(case, which)[:4]


def reference(case, which=0):
    """-> (x, e, d_zt, d_logdet, ``autograd_ref`` in float64, own: the largest rel-L2 of the oracle's fp32 run against it, draws used)"""
    key = (case["id"], which)
    if key not in _INPUTS:
        B = case["B"]
        x, e, kept, drawn = pool(case)
        assert kept >= 2 * B and 8 * kept >= drawn, (case["id"], kept, drawn)
        x, e = x[which * B:(which + 1) * B].contiguous(), e[which * B:(which + 1) * B].contiguous()
        for draw in range(16):
            g = torch.Generator().manual_seed(777 + 31 * B + case["E"] + 1000 * which + 100000 * draw)
            d_zt, d_ld = torch.randn(B, 64, generator=g), torch.randn(B, generator=g)
            ref = autograd_ref(case, x, e, d_zt, d_ld)
            r32 = autograd_ref(case, x, e, d_zt, d_ld, torch.float32)
            own = max(max(fc.rel(r32[2][k], ref[2][k]) for k in ref[2]), fc.rel(r32[0], ref[0]), fc.rel(r32[1], ref[1]))
            if own <= 0.5 * OWN_FP32:
                break
        _INPUTS[key] = (x, e, d_zt, d_ld, ref, own, draw + 1)
    return _INPUTS[key]


# ---------------------------------------------------------------------------------------------------------------- the units

def _lrelu(y, mask_of, slope):
    return torch.where(mask_of > 0, y, y * slope)


def u_linear(X, W, b, act):
    y = X @ W.T + b
    return _lrelu(y, y, 0.01) if act else y


def b_linear(X, W, b):
    R = W.shape[1]
    return (R + 3) * U * (X.abs() @ W.abs().T + b.abs()) + R * TINY


def u_dx(dY, W, mask):
    v = dY @ W
    return v if mask is None else _lrelu(v, mask, 0.01)


def b_dx(dY, W):
    R = W.shape[0]
    return (R + 2) * U * (dY.abs() @ W.abs()) + R * TINY


def u_dw(dY, X):
    return dY.T @ X, dY.sum(0)


def b_dw(dY, X):
    B = dY.shape[0]
    return (B + 2) * U * (dY.abs().T @ X.abs()) + B * TINY, (B + 2) * U * dY.abs().sum(0) + B * TINY


def u_actnorm_grad(g, xin, dld, loc, scale):
    return (g.sum(0) * scale).reshape(-1), ((g * (xin + loc)).sum(0) + dld.sum() / scale).reshape(-1)


def b_actnorm_grad(g, xin, dld, loc, scale):
    B = g.shape[0]
    return ((B + 4) * U * (g.abs().sum(0) * scale.abs())).reshape(-1), \
           ((B + 4) * U * ((g.abs() * (xin + loc).abs()).sum(0) + dld.abs().sum() / scale.abs())).reshape(-1)


def _side(v, neg):
    """1 where v >= 0, ``neg`` elsewhere, in v's dtype"""
    return torch.where(v >= 0, torch.ones_like(v), torch.full_like(v, neg))


def _swap(v):
    return torch.cat((v[:, 32:], v[:, :32]), 1)


def dw_operands(R, st, net, l):
    """(dY, X) of the dW / db of Linear l, as ``dw_gemm`` picks them"""
    c = R.case
    D = c["depth"]
    if l == 0:
        return R["dpre", st, net, 0], R["cin", st][:, :kin(c, st)]
    if l <= D:
        return R["dpre", st, net, l], R["act", st, net, l - 1]
    return R["dout", st, net], R["act", st, net, D]


class Run:
    """The record of one forward + backward: the regions of ``saved`` by name, zt, logdet, d_x, d_embed and the parameter gradients"""

    def __init__(self, case, B):
        self.case, self.B, self.v, self.grads = case, B, {}, {}
        self.zt = self.logdet = self.d_x = self.d_embed = None

    def __getitem__(self, k):
        return self.v[k]

    def __setitem__(self, k, t):
        self.v[k] = t

    def double(self):
        r = Run(self.case, self.B)
        r.v = {k: t.double() for k, t in self.v.items()}
        r.grads = {k: t.double() for k, t in self.grads.items()}
        r.zt, r.logdet, r.d_x, r.d_embed = (None if t is None else t.double() for t in (self.zt, self.logdet, self.d_x, self.d_embed))
        return r

    @staticmethod
    def from_saved(case, B, L, saved, zt, logdet, d_x, d_embed, grads):
        """saved: the flat float32 CPU tensor; grads: {state_dict key: tensor}"""
        r = Run(case, B)
        for name, off, shape in regions(case, B, L):
            r.v[name] = saved[off:off + shape[0] * shape[1]].reshape(shape)
        r.zt, r.logdet, r.d_x, r.d_embed, r.grads = zt, logdet, d_x, d_embed, dict(grads)
        return r


def emulate(case, x, e, d_zt, d_ld, dt=torch.float32, mutate=None):
    """The whole pass in plain torch in ``dt``, launch by launch as the host code of i2v_flow_train.hip schedules it, with one
    deliberate error where ``mutate`` names one -> Run"""
    c, B, D, E = case, x.shape[0], case["depth"], case["E"]
    P = params(case, dt)
    x, e, d_zt, d_ld = x.to(dt), e.to(dt), d_zt.to(dt), d_ld.to(dt)
    R = Run(case, B)
    use_an, use_sh, use_act = not c["skip_an"], not c["skip_sh"], c["act"] == "lrelu"
    KP = kp(c)
    for st in range(-1, S):
        if st >= 0:
            for net in range(2):
                for l in range(D + 2):
                    X = R["cin", st][:, :kin(c, st)] if l == 0 else R["act", st, net, l - 1]
                    R[("out", st, net) if l == D + 1 else ("act", st, net, l)] = u_linear(X, *lin(P, st, net, l), act=l <= D)
        if st < 0:
            y, ld = x, torch.zeros(B, dtype=dt)
        else:
            xs, s, t = R["xs", st], R["out", st, 0], R["out", st, 1]
            y = torch.cat((xs[:, :32], xs[:, 32:] * torch.exp(s) + t), 1)
            ld = (s[:, :31] if mutate == "logdet_missing_channel" and st == S - 1 else s).sum(1)
        if st >= 0 and not st & 1:
            y = _swap(y)
        else:
            if st >= 0 and use_sh:
                y = y[:, shuffle_idx(P, st // 2)[0]]
            if st == S - 1:
                R.zt, R.logdet = y, R.logdet + ld
                break
            fl = (st + 1) // 2
            R["xin", fl] = y
            if use_an:
                loc, scale = actnorm(P, fl)
                y = scale * (y + loc)
                ld = ld + torch.log(scale.abs()).sum()
            if use_act:
                y = torch.where(y >= 0, y, y * 0.9)
        R["xs", st + 1] = y
        cn = cond(c, st + 1)
        cin = torch.zeros(B, KP, dtype=dt)
        off = 0 if cn and mutate != "cond_offset_32" else 32
        if not cn:
            cin[:, :32] = y[:, :32]
        cin[:, off:off + E] = e
        if mutate == "cin_drop_last_embed" and st + 1 == S - 1:
            cin[:, off + E - 1] = 0
        R["cin", st + 1] = cin
        R.logdet = ld if st < 0 else R.logdet + ld
    part = dcin = None
    for st in range(S - 1, -2, -1):
        if st == S - 1:
            dy = d_zt[:, shuffle_idx(P, NFL - 1)[1]] if use_sh else d_zt
        else:
            t1 = st + 1
            c1 = cond(c, t1)
            gx = part.clone()
            if not c1:
                gx[:, :32] += dcin[:, :32]
            off = 0 if c1 else 32
            de = dcin[:, off:off + E]
            R.d_embed = de.clone() if t1 == S - 1 else R.d_embed + de
            if t1 & 1:
                dy = gx if mutate == "no_unswap" else _swap(gx)
            else:
                fl = t1 >> 1
                if use_act:
                    gx = gx * _side(R["xs", t1], 0.9)
                R["gan", fl] = gx
                if use_an:
                    gx = gx * actnorm(P, fl)[1]
                if fl == 0:
                    R.d_x = gx
                    break
                dy = gx[:, shuffle_idx(P, fl - 1)[1]] if use_sh else gx
        es = torch.exp(R["out", st, 0])
        d0 = dy[:, 32:] * R["xs", st][:, 32:] * es
        R["dout", st, 0] = d0 if mutate == "dout0_no_dlogdet" and st == 1 else d0 + d_ld[:, None]
        R["dout", st, 1] = dy[:, 32:].clone()
        part = torch.cat((dy[:, :32], dy[:, 32:] * es), 1)
        for l in range(D + 1, 0, -1):
            for net in range(2):
                dY = R["dout", st, net] if l == D + 1 else R["dpre", st, net, l]
                ml = l if mutate == "dx_mask_wrong_layer" and l <= D and st == 2 else l - 1
                R["dpre", st, net, l - 1] = u_dx(dY, lin(P, st, net, l)[0], R["act", st, net, ml])
        nets = (0,) if mutate == "dcin_drop_tnet" and st == 2 else (0, 1)
        dcin = torch.zeros(B, KP, dtype=dt)
        dcin[:, :kin(c, st)] = u_dx(torch.cat([R["dpre", st, n, 0] for n in nets], 1), torch.cat([lin(P, st, n, 0)[0] for n in nets], 0), None)
    R["part",], R["dcin",] = part, dcin
    for st in range(S):
        for net in range(2):
            for l in range(D + 2):
                dY, X = dw_operands(R, st, net, l)
                here = (st, net) == (1, 1)
                dW, db = u_dw(dY, X)
                if mutate == "dw_drop_last_sample" and here and l == 1:
                    dW = u_dw(dY[:-1], X[:-1])[0]
                if mutate == "dw_ragged_block0" and l == 0 and X.shape[1] > 64 and X.shape[1] % 64:
                    dW = torch.cat((dW[:, :64], dW[:, :X.shape[1] - 64]), 1)
                if mutate == "db_drop_sample" and here and l == D + 1:
                    db = u_dw(dY[1:], X[1:])[1]
                k = lin_key(st, net, l)
                R.grads[k + ".weight"], R.grads[k + ".bias"] = dW, db
    if use_an:
        for fl in range(NFL):
            loc, scale = actnorm(P, fl)
            dl, ds = u_actnorm_grad(R["gan", fl], R["xin", fl], torch.zeros_like(d_ld) if mutate == "dscale_no_dlogdet" and fl == 1 else d_ld,
                                    loc, scale)
            R.grads[f"sub_layers.{fl}.norm_layer.loc"], R.grads[f"sub_layers.{fl}.norm_layer.scale"] = dl, ds
    return R


# ---------------------------------------------------------------------------------------------------------------- the unit references

def grad_refs(R, d_ld):
    """{state_dict key: (kind, float64 reference, bound)} of every parameter gradient, from the operands the run itself saved"""
    c, D = R.case, R.case["depth"]
    R, P = R.double(), params(R.case, torch.float64)
    out = {}
    for st in range(S):
        for net in range(2):
            for l in range(D + 2):
                dY, X = dw_operands(R, st, net, l)
                (dW, db), (bW, bb) = u_dw(dY, X), b_dw(dY, X)
                k = lin_key(st, net, l)
                out[k + ".weight"], out[k + ".bias"] = ("dw", dW, bW), ("db", db, bb)
    if not c["skip_an"]:
        for fl in range(NFL):
            a = (R["gan", fl], R["xin", fl], d_ld.double()) + actnorm(P, fl)
            (dl, ds), (bl, bs) = u_actnorm_grad(*a), b_actnorm_grad(*a)
            out[f"sub_layers.{fl}.norm_layer.loc"], out[f"sub_layers.{fl}.norm_layer.scale"] = ("actnorm", dl, bl), ("actnorm", ds, bs)
    return out


def unit_refs(run, x, e, d_zt, d_ld):
    """Yields (kind, name, got, float64 reference, bound) of every unit of a pass, each from the run's own saved inputs of that unit.
    ``got`` is the run's value (fp32 or whatever the run holds); a bound of None means exact."""
    c, B, D, E = run.case, run.B, run.case["depth"], run.case["E"]
    R, P = run.double(), params(run.case, torch.float64)
    x, e, d_zt, d_ld = x.double(), e.double(), d_zt.double(), d_ld.double()
    use_an, use_sh, use_act = not c["skip_an"], not c["skip_sh"], c["act"] == "lrelu"
    for st in range(S):
        K = kin(c, st)
        for net in range(2):
            for l in range(D + 2):                                   # forward Linear
                X = R["cin", st][:, :K] if l == 0 else R["act", st, net, l - 1]
                W, b = lin(P, st, net, l)
                name = ("out", st, net) if l == D + 1 else ("act", st, net, l)
                yield "linear", name, run[name], u_linear(X, W, b, l <= D), b_linear(X, W, b)
            for l in range(D + 1, 0, -1):                            # dX
                dY = R["dout", st, net] if l == D + 1 else R["dpre", st, net, l]
                W = lin(P, st, net, l)[0]
                name = ("dpre", st, net, l - 1)
                yield "dx", name, run[name], u_dx(dY, W, R["act", st, net, l - 1]), b_dx(dY, W)
        # cin: the kept half as saved in xs, the embedding, zeros behind it
        cin = torch.zeros(B, kp(c), dtype=torch.float64)
        if cond(c, st):
            cin[:, :E] = e
        else:
            cin[:, :32], cin[:, 32:32 + E] = R["xs", st][:, :32], e
        yield "cin", ("cin", st), run["cin", st], cin, None
    dY, W = torch.cat([R["dpre", 0, n, 0] for n in range(2)], 1), torch.cat([lin(P, 0, n, 0)[0] for n in range(2)], 0)
    K = kin(c, 0)
    yield "dcin", ("dcin",), run["dcin",][:, :K], u_dx(dY, W, None), b_dx(dY, W)
    yield "dcin", ("dcin", "pad"), run["dcin",][:, K:], torch.zeros(B, kp(c) - K, dtype=torch.float64), None
    for k, (kind, ref, bound) in grad_refs(run, d_ld).items():
        yield kind, k, run.grads[k].reshape(ref.shape), ref, bound
    # forward links
    ld, ld_abs = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for st in range(-1, S):
        if st < 0:
            y, dy = x, torch.zeros_like(x)
        else:
            xs, s, t = R["xs", st], R["out", st, 0], R["out", st, 1]
            xe = xs[:, 32:] * torch.exp(s)
            ya = xe + t
            y = torch.cat((xs[:, :32], ya), 1)
            dy = torch.cat((torch.zeros(B, 32, dtype=torch.float64), (C_EXP + UL) * U * xe.abs() + UL * U * ya.abs() + TINY), 1)
            ld, ld_abs = ld + s.sum(1), ld_abs + s.abs().sum(1)
        if st >= 0 and not st & 1:
            yield "fwd_link", ("xs", st + 1), run["xs", st + 1], _swap(y), _swap(dy)
            continue
        if st >= 0 and use_sh:
            f = shuffle_idx(P, st // 2)[0]
            y, dy = y[:, f], dy[:, f]
        if st == S - 1:
            yield "zt", ("zt",), run.zt, y, dy
            break
        fl = (st + 1) // 2
        yield "fwd_link", ("xin", fl), run["xin", fl], y, dy
        v, dv = R["xin", fl], torch.zeros(B, 64, dtype=torch.float64)      # from here on: from the block input as saved
        if use_an:
            loc, scale = actnorm(P, fl)
            a = v + loc
            v = scale * a
            dv = UL * U * (scale.abs() * a.abs() + v.abs())
            k = torch.log(scale.abs())
            ld, ld_abs = ld + k.sum(), ld_abs + k.abs().sum()
        if use_act:
            v = torch.where(v >= 0, v, v * 0.9)
            dv = dv + 2 * UL * U * v.abs()
        yield "fwd_link", ("xs", st + 1), run["xs", st + 1], v, dv
    yield "logdet", ("logdet",), run.logdet, ld, (6 + C_EXP + 2 * (S + 1)) * U * ld_abs
    # backward links
    for st in range(S - 1, -1, -1):
        dy = R["dout", st, 1]
        if st == S - 1:
            want = (d_zt[:, shuffle_idx(P, NFL - 1)[1]] if use_sh else d_zt)[:, 32:]
            yield "bwd_link", ("dout", st, 1), run["dout", st, 1], want, None
        elif st & 1:
            fl = (st + 1) // 2
            g = R["gan", fl] * (actnorm(P, fl)[1] if use_an else 1.0)
            g = (g[:, shuffle_idx(P, fl - 1)[1]] if use_sh else g)[:, 32:]
            yield "bwd_link", ("dout", st, 1), run["dout", st, 1], g, (UL * U * g.abs() if use_an else None)
        es = torch.exp(R["out", st, 0])
        prod = dy * R["xs", st][:, 32:] * es
        ref = prod + d_ld[:, None]
        yield "bwd_link", ("dout", st, 0), run["dout", st, 0], ref, (C_EXP + 2 * UL) * U * prod.abs() + UL * U * ref.abs() + TINY
        if st == 0:
            pe = dy * es
            yield "bwd_link", ("part", "upper"), run["part",][:, 32:], pe, (C_EXP + UL) * U * pe.abs() + TINY
    g = R["part",].clone()
    dg = torch.zeros_like(g)
    if not cond(c, 0):
        g[:, :32] += R["dcin",][:, :32]
        dg[:, :32] = UL * U * g[:, :32].abs()
    if use_act:
        g = g * _side(R["xs", 0], 0.9)
        dg = dg + 2 * UL * U * g.abs()
    yield "bwd_link", ("gan", 0), run["gan", 0], g, dg
    if run.d_x is not None:
        gx = R["gan", 0] * (actnorm(P, 0)[1] if use_an else 1.0)
        yield "bwd_link", ("d_x",), run.d_x, gx, (UL * U * gx.abs() if use_an else None)


def ratio(got, ref, bound):
    """worst |got - ref| / (bound + u |ref|) (0 / 0 = 0); inf where got is not finite or the shapes differ"""
    if tuple(got.shape) != tuple(ref.shape) or not bool(torch.isfinite(got).all()):
        return float("inf")
    if got.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    lim = U * ref.abs() if bound is None else bound + U * ref.abs()
    return float(torch.where(err == 0, torch.zeros_like(err), torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.full_like(err, float("inf")))).max())


def check_units(run, x, e, d_zt, d_ld):
    """-> ({kind: worst ratio}, [(kind, name, ratio) above 1])"""
    worst, bad = {}, []
    for kind, name, got, ref, bound in unit_refs(run, x, e, d_zt, d_ld):
        r = ratio(got, ref, bound)
        worst[kind] = max(worst.get(kind, 0.0), r)
        if not r <= 1.0:
            bad.append((kind, name, r))
    return worst, bad


def check_e2e(case, run, ref):
    """rel-L2 of every gradient tensor, d_x, d_embed, zt and logdet against ``autograd_ref`` -> ({name: rel-L2}, [(name, rel-L2) above 1e-4])"""
    zt, ld, grads = ref
    pairs = {"zt": (run.zt, zt), "logdet": (run.logdet, ld), "d_x": (run.d_x, grads["x"]), "d_embed": (run.d_embed, grads["embed"])}
    for k in grad_keys(case):
        pairs[k] = (run.grads[k], grads[k])
    errs = {}
    for k, (got, want) in pairs.items():
        errs[k] = fc.rel(got, want) if bool(torch.isfinite(torch.as_tensor(got)).all()) else float("inf")
    return errs, [(k, v) for k, v in errs.items() if not v <= TOL_L2]


def check_accumulate(run1, run2, got, d_ld1, d_ld2):
    """The gradients ``got`` of two backwards into one buffer against the float64 sum of both runs' unit references, within
    bound1 + bound2 + u |sum| -> (worst ratio, [(key, ratio) above 1])"""
    r1, r2 = grad_refs(run1, d_ld1), grad_refs(run2, d_ld2)
    worst, bad = 0.0, []
    for k in r1:
        r = ratio(got[k].reshape(r1[k][1].shape), r1[k][1] + r2[k][1], r1[k][2] + r2[k][2])
        worst = max(worst, r)
        if not r <= 1.0:
            bad.append((k, r))
    return worst, bad


# ---------------------------------------------------------------------------------------------------------------- Adam

ADAM_NUMELS = (1, 3, 4, 5, 7, 2047, 2048, 2049, 4099)
ADAM_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8)
ADAM_STEPS = (1, 2, 3, 1000)      # three consecutive steps, then one launch far along


def adam_slices(shift):
    """[(start, numel)] of the tensors in one flat buffer, every start = ``shift`` (mod 4) floats, at least one guard float between
    neighbours -> (slices, total)"""
    out, off = [], 0
    for n in ADAM_NUMELS:
        start = (off + 3) // 4 * 4 + shift
        out.append((start, n))
        off = start + n + 1
    return out, off + 4


def adam_scalars(step, wd, lr, beta1, beta2, eps):
    """The fp32 scalars ``i2v_adam_step`` hands to the kernel (its arguments are C floats; the bias corrections are formed in double)"""
    f = lambda v: float(np.float32(v))   # noqa: E731
    b1, b2 = f(beta1), f(beta2)
    return dict(step_size=f(f(lr) / (1.0 - b1 ** step)), bc2_sqrt=f(np.sqrt(1.0 - b2 ** step)), b1=b1, b2=b2, omb1=f(np.float32(1) - np.float32(b1)),
                omb2=f(np.float32(1) - np.float32(b2)), eps=f(eps), wd=f(wd))


def adam_one(p, g, m, v, vm, sc, amsgrad, dt=torch.float64, mutate=None):
    """``adam_one`` of the kernel on flat tensors in ``dt`` -> (p', m', v', vm' or None[, bounds (dp, dm, dv, dvm) in float64])"""
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    k = {n: torch.tensor(val, dtype=dt) for n, val in sc.items()}
    dg = torch.zeros_like(g)
    if sc["wd"] != 0.0:
        dg = 2 * UL * U * (g.abs() + (k["wd"] * p).abs())
        g = g + k["wd"] * p
    m2 = m + (g - m) * k["omb1"]
    v2 = v * k["b2"] + k["omb2"] * g * g
    if amsgrad:
        vm2 = v2.clone() if mutate == "adam_vmax_not_maxed" else torch.maximum(vm.to(dt), v2)
        V = vm2
    else:
        vm2, V = None, v2
    q = torch.sqrt(V) / k["bc2_sqrt"]
    D = q + k["eps"]
    r = m2 / D
    p2 = p - k["step_size"] * r
    if mutate == "adam_tail_not_updated" and p.numel() % 4:
        p2[-1] = p[-1]
    if dt != torch.float64:
        return p2, m2, v2, vm2
    u1 = UL * U
    dm = k["omb1"] * dg + 2 * u1 * k["omb1"] * (g.abs() + m.abs()) + u1 * m2.abs()
    dv = 2 * k["omb2"] * g.abs() * dg + 2 * u1 * k["omb2"] * g * g + u1 * k["b2"] * v + u1 * v2 + 4 * TINY
    sq = torch.sqrt(V)
    dsq = torch.where(sq > 0, dv / sq.clamp_min(1e-300), torch.sqrt(dv))
    dq = (dsq + u1 * sq) / k["bc2_sqrt"] + u1 * q
    dD = dq + u1 * D
    dr = dm / D + m2.abs() * dD / (D * D) + u1 * r.abs()
    dp = k["step_size"] * dr + u1 * k["step_size"] * r.abs() + u1 * p2.abs()
    return p2, m2, v2, vm2, (dp, dm, dv, dv)


def adam_state(shift_p, shift_g, seed=0):
    """Flat fp32 buffers {p, g, m, v, vm} and their slices: p, m, v, vm share ``shift_p``; every float outside a slice is a guard"""
    gen = torch.Generator().manual_seed(4242 + seed)
    sp, tp = adam_slices(shift_p)
    sg, tg = adam_slices(shift_g)
    buf = {"p": torch.randn(tp, generator=gen), "g": 0.3 * torch.randn(tg, generator=gen), "m": 0.1 * torch.randn(tp, generator=gen),
           "v": 0.05 * torch.randn(tp, generator=gen) ** 2, "vm": 0.05 * torch.randn(tp, generator=gen) ** 2}
    return buf, {"p": sp, "g": sg, "m": sp, "v": sp, "vm": sp}


def adam_check(before, after, slices, sc, amsgrad):
    """One launch: ``after`` against the float64 update of ``before`` (both {name: flat fp32 buffer}; "vm" absent without amsgrad) ->
    (worst ratio, failures).  The gradient, every guard float and, without amsgrad, nothing else may change bits."""
    worst, bad = 0.0, []
    names = ("p", "m", "v") + (("vm",) if amsgrad else ())
    touched = {n: torch.zeros(before[n].numel(), dtype=torch.bool) for n in names}
    for i, (start, n) in enumerate(slices["p"]):
        sl = {k: before[k][slices[k][i][0]:slices[k][i][0] + n] for k in before}
        ref = adam_one(sl["p"], sl["g"], sl["m"], sl["v"], sl.get("vm"), sc, amsgrad)
        for j, name in enumerate(names):
            r = ratio(after[name][start:start + n], ref[j], ref[4][j])
            worst = max(worst, r)
            if not r <= 1.0:
                bad.append((name, n, r))
            touched[name][start:start + n] = True
    for name in names:
        keep = ~touched[name]
        if not torch.equal(after[name][keep].view(torch.int32), before[name][keep].view(torch.int32)):
            bad.append((name, "a guard float changed"))
    if not torch.equal(after["g"].view(torch.int32), before["g"].view(torch.int32)):
        bad.append(("g", "the gradient changed"))
    return worst, bad


def adam_emulate(before, slices, sc, amsgrad, mutate=None):
    """The launch in plain fp32 torch -> {name: flat buffer} like ``after`` of ``adam_check``"""
    after = {k: t.clone() for k, t in before.items()}
    for i, (start, n) in enumerate(slices["p"]):
        sl = {k: before[k][slices[k][i][0]:slices[k][i][0] + n] for k in before}
        out = adam_one(sl["p"], sl["g"], sl["m"], sl["v"], sl.get("vm"), sc, amsgrad, dt=torch.float32, mutate=mutate)
        for name, t in zip(("p", "m", "v", "vm"), out):
            if t is not None:
                after[name][start:start + n] = t
    return after
