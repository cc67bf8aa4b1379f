"""Shared by tests/test_host_flow_units.py and tests/test_gpu_flow_units.py: a plain torch float64 oracle of a short ``ConditionalFlow``
that carries a forward error bound next to every value, the deliberate errors (``MUTATIONS``) that show what the gate catches, the gate,
the seeded weights and inputs, and the case matrix of the cINN chain kernels (csrc/i2v_flow_tile.hip, the generic chain of
csrc/i2v_flow.hip).

The oracle is written from the layer definitions (a block is ActNorm -> InvLeakyRelu -> two coupling half-steps -> Shuffle, reversed in
the other direction; an s- / t-net is Linear -> LeakyReLU(0.01) x (depth + 1) -> Linear) and takes the switches the native handle takes:
``skip_actnorm``, ``skip_shuffle``, ``activation`` and ``control`` in {0, 1, 2} (1: blocks with fl % 4 != 0 are mode 'cond', 2: every
block).  It is pinned to oracle/flow_ref in float64 and to tests/golden/flow_units.npz by tests/test_host_flow_units.py.

Error bound.  Every value v carries d >= 0 with |fp32 evaluation - v| <= d, computed from float64 quantities alone (never from an output of
the code under test), u = 2^-24, gamma(n) = n u / (1 - n u) (i3d_units_common):

* Linear with K stored inputs and a bias: dy = |W| dx + gamma(K + 2) (|W| |x| + |b|) -- the dot-product bound of ANY summation order
  (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5), so it covers the first layer split into the state part and the
  embedding part computed ahead, the K split over waves and the partial tiles of the last Linear.  K is the length as stored: 32 +
  16 ceil(E / 16) for a 'normal' first layer, 16 ceil(E / 16) for 'cond', the hidden width elsewhere.
* LeakyReLU(0.01), InvLeakyRelu (x 0.9 forward, / 0.9 reverse): d is multiplied by the op's Lipschitz factor ON THE INTERVAL [v - d, v + d]
  (the slope of the side when the interval stays on one side of 0, else the larger of the two, which is valid across the kink), plus 2 u |result|
  on the scaled side: the fp32 constant (0.01f, 0.9f) is not the float64 one, and the product is rounded.
* ActNorm forward scale (x + loc): d = |scale| (dx + u |x + loc|) + u |result|; reverse x / scale - loc: d = dx / |scale| + u |x / scale| + u |result|.
* Shuffle and the half swap: exact.
* Coupling forward fma(x, expf(s), t): d = e^s dx + |x| e^s ds + dt + C_EXP u |x| e^s + u |result|; reverse (x - t) expf(-s):
  d = e^-s (dx + dt + u |x - t|) + |x - t| e^-s ds + (C_EXP + 1) u |result|.  C_EXP = 2: no document or header of the installed HIP / device
  library states an ulp figure for the device expf (searched: the HIP headers, the packaged documentation, the device-library
  package), so the fallback of 2 ulp is used.
* Log-det: d = sum ds over the summed channels + gamma(n) sum |term| for the n terms added (32 s per half-step, one constant per ActNorm)
  + u |constant| per ActNorm (the constant is summed in double on the host and rounded once).

fp16-operand mode (``f16=True``): the oracle emulates the operand rounding -- weights rounded to fp16 once from the fp32 values (the same
on both sides: no error), every activation rounded to fp16 (round to nearest even, done here in float64 arithmetic) before each Linear.
At such a rounding an element whose float64 value lies within its incoming d of a rounding midpoint may round the other way in an fp32
evaluation: d grows there by ulp16 (taken at |v| + d); every other element rounds to the same fp16 number on both sides or moves with
its d, and d grows by nothing.  (Midpoints tested: those of v's own binade and, just above a power of two, the one below it.)

Weights and inputs (``state_dict``, ``candidates``) are chosen so that the gate can see a wrong GEMM: the bound of a Linear is relative
to |W| |x| + |b|, so the sums are kept free of cancellation -- one sign per output row, positive embeddings, biases scaled with their
weights -- and every value stays comparable to what its bound is relative to.  tests/test_host_flow_units.py shows that a lost
k-block, output row or wave partial of one Linear fails the gate at every hidden width in both precisions.

The bound is first-order, so it holds on the smooth side of a LeakyReLU / InvLeakyRelu only: ``pool`` keeps the samples of which no
such input is within its own d of 0, in the exact-mode oracle and in the fp16-mode oracle (other values, larger d).  Should an
interval [v - d, v + d] reach across 0 all the same, d is propagated with the larger of the two slopes, which is valid there too.

Gate: element-wise |got - ref64| <= d + u |ref64| on z~, z and the log-det, and, in exact fp32 mode, rel-L2 <= 1e-4 per sample row."""
import itertools

import numpy as np
import torch

import i2v_synth as synth
from i3d_units_common import TOL_L2, U, gamma

C_EXP = 2.0
SLOPE, ALPHA = 0.01, 0.9
NFL = 2

# deliberate errors -> where they apply (d: "fwd" | "rev" | "both"; needs: a property of the case)
MUTATIONS = {
    "drop_last_embed": dict(d="both"),                       # embedding element E - 1 dropped from the first Linear
    "last_sample_embed": dict(d="both", needs="B2"),         # sample B - 1 reads sample B - 2's embedding
    "logdet_missing_channel": dict(d="fwd"),                 # one channel's s missing from the log-det
    "logdet_missing_actnorm": dict(d="fwd", needs="an"),     # ActNorm log-det missing from one block
    "shuffle_swapped": dict(d="both", needs="shuffle"),      # forward and backward shuffle indices exchanged
    "inv_lrelu_wrong_sign": dict(d="both", needs="act"),     # InvLeakyRelu applied to the wrong sign
    "lrelu_slope_zero": dict(d="both"),                      # LeakyReLU slope 0.01 -> 0
    "cond_fed_state": dict(d="both", needs="cond"),          # 'cond' block fed the state channels
    "reverse_t_first": dict(d="rev"),                        # t added before the scaling in reverse: x e^-s - t
    "f16_unrounded": dict(d="both", needs="f16"),            # one fp16 activation (the input of one Linear) left unrounded
    # what a wrong GEMM of the chain kernels would do (WEIGHT_MUTATIONS: done on the weights)
    "drop_k_block": dict(d="both", needs="hid"),             # one 16-wide k-block (columns 16 .. 31) of one hidden Linear dropped
    "drop_hidden_row": dict(d="both", needs="hid"),          # one output row of one hidden Linear dropped
    "drop_last_partial": dict(d="both"),                     # one wave's partial tile of the last Linear dropped
}


def mutate_weights(sd, name, case):
    """The WEIGHT_MUTATIONS on an oracle's (float64 torch) weights.
    drop_k_block: columns 16 .. 31 of the first hidden Linear of the s-net of half-step 1 of block 1.
    drop_hidden_row: weights and bias of one output row of the first hidden Linear of the t-net of half-step 0 of block 0, the first
    row of positive sign.  (A row of negative sign reaches the next Linear through the 0.01 side of the LeakyReLU: losing it moves
    that Linear's outputs by 1 % of one term in ``hidden``, which no bound of a ``hidden``-term fp32 sum can separate from rounding.)
    drop_last_partial: the last Linear of the s-net of half-step 0 of block 1, output rows 16 .. 31, the upper half of K -- the
    partial tile one wave of the tile chain contributes."""
    H, D = case["hidden"], case["depth"]
    sd = dict(sd)
    if name == "drop_k_block":
        k = "sub_layers.1.coupling.s.1.main.2.weight"
        w = sd[k].clone()
        w[:, 16:32] = 0
        sd[k] = w
    elif name == "drop_hidden_row":
        k = "sub_layers.0.coupling.t.0.main.2."
        w, b = sd[k + "weight"].clone(), sd[k + "bias"].clone()
        r = int((w.sum(1) > 0).nonzero()[0])
        w[r], b[r] = 0, 0
        sd[k + "weight"], sd[k + "bias"] = w, b
    elif name == "drop_last_partial":
        k = f"sub_layers.1.coupling.s.0.main.{2 * (D + 1)}.weight"
        w = sd[k].clone()
        w[16:32, H // 2:] = 0
        sd[k] = w
    return sd


WEIGHT_MUTATIONS = ("drop_k_block", "drop_hidden_row", "drop_last_partial")


def mutation_applies(name, case, f16, reverse, B):
    m = MUTATIONS[name]
    if m["d"] == ("fwd" if reverse else "rev"):
        return False
    return {None: True, "B2": B >= 2, "an": not case["skip_an"], "shuffle": not case["skip_sh"], "act": case["act"] == "lrelu",
            "cond": case["control"] != 0, "f16": f16, "hid": case["depth"] >= 1}[m.get("needs")]


# ---------------------------------------------------------------------------------------------------------------- weights, inputs

_SD = {}
ROW_SUM = dict(first_e=3.0, first_x=0.5, hidden=4.0, t=0.1, s=0.05)   # the largest row sum of |W| of each kind of Linear (state_dict)
ACTIVE = 0.25                                                         # the share of positive output rows of a first or hidden Linear


def block_cond(control, fl):
    return control == 2 or (control == 1 and fl % 4 != 0)


def state_dict(case):
    """The seeded synthetic state_dict (numpy, fp32) of a case's geometry.  control 2: every first layer sees the embedding alone."""
    key = (case["hidden"], case["depth"], case["E"], case["control"], case.get("sparse", False))
    if key not in _SD:
        H, D, E, control = key[:4]
        sd = synth.flow_state_dict(seed=100 + H // 64 + 10 * D + 1000 * control + 7 * E, n_flows=NFL, embedding_dim=E, hidden_dim=H, hidden_depth=D,
                                   control=control == 1)
        if control == 2:
            sd = {k: (np.ascontiguousarray(v[:, 32:]) if k.endswith("main.0.weight") else v) for k, v in sd.items()}
        # The bound of a Linear is relative to |W| |x| + |b| and travels on through |W|, whatever the signs.  With the synthesiser's random
        # signs the value itself is a sum that cancels to about |W| |x| / sqrt(K) in EVERY layer, so after a few layers the bound is
        # orders above the signal and a wrong GEMM hides in it.  So the signs are made coherent: every hidden and last Linear keeps
        # the synthesiser's magnitudes and gives a whole output row one sign, drawn from a seeded stream.  Its inputs are LeakyReLU
        # outputs, where the positive ones carry the sum, so W x = +- |W| |x| up to the few % the negative side adds: the value stays comparable to what the bound is relative to, and a
        # lost k-block, row or partial sum moves the output by its share of the sum, far above the bound.  In the first Linear the
        # embedding columns are made coherent in the same way (the embeddings of ``candidates`` are positive) and carry the sum; the
        # state columns keep their random signs, as the state has them too, at a smaller weight.
        # ACTIVE = a quarter of the rows of a first or hidden Linear are positive, so one input of the next Linear in four carries
        # its sum and a single lost row is 1 / (hidden / 4) of it; s and t come out in both signs half and half.
        # Scale (ROW_SUM, the largest row sum of |W|): 4 for the hidden Linears (with a quarter of the inputs active the magnitudes
        # and d neither grow nor shrink from layer to layer), 3 + 0.5 for the embedding and state columns of the first, 0.1 for the
        # t-net's last and 0.05 for the s-net's last: the synthesiser's own gain (row sums of 5 .. 20) would grow d by that factor per
        # layer, 16 layers deep, and in fp16 mode every operand rounding about triples d (an element is charged one ulp16 with
        # probability 2 d / ulp16), so s and t are kept small next to the state, whose d then stays far under half an ulp16.  Each
        # bias is scaled with its weight, so no activation is dominated by its bias.
        last = 2 * (D + 1)
        rng = np.random.default_rng(9000 + H + D)
        for k, v in list(sd.items()):
            if k.endswith(".weight") and "coupling" in k:
                li = int(k.split("main.")[1].split(".")[0])
                w = v.astype(np.float64)
                sign = np.where(rng.uniform(size=(w.shape[0], 1)) < (0.5 if li == last else ACTIVE), 1.0, -1.0)
                if li == 0:
                    ns = w.shape[1] - E                      # the state columns come first: 32 of them, or none in a 'cond' block
                    we = np.abs(w[:, ns:]) * sign
                    f = ROW_SUM["first_e"] / np.abs(we).sum(1).max()
                    ws = w[:, :ns] * (ROW_SUM["first_x"] / np.abs(w[:, :ns]).sum(1).max()) if ns else w[:, :0]
                    w = np.concatenate((ws, we * f), 1)
                else:
                    target = ROW_SUM["s" if ".s." in k else "t"] if li == last else ROW_SUM["hidden"]
                    w = np.abs(w) * sign
                    f = target / np.abs(w).sum(1).max()
                    w = w * f
                sd[k] = w.astype(np.float32)
                kb = k[:-len("weight")] + "bias"
                sd[kb] = (sd[kb].astype(np.float64) * f).astype(np.float32)
        if key[4]:
            # hidden and last Linear layers with ONE weight per row (column (5 row + 3) mod K): every output follows one chain of
            # elements, so the bound of an output holds few terms and a single operand rounding shows in it
            for k, v in list(sd.items()):
                if k.endswith(".weight") and "coupling" in k and not k.endswith("main.0.weight"):
                    w = np.zeros_like(v)
                    rows = np.arange(v.shape[0])
                    cols = (5 * rows + 3) % v.shape[1]
                    w[rows, cols] = np.sign(v[rows, cols]) * (0.75 + np.abs(v[rows, cols]))
                    sd[k] = w
        _SD[key] = sd
    return _SD[key]


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def candidates(case, n):
    """n candidate samples (x [n, 64] normal, e [n, E] half-normal: positive, see ``state_dict``; fp32) of one seeded stream per geometry"""
    g = torch.Generator().manual_seed(50000 + 13 * case["hidden"] + 101 * case["E"] + case["depth"] + 7 * case["control"])
    return torch.randn(n, 64, generator=g), torch.randn(n, case["E"], generator=g).abs()


# ---------------------------------------------------------------------------------------------------------------- fp16 rounding

def ulp16(v):
    """The spacing of fp16 numbers at |v| (float64 tensor), 2^-24 in the subnormal range"""
    _, ex = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), (ex - 1).clamp_min(-14) - 10)


def round16(v, d):
    """(v rounded to the nearest fp16 number, ties to even; d grown by ulp16 where a rounding midpoint lies within d of v)"""
    ulp = ulp16(v)
    q = v / ulp
    r = torch.round(q) * ulp
    assert float(r.abs().max()) <= 65504.0
    to_mid = ((q - torch.floor(q)) - 0.5).abs() * ulp
    # just above a power of two the nearest midpoint lies BELOW it, in the finer binade: at 2^k - ulp / 4 (no finer binade under 2^-14)
    _, ex = torch.frexp(v)
    low = torch.ldexp(torch.ones_like(v), ex - 1)
    to_mid = torch.where(ex - 1 > -14, torch.minimum(to_mid, v.abs() - low + ulp / 4), to_mid)
    return r, d + torch.where(to_mid <= d, ulp16(v.abs() + d), torch.zeros_like(d))


# ---------------------------------------------------------------------------------------------------------------- the oracle

class Oracle:
    """One run: ``Oracle(case, B, f16, reverse, mutate).run(x, e)`` -> self.z, self.dz ([B, 64] value and bound), self.ld, self.dld
    (forward), self.margin [B]: the smallest |v| - d over every LeakyReLU / InvLeakyRelu input of a sample (> 0: no input of that sample is
    within its own d of a kink)."""

    def __init__(self, case, f16=False, reverse=False, mutate=None, sd=None, blocks=None):
        """``sd``: another state_dict (numpy) than the case's own; ``blocks``: the block indices to run (default: all NFL)"""
        self.c, self.f16, self.reverse, self.mutate = case, bool(f16), bool(reverse), mutate
        self.blocks = list(range(NFL) if blocks is None else blocks)
        sd = state_dict(case) if sd is None else sd
        self.sd = {k: (torch.from_numpy(v).double() if v.dtype == np.float32 else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}
        if self.f16:   # weights: rounded to fp16 once, from the fp32 values
            self.sd = {k: (round16(v, torch.zeros_like(v))[0] if k.endswith(".weight") and "coupling" in k else v) for k, v in self.sd.items()}
        if mutate in WEIGHT_MUTATIONS:
            self.sd = mutate_weights(self.sd, mutate, case)

    # -- leaves
    def _kink(self, v, d):
        m = (v.abs() - d).reshape(v.shape[0], -1).min(1).values
        self.margin = torch.minimum(self.margin, m)

    def _scaled(self, v, d, pos, neg, wrong_sign=False):
        """v * pos where v >= 0, v * neg where v < 0, with the interval Lipschitz factor and 2 u |result| where the factor is not 1"""
        self._kink(v, d)
        side = (v < 0) if wrong_sign else (v >= 0)
        f = torch.where(side, torch.full_like(v, pos), torch.full_like(v, neg))
        crossing = v.abs() <= d
        lip = torch.where(crossing, torch.full_like(v, max(abs(pos), abs(neg))), f.abs())
        out = v * f
        return out, lip * d + torch.where(f != 1.0, 2 * U * out.abs(), torch.zeros_like(d))

    def linear(self, v, d, W, b, K, rounded=True):
        if self.f16 and rounded:
            v, d = round16(v, d)
        Wa = W.abs()
        y = v @ W.T + b
        return y, d @ Wa.T + gamma(K + 2) * (v.abs() @ Wa.T + b.abs())

    def mlp(self, prefix, v, d, K0, unrounded_layer=None):
        D, H = self.c["depth"], self.c["hidden"]
        slope = 0.0 if self.mutate == "lrelu_slope_zero" else SLOPE
        for li in range(D + 2):
            W, b = self.sd[f"{prefix}main.{2 * li}.weight"], self.sd[f"{prefix}main.{2 * li}.bias"]
            v, d = self.linear(v, d, W, b, K0 if li == 0 else H, rounded=li != unrounded_layer)
            if li < D + 1:
                v, d = self._scaled(v, d, 1.0, slope)
        return v, d

    def nets(self, fl, i, keep, dkeep, e):
        """s, ds, t, dt of half-step i of block fl from the passive half and the embedding"""
        E = self.c["E"]
        cond = block_cond(self.c["control"], fl)
        K0 = (0 if cond else 32) + 16 * ((E + 15) // 16)
        e = e.clone()
        if self.mutate == "drop_last_embed":
            e[:, E - 1] = 0
        if self.mutate == "last_sample_embed":
            e[-1] = e[-2]
        de = torch.zeros_like(e)
        if cond and self.mutate == "cond_fed_state":
            full = torch.cat((keep, e), 1)
            cin, dcin = full[:, :E], torch.cat((dkeep, de), 1)[:, :E]
        elif cond:
            cin, dcin = e, de
        else:
            cin, dcin = torch.cat((keep, e), 1), torch.cat((dkeep, de), 1)
        # the fp16 mutation: the input of the first Linear of the s-net of the LAST half-step of the pass is left unrounded
        last = (fl, i) == ((0, 0) if self.reverse else (NFL - 1, 1))
        un = 0 if (self.mutate == "f16_unrounded" and last) else None
        p = f"sub_layers.{fl}.coupling."
        s, ds = self.mlp(f"{p}s.{i}.", cin, dcin, K0, un)
        t, dt = self.mlp(f"{p}t.{i}.", cin, dcin, K0)
        return s, ds, t, dt

    @staticmethod
    def _swap(v):
        return torch.cat((v[:, 32:], v[:, :32]), 1)

    def run(self, x, e):
        c, sd = self.c, self.sd
        v, e = x.double().reshape(x.shape[0], 64), e.double()
        d = torch.zeros_like(v)
        B = v.shape[0]
        self.margin = torch.full((B,), float("inf"), dtype=torch.float64)
        ld, dld, ld_abs, n_ld = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), 0
        use_an, use_sh, use_act = not c["skip_an"], not c["skip_sh"], c["act"] == "lrelu"
        wrong = self.mutate == "inv_lrelu_wrong_sign"
        for fl in (reversed(self.blocks) if self.reverse else self.blocks):
            p = f"sub_layers.{fl}."
            scale, loc = (sd[p + "norm_layer." + n].reshape(1, 64) for n in ("scale", "loc"))
            fwd_idx, bwd_idx = sd[p + "shuffle.forward_shuffle_idx"], sd[p + "shuffle.backward_shuffle_idx"]
            if self.mutate == "shuffle_swapped":
                fwd_idx, bwd_idx = bwd_idx, fwd_idx
            if not self.reverse:
                if use_an:
                    a = v + loc
                    v, d = scale * a, scale.abs() * (d + U * a.abs())
                    d = d + U * v.abs()
                    if not (self.mutate == "logdet_missing_actnorm" and fl == NFL - 1):
                        k = float(torch.log(scale.abs()).sum())
                        ld, dld, ld_abs, n_ld = ld + k, dld + U * abs(k), ld_abs + abs(k), n_ld + 1
                if use_act:
                    v, d = self._scaled(v, d, 1.0, ALPHA, wrong)
                for i in range(2):
                    if i == 1:
                        v, d = self._swap(v), self._swap(d)
                    s, ds, t, dt = self.nets(fl, i, v[:, :32], d[:, :32], e)
                    xa, dxa = v[:, 32:], d[:, 32:]
                    es = torch.exp(s)
                    y = xa * es + t
                    dy = es * dxa + xa.abs() * es * ds + dt + C_EXP * U * xa.abs() * es + U * y.abs()
                    v, d = torch.cat((v[:, :32], y), 1), torch.cat((d[:, :32], dy), 1)
                    sl = s[:, :31] if (self.mutate == "logdet_missing_channel" and (fl, i) == (NFL - 1, 1)) else s
                    ld, dld, ld_abs, n_ld = ld + sl.sum(1), dld + ds.sum(1), ld_abs + s.abs().sum(1), n_ld + 32
                if use_sh:
                    v, d = v[:, fwd_idx], d[:, fwd_idx]
            else:
                if use_sh:
                    v, d = v[:, bwd_idx], d[:, bwd_idx]
                for i in (1, 0):
                    s, ds, t, dt = self.nets(fl, i, v[:, :32], d[:, :32], e)
                    xa, dxa = v[:, 32:], d[:, 32:]
                    ens = torch.exp(-s)
                    if self.mutate == "reverse_t_first":
                        y = xa * ens - t
                        dy = torch.zeros_like(y)
                    else:
                        diff = xa - t
                        y = diff * ens
                        dy = ens * (dxa + dt + U * diff.abs()) + diff.abs() * ens * ds + (C_EXP + 1) * U * y.abs()
                    v, d = torch.cat((v[:, :32], y), 1), torch.cat((d[:, :32], dy), 1)
                    if i == 1:
                        v, d = self._swap(v), self._swap(d)
                if use_act:
                    v, d = self._scaled(v, d, 1.0, 1.0 / ALPHA, wrong)
                if use_an:
                    a = v / scale
                    v, d = a - loc, d / scale.abs() + U * a.abs()
                    d = d + U * v.abs()
        self.z, self.dz = v, d
        self.ld, self.dld = ld, dld + gamma(max(n_ld, 1)) * ld_abs
        return self


_ORACLES = {}


def oracle(case, B, f16, reverse, mutate=None):
    """The (cached) oracle run of a case's geometry at batch B on the first B samples of its pool"""
    key = (geometry_key(case), B, bool(f16), bool(reverse), mutate)
    if key not in _ORACLES:
        x, e = inputs(case, B, reverse)
        _ORACLES[key] = Oracle(case, f16, reverse, mutate).run(x, e)
    return _ORACLES[key]


def geometry_key(case):
    return (case["hidden"], case["depth"], case["E"], case["control"], case["skip_an"], case["skip_sh"], case["act"], case.get("sparse", False))


# ---------------------------------------------------------------------------------------------------------------- inputs without kinks

_POOLS = {}
POOL_FACTOR = 2     # candidates drawn per sample needed: at least half must qualify


def pool(case, reverse):
    """The samples of a geometry and direction: 2 Bmax candidates from one seeded stream, kept when, in the oracle of that direction
    in BOTH modes (exact fp32, and fp16 operands with its own values and its larger d), every LeakyReLU / InvLeakyRelu input is
    further from 0 than its own bound d.  The rule looks at the float64 oracle alone.  Returns (x, e, kept, drawn)."""
    key = (geometry_key(case), bool(reverse))
    if key not in _POOLS:
        n = POOL_FACTOR * case["Bmax"]
        x, e = candidates(case, n)
        margin = torch.minimum(Oracle(case, False, reverse).run(x, e).margin, Oracle(case, True, reverse).run(x, e).margin)
        keep = (margin > 0).nonzero().flatten()
        _POOLS[key] = (x[keep].contiguous(), e[keep].contiguous(), int(len(keep)), n)
    return _POOLS[key]


def inputs(case, B, reverse):
    x, e, kept, drawn = pool(case, reverse)
    assert kept >= case["Bmax"] >= B, (case["id"], kept, drawn)
    return x[:B].contiguous(), e[:B].contiguous()


# ---------------------------------------------------------------------------------------------------------------- the fp32 reference

def reference_fp32(case, x, e, f16, reverse):
    """oracle/flow_ref in plain fp32 torch on the CPU (under ``linear_f16_emulation()`` in fp16 mode), composed from its leaf functions
    in the order the switches select -> (z, logdet or None)"""
    from oracle import flow_ref
    sd = tensors(state_dict(case))
    h, e = x.float().reshape(x.shape[0], 64), e.float()
    ld = torch.zeros(h.shape[0])
    with flow_ref.linear_f16_emulation(f16):
        for fl in (reversed(range(NFL)) if reverse else range(NFL)):
            p = f"sub_layers.{fl}."
            mode = "cond" if block_cond(case["control"], fl) else "normal"
            if not reverse:
                if not case["skip_an"]:
                    h, l = flow_ref.actnorm_forward(sd, p + "norm_layer.", h)
                    ld = ld + l
                if case["act"] == "lrelu":
                    h = flow_ref.inv_lrelu_forward(h)
                h, l = flow_ref.coupling_forward(sd, p + "coupling.", h, e, mode, case["depth"])
                ld = ld + l
                if not case["skip_sh"]:
                    h = h[:, sd[p + "shuffle.forward_shuffle_idx"]]
            else:
                if not case["skip_sh"]:
                    h = h[:, sd[p + "shuffle.backward_shuffle_idx"]]
                h = flow_ref.coupling_reverse(sd, p + "coupling.", h, e, mode, case["depth"])
                if case["act"] == "lrelu":
                    h = flow_ref.inv_lrelu_reverse(h)
                if not case["skip_an"]:
                    h = flow_ref.actnorm_reverse(sd, p + "norm_layer.", h)
    return h, (None if reverse else ld)


# ---------------------------------------------------------------------------------------------------------------- the gate

def rel_l2_rows(got, ref):
    got, ref = got.double().reshape(got.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    return (got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)


def gate(o, z, ld, f16):
    """(passes, worst |err| / bound over z and the log-det, worst rel-L2 of a row) of an output against an Oracle run: every element of z
    (z~ forward, z reverse) and of the log-det (forward; ``ld`` None in reverse) within d + u |ref|; exact mode: rel-L2 <= 1e-4 per row."""
    if tuple(z.shape) != tuple(o.z.shape) or (ld is not None and tuple(ld.shape) != tuple(o.ld.shape)):
        return False, float("inf"), float("inf")
    ok = bool(torch.isfinite(z).all())
    ratio = float(((z.double() - o.z).abs() / (o.dz + U * o.z.abs()).clamp_min(1e-300)).max())
    l2 = float(rel_l2_rows(z, o.z).max())
    if not o.reverse:
        assert ld is not None
        ok = ok and bool(torch.isfinite(ld).all())
        ratio = max(ratio, float(((ld.double() - o.ld).abs() / (o.dld + U * o.ld.abs()).clamp_min(1e-300)).max()))
    return ok and ratio <= 1.0 and (f16 or l2 <= TOL_L2), ratio, l2


# ---------------------------------------------------------------------------------------------------------------- the case matrix

FLAG_SETS = list(itertools.product((False, True), (False, True), ("lrelu", "none")))   # skip_actnorm, skip_shuffle, activation
NS_FOLD = ((1, 1), (1, 0), (2, 1), (2, 0), (4, 1), (4, 0))
NS_BATCHES = {1: (1, 17), 2: (35,), 4: (147,)}     # 35: the last group holds one tile; 147: three groups, the last with two tiles, the last tile with 3 samples
GENERIC_BATCHES = (1, 63, 64, 65, 130)


def _case(group, hidden, depth, E, control=0, flags=(False, False, "lrelu"), chain="tile", ns=None, fold=None, batches=(17,), precisions=(0, 1),
          sparse=False):
    c = dict(group=group, hidden=hidden, depth=depth, E=E, control=control, skip_an=flags[0], skip_sh=flags[1], act=flags[2], chain=chain,
             ns=ns, fold=fold, batches=tuple(batches), precisions=tuple(precisions), sparse=sparse)
    c["id"] = (f"{group}-h{hidden}-d{depth}-e{E}-c{control}" + ("-noan" if flags[0] else "") + ("-nosh" if flags[1] else "") +
               ("-noact" if flags[2] != "lrelu" else "") + (f"-ns{ns}" if ns else "") + ("" if fold is None else f"-fold{fold}") +
               ("-sparse" if sparse else "") + ("-generic" if chain == "generic" else "") + ("-auto" if chain == "auto" else ""))
    return c


def cases():
    """Every case of the GPU test.  ``chain``: "tile" (the default chain; ns / fold None: the launcher's own rule), "generic"
    (I2V_FLOW_TILE=0) or "auto" (no switch; the geometry is outside the tile chain's, so the handle must report the generic chain).
    ``precisions``: linear_f16 values the case runs in."""
    out = []
    for hidden in (128, 256, 384, 512):                                      # the full instantiation matrix
        for ns, fold in NS_FOLD:
            out.append(_case("matrix", hidden, 2, 64, ns=ns, fold=fold, batches=NS_BATCHES[ns]))
    out.append(_case("edges", 128, 2, 64, batches=(64, 65, 128, 129)))       # the default rule on both sides of NST = 4 / 5 and 8 / 9
    for hidden in (128, 384):
        for depth in (1, 3):
            out.append(_case("depth", hidden, depth, 64, batches=(17, 35)))
    for E in (1, 15, 16, 17, 94, 128):
        for control in (0, 1, 2):
            out.append(_case("embed", 128, 2, E, control, batches=(17,)))
    for flags in FLAG_SETS:
        out.append(_case("flags", 128, 2, 64, flags=flags, batches=(17,), precisions=(1,)))
    out.append(_case("sparse", 128, 1, 16, 2, batches=(17,), sparse=True))   # one weight per row: a single operand rounding shows
    # E and control move with hidden index + depth, so every depth meets every E, and every (E, control) pair occurs
    for hi, hidden in enumerate((64, 192, 320, 448, 512)):
        for depth in (0, 1, 2):
            out.append(_case("generic", hidden, depth, (1, 17, 94)[(hi + depth) % 3], (0, 2)[(hi + depth) % 2], chain="generic",
                             batches=GENERIC_BATCHES, precisions=(0,)))
    for n, (hidden, depth) in enumerate(((64, 1), (192, 2), (128, 0))):
        out.append(_case("generic", hidden, depth, (17, 1, 94)[n], (2, 0, 2)[n], chain="auto", batches=GENERIC_BATCHES, precisions=(0,)))
    bmax = {}
    for c in out:
        k = geometry_key(c)
        bmax[k] = max(bmax.get(k, 0), max(c["batches"]))
    for c in out:
        c["Bmax"] = bmax[geometry_key(c)]
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = cases()


def runs(case):
    """(B, f16, reverse) of every pass a case makes"""
    return [(B, bool(f), r) for f in case["precisions"] for B in case["batches"] for r in (False, True)]
