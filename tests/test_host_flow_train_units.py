"""CPU-side checks of the unit tests of the cINN training kernels (tests/flow_train_units_common.py, tests/test_gpu_flow_train_units.py):
the ``saved`` layout accessor against an independent statement of the layout, the float64 emulation of the pass against autograd through
the oracle, every bound against a plain fp32 torch emulation of its unit (at most half of it is used), every deliberate error against
the gate, the sample rule of the end-to-end check, and the coverage of the case matrix.  No GPU: ``i2v_flow_train_saved_layout`` is a
host function."""
import ctypes
import os
import re

import pytest
import torch

import flow_train_units_common as tu
from conftest import REPO

GROUPS = ("hidden", "depth", "embed", "flags", "batch")
HALF = 0.5
_RES = {}


@pytest.fixture(scope="module", autouse=True)
def _no_grad():
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(prev)


def _lib():
    import i2v_native
    if not os.path.exists(i2v_native.LIB_PATH):
        i2v_native.build()
    lib = ctypes.CDLL(i2v_native.LIB_PATH)
    fn = lib.i2v_flow_train_saved_layout
    fn.restype, fn.argtypes = i2v_native.SYMBOLS["i2v_flow_train_saved_layout"]
    return i2v_native, fn


def _layout_by_the_comment(B, H, depth, E, nfl):
    """The layout comment of i2v_flow_train.hip, stated again: per half-step xs [B][64], cin [B][KP], act [2][depth + 1][B][H],
    out [2][B][32], dpre like act, dout like out; then xin and gan [nfl][B][64], part [B][64], dcin [B][KP]"""
    KP = -(-(32 + E) // 4) * 4
    sizes = [("xs", B * 64), ("o_cin", B * KP), ("o_act", 2 * (depth + 1) * B * H), ("o_out", 2 * B * 32), ("o_dpre", 2 * (depth + 1) * B * H),
             ("o_dout", 2 * B * 32)]
    L, off = {"KP": KP}, 0
    for name, n in sizes:
        L[name] = off
        off += n
    L["step_sz"] = off
    off *= 2 * nfl
    for name, n in (("o_xin", nfl * B * 64), ("o_gan", nfl * B * 64), ("o_part", B * 64), ("o_dcin", B * KP)):
        L[name] = off
        off += n
    L["total"] = off
    del L["xs"]
    return L


def test_saved_layout_accessor():
    native, fn = _lib()
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    assert "i2v_flow_train_saved_layout" in set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    assert [n for n, _ in native.FlowTrainLayout._fields_] == list(tu.LAYOUT_FIELDS)
    for c in tu.CASES:
        out = native.FlowTrainLayout()
        assert fn(c["hidden"], c["depth"], c["E"], tu.NFL, c["B"], ctypes.byref(out)) == 0, c["id"]
        L = {n: int(getattr(out, n)) for n in tu.LAYOUT_FIELDS}
        assert L == _layout_by_the_comment(c["B"], c["hidden"], c["depth"], c["E"], tu.NFL), c["id"]
        assert L["KP"] == tu.kp(c) and all(v % 4 == 0 for v in L.values()), (c["id"], L)
        spans = sorted((off, off + shape[0] * shape[1], name) for name, off, shape in tu.regions(c, c["B"], L))
        assert spans[0][0] == 0 and spans[-1][1] == L["total"], c["id"]
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (c["id"], "regions overlap or leave a gap")
    out = native.FlowTrainLayout()
    for bad in ((192, 2, 64, 2, 4), (640, 2, 64, 2, 4), (128, 0, 64, 2, 4), (128, 2, 129, 2, 4), (128, 2, 0, 2, 4), (128, 2, 64, 0, 4),
                (128, 2, 64, 2, 0)):
        assert fn(*bad, ctypes.byref(out)) != 0, bad
    assert fn(128, 2, 64, 2, 4, None) != 0


def test_case_ids_are_unique_and_the_matrix_covers_every_branch():
    assert len({c["id"] for c in tu.CASES}) == len(tu.CASES)
    first = {(tu.kin(c, st) % 16 == 0, "cond" if tu.cond(c, st) else "normal") for c in tu.CASES for st in range(tu.S)}
    assert first == {(True, "normal"), (False, "normal"), (True, "cond"), (False, "cond")}
    assert {1, 16, 125, 126, 127, 129} <= {tu.kin(c, st) for c in tu.CASES for st in range(tu.S)}
    ragged = {c["B"] for c in tu.CASES if any(tu.kin(c, st) % 16 for st in range(tu.S))}
    assert {1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130} <= ragged
    assert {c["hidden"] for c in tu.CASES} == {128, 256, 384, 512} and {c["depth"] for c in tu.CASES} == {1, 2, 3}
    assert {c["control"] for c in tu.CASES} == {0, 1, 2}
    assert {(c["skip_an"], c["skip_sh"], c["act"]) for c in tu.group("flags")} == set(tu.fu.FLAG_SETS) and len(tu.group("flags")) == 8
    assert {(c["hidden"], c["B"]) for c in tu.group("hidden")} == {(h, b) for h in (128, 256, 384, 512) for b in (17, 65)}
    assert {(c["E"], c["control"]) for c in tu.group("embed")} == {(e, k) for e in (1, 15, 16, 17, 93, 94, 95, 97, 128) for k in (0, 1, 2)}
    # dw_gemm: K < 64, K just above a 16 and a 64 column tile
    ks = {tu.kin(c, st) for c in tu.CASES for st in range(tu.S)}
    assert {1, 15, 17, 33, 49, 97, 129} <= ks, sorted(ks)
    assert set().union(*(tu.branches(c) for c in tu.CASES)) >= tu.LEDGER_WANT


def _result(c):
    """(worst ratio per unit kind of the fp32 emulation, failures, rel-L2 of the float64 emulation against autograd) of a case"""
    if c["id"] not in _RES:
        x, e, d_zt, d_ld, ref, own, draws = tu.reference(c)
        worst, bad = tu.check_units(tu.emulate(c, x, e, d_zt, d_ld), x, e, d_zt, d_ld)
        pin = tu.check_e2e(c, tu.emulate(c, x, e, d_zt, d_ld, torch.float64), ref)[0]
        _RES[c["id"]] = (worst, bad, max(pin.values()))
    return _RES[c["id"]]


@pytest.mark.parametrize("name", GROUPS)
def test_sample_rule_keeps_enough_and_the_reference_is_good_there(name):
    for c in tu.group(name):
        _, _, kept, drawn = tu.pool(c)
        assert 8 * kept >= drawn and kept >= 2 * c["B"], (c["id"], kept, drawn)
        for which in (0, 1):
            *_, own, draws = tu.reference(c, which)
            print(f"FLOWTRAINUNITS {c['id']} batch {which}: {kept} of {drawn} candidates kept, cotangent draw {draws}, the oracle's fp32 run {own:.2e}")
            assert own <= tu.OWN_FP32, (c["id"], which, own)


@pytest.mark.parametrize("name", GROUPS)
def test_fp32_emulation_uses_at_most_half_of_every_bound(name):
    worst = {}
    for c in tu.group(name):
        w, bad, pin = _result(c)
        assert not bad, (c["id"], bad[:5])
        assert pin <= 1e-12, (c["id"], "the float64 emulation is not autograd through the oracle", pin)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"FLOWTRAINUNITS cpu fp32 worst |err| / bound, group {name}:", {k: f"{v:.3f}" for k, v in sorted(worst.items())})
    assert set(worst) == {"linear", "dx", "dcin", "dw", "db", "actnorm", "fwd_link", "cin", "zt", "logdet", "bwd_link"} - \
        ({"actnorm"} if all(c["skip_an"] for c in tu.group(name)) else set())
    assert max(worst.values()) <= HALF, worst


def test_composed_oracle_is_flow_forward_where_both_apply():
    c = tu.group("batch")[4]
    assert tu.expressible(c)
    x, e, d_zt, d_ld = tu.inputs(c)
    a, b = tu.autograd_ref(c, x, e, d_zt, d_ld, composed=False), tu.autograd_ref(c, x, e, d_zt, d_ld, composed=True)
    assert torch.equal(a[0], b[0]) and tu.fc.rel(b[1], a[1]) <= 1e-14 and set(a[2]) == set(b[2])    # the log-det terms add in another order
    assert all(tu.fc.rel(b[2][k], a[2][k]) <= 1e-14 for k in a[2])
    assert torch.equal(tu.margins(c, x, e, composed=False), tu.margins(c, x, e, composed=True))


MUTATION_CASES = ("hidden-h128-d2-e64-c0-b17", "embed-h128-d2-e94-c1-b17", "embed-h128-d2-e97-c2-b17", "batch-h128-d2-e94-c1-b65",
                  "flags-h128-d2-e64-c0-b17-nosh-noact")
NEEDS = {"dw_ragged_block0": lambda c: any(tu.kin(c, st) > 64 and tu.kin(c, st) % 64 for st in range(tu.S)),
         "dscale_no_dlogdet": lambda c: not c["skip_an"], "cond_offset_32": lambda c: c["control"] != 0}


@pytest.mark.parametrize("mutation", [m for m in tu.MUTATIONS if m not in tu.ADAM_MUTATIONS])
def test_every_pass_mutation_fails_the_gate(mutation):
    """The factor over the gate (unit: |err| / bound; end to end: rel-L2 / 1e-4) of the error on every case it applies to"""
    hit = []
    for c in (c for c in tu.CASES if c["id"] in MUTATION_CASES):
        if not NEEDS.get(mutation, lambda c: True)(c):
            continue
        x, e, d_zt, d_ld, ref, _, _ = tu.reference(c)
        if mutation == "accumulate_overwrites":
            x2, e2, d_zt2, d_ld2 = tu.inputs(c, 1)
            r1, r2 = tu.emulate(c, x, e, d_zt, d_ld), tu.emulate(c, x2, e2, d_zt2, d_ld2)
            good = tu.check_accumulate(r1, r2, {k: r1.grads[k] + r2.grads[k] for k in r1.grads}, d_ld, d_ld2)
            assert not good[1] and good[0] <= HALF, (c["id"], good)
            factor = tu.check_accumulate(r1, r2, r2.grads, d_ld, d_ld2)[0]
        else:
            run = tu.emulate(c, x, e, d_zt, d_ld, mutate=mutation)
            factor = max(max(tu.check_units(run, x, e, d_zt, d_ld)[0].values()), max(tu.check_e2e(c, run, ref)[0].values()) / tu.TOL_L2)
        print(f"FLOWTRAINUNITS mutation {mutation} on {c['id']}: {factor:.3g} x the gate")
        assert factor >= 2.0, (mutation, c["id"], factor)
        hit.append(c["id"])
    assert hit, mutation


ADAM_LAYOUTS = {"aligned": (0, 0), "param_off_4_bytes": (1, 0), "grad_off_4_bytes": (0, 1)}


def _adam_steps(amsgrad, wd):
    return [(step, tu.adam_scalars(step, wd, **tu.ADAM_HYPER)) for step in tu.ADAM_STEPS]


@pytest.mark.parametrize("layout", list(ADAM_LAYOUTS))
def test_adam_bound_holds_twice_over_for_fp32_torch(layout):
    for sp, sg in ((0, 0), (1, 0), (0, 1)):
        slices = tu.adam_slices(sp)[0]
        assert all(s % 4 == sp for s, _ in slices) and all(b[0] - (a[0] + a[1]) >= 1 for a, b in zip(slices, slices[1:]))
    worst = 0.0
    for amsgrad in (False, True):
        for wd in (0.0, 1e-2):
            state, slices = tu.adam_state(*ADAM_LAYOUTS[layout])
            if not amsgrad:
                del state["vm"]
            for step, sc in _adam_steps(amsgrad, wd):
                after = tu.adam_emulate(state, slices, sc, amsgrad)
                r, bad = tu.adam_check(state, after, slices, sc, amsgrad)
                assert not bad, (layout, amsgrad, wd, step, bad[:4])
                worst, state = max(worst, r), after
    print(f"FLOWTRAINUNITS cpu fp32 adam worst |err| / bound, {layout}: {worst:.3f}")
    assert worst <= HALF


@pytest.mark.parametrize("mutation", tu.ADAM_MUTATIONS)
def test_every_adam_mutation_fails_the_gate(mutation):
    factors = []
    for wd in (0.0, 1e-2):
        state, slices = tu.adam_state(1, 0)
        for step, sc in _adam_steps(True, wd):
            used = tu.adam_scalars(step + 1, wd, **tu.ADAM_HYPER) if mutation == "adam_bc2_wrong_step" else sc
            after = tu.adam_emulate(state, slices, used, True, mutate=mutation)
            factors.append(tu.adam_check(state, after, slices, sc, True)[0])
            state = tu.adam_emulate(state, slices, sc, True)
    print(f"FLOWTRAINUNITS mutation {mutation}: {min(factors):.3g} .. {max(factors):.3g} x the gate over the launches")
    assert max(factors) >= 2.0 and (mutation != "adam_tail_not_updated" or min(factors) >= 2.0), factors
