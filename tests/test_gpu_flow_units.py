"""Every cINN chain kernel variant against float64 at a derived bound: the 48 instantiations of the tile chain's hidden-layer launch
({hidden, folded first} x fp32 / fp16 operands x KPW 1..4 x NS 1 / 2 / 4), its unfolded tail kernel and its pre-GEMM at ragged embedding
widths, and the generic chain at every hidden width class and depth 0..2, on short flows (two blocks: one block boundary and both ends of
the pass), forward with log-det and reverse.

Oracle, bound, gate, cases and inputs: tests/flow_units_common.py (checked on the CPU by tests/test_host_flow_units.py).  The gate is
element-wise |got - ref64| <= d + 2^-24 |ref64| on every element of z~, z and the log-det, plus rel-L2 <= 1e-4 per sample row in exact
mode; plain fp32 torch on the CPU uses at most 0.31 (exact) / 0.36 (fp16 operands) of the bound, the GPU's measured maxima are in
profiles/flow_units_gate.md.  ``plan()`` of every pass is collected: the ledger test asserts that all 48 instantiations, both tail
kernels and the generic chain were run.  Every row of a batched tile-chain result equals the sample run alone, bit for bit."""
import pytest
import torch

import flow_units_common as fu

pytestmark = pytest.mark.gpu
LEDGER = set()     # ("first" | "hid", f16, kpw, ns), ("tail", f16), ("generic",)
_DONE = {}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    torch.set_grad_enabled(False)
    yield
    # the source of profiles/flow_units_gate.md: whatever ran in this session, printed once at its end
    print("\nFLOWUNITS worst |err| / bound per group:", {f"{g}/{p}": f"{r:.3f}" for (g, p), r in sorted(WORST.items())})


def _handle(monkeypatch, case, f16):
    """A loaded NativeFlow on the case's chain: I2V_FLOW_TILE is read at create, I2V_FLOW_NS / I2V_FLOW_FOLD at load."""
    import i2v_native
    env = {}
    if case["chain"] == "generic":
        env["I2V_FLOW_TILE"] = "0"
    if case["ns"] is not None:
        env["I2V_FLOW_NS"], env["I2V_FLOW_FOLD"] = str(case["ns"]), str(case["fold"])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = i2v_native.NativeFlow(64, case["E"], case["hidden"], case["depth"], fu.NFL, control=case["control"], activation=case["act"],
                              skip_actnorm=case["skip_an"], skip_shuffle=case["skip_sh"], linear_f16=f16)
    h.load(fu.tensors(fu.state_dict(case)))
    for k in env:
        monkeypatch.delenv(k)
    return h


def _note(case, f16, plan):
    if plan["chain"] == "generic":
        LEDGER.add(("generic",))
        return
    if plan["fold"]:
        LEDGER.add(("first", f16, plan["kpw"], plan["ns"]))
        if case["depth"] > 1:
            LEDGER.add(("hid", f16, plan["kpw"], plan["ns"]))
    else:
        LEDGER.add(("hid", f16, plan["kpw"], plan["ns"]))
        LEDGER.add(("tail", f16))


def _pass(h, x, e, reverse):
    if reverse:
        return h.inverse(x, e).cpu(), None
    zt, ld = h.forward(x, e)
    return zt.cpu(), ld.cpu()


def run_case(monkeypatch, case, poison=False):
    """Every pass of a case (once per process): gate, plan, row independence (tile chain), optionally one pass per precision and
    direction on a workspace filled with NaN.  Returns {(B, f16): plan}."""
    if case["id"] in _DONE:
        return _DONE[case["id"]]
    plans, failures = {}, []
    for f16 in case["precisions"]:
        h = _handle(monkeypatch, case, f16)
        one = _handle(monkeypatch, case, f16) if case["chain"] == "tile" else None   # the same chain at B = 1: a graph of its own
        for B in case["batches"]:
            plan = h.plan(B)
            plans[B, f16] = plan
            _note(case, f16, plan)
            for reverse in (False, True):
                x, e = fu.inputs(case, B, reverse)
                xd, ed = x.cuda(), e.cuda()
                z, ld = _pass(h, xd, ed, reverse)
                o = fu.oracle(case, B, bool(f16), reverse)
                ok, ratio, l2 = fu.gate(o, z, ld, bool(f16))
                tag = (case["id"], "fp16" if f16 else "fp32", B, "reverse" if reverse else "forward")
                print(f"FLOWUNITS {case['group']} {tag}: plan {plan}, |err| / bound {ratio:.3e}, rel-L2 {l2:.3e}")
                k = (case["group"], "fp16" if f16 else "fp32")
                WORST[k] = max(WORST.get(k, 0.0), ratio)
                if not ok:
                    failures.append((tag, ratio, l2))
                if poison and B == case["batches"][-1]:
                    h._ws.buf.view(torch.float32).fill_(float("nan"))
                    zp, ldp = _pass(h, xd, ed, reverse)
                    if not (torch.equal(zp, z) and (reverse or torch.equal(ldp, ld)) and bool(torch.isfinite(zp).all())):
                        failures.append((tag, "a pass on a NaN-filled workspace differs or is not finite"))
                if one is not None and B > 1:
                    for b in range(B):
                        z1, ld1 = _pass(one, xd[b:b + 1].contiguous(), ed[b:b + 1].contiguous(), reverse)
                        if not (torch.equal(z1[0], z[b]) and (reverse or torch.equal(ld1[0], ld[b]))):
                            failures.append((tag, f"row {b} differs from the sample run alone"))
                            break
    assert not failures, failures
    _DONE[case["id"]] = plans
    return plans


def _group(name):
    return [c for c in fu.CASES if c["group"] == name]


@pytest.mark.parametrize("case", _group("matrix"), ids=[c["id"] for c in _group("matrix")])
def test_tile_matrix(monkeypatch, case):
    plans = run_case(monkeypatch, case, poison=(case["ns"], case["fold"]) in ((1, 1), (4, 0)))
    for (B, f16), p in plans.items():
        assert p == {"chain": "tile", "kpw": case["hidden"] // 128, "ns": case["ns"], "fold": bool(case["fold"])}, (B, f16, p)


def test_ledger_every_instantiation_ran(monkeypatch):
    for case in _group("matrix"):
        run_case(monkeypatch, case, poison=(case["ns"], case["fold"]) in ((1, 1), (4, 0)))
    for case in _group("generic")[:1]:
        run_case(monkeypatch, case)
    want = {(k, f, kpw, ns) for k in ("first", "hid") for f in (0, 1) for kpw in (1, 2, 3, 4) for ns in (1, 2, 4)}
    assert len(want) == 48 and want <= LEDGER, sorted(want - LEDGER)
    assert {("tail", 0), ("tail", 1), ("generic",)} <= LEDGER
    print("FLOWUNITS ledger:", len(LEDGER & want), "instantiations, tails", sorted(t for t in LEDGER if t[0] == "tail"), "generic chain run")


def test_default_rule_edges(monkeypatch):
    (case,) = _group("edges")
    plans = run_case(monkeypatch, case)
    for f16 in (0, 1):
        got = [(plans[B, f16]["ns"], plans[B, f16]["fold"]) for B in (64, 65, 128, 129)]
        assert got == [(1, True), (2, False), (2, False), (4, False)], got


@pytest.mark.parametrize("case", _group("depth"), ids=[c["id"] for c in _group("depth")])
def test_depth(monkeypatch, case):
    run_case(monkeypatch, case)


@pytest.mark.parametrize("case", _group("embed"), ids=[c["id"] for c in _group("embed")])
def test_embedding_width_and_control(monkeypatch, case):
    run_case(monkeypatch, case)


@pytest.mark.parametrize("case", _group("flags") + _group("sparse"), ids=[c["id"] for c in _group("flags") + _group("sparse")])
def test_flags_fp16_and_sparse_weights(monkeypatch, case):
    run_case(monkeypatch, case)


@pytest.mark.parametrize("case", _group("generic"), ids=[c["id"] for c in _group("generic")])
def test_generic_chain(monkeypatch, case):
    plans = run_case(monkeypatch, case)
    assert all(p == {"chain": "generic", "kpw": 0, "ns": 0, "fold": False} for p in plans.values()), plans


def test_plan_refusals(monkeypatch):
    import ctypes
    import i2v_native
    lib = i2v_native.lib()
    h = _handle(monkeypatch, _group("edges")[0], 0)
    v = [ctypes.c_int32() for _ in range(4)]
    r = [ctypes.byref(i) for i in v]
    assert lib.i2v_flow_plan(h._h, 0, *r) == -1 and lib.i2v_flow_plan(h._h, -3, *r) == -1
    for i in range(4):
        assert lib.i2v_flow_plan(h._h, 8, *[None if j == i else r[j] for j in range(4)]) == -1
    raw = i2v_native.NativeFlow(64, 64, 128, 2, fu.NFL)
    assert lib.i2v_flow_plan(raw._h, 8, *r) == -5    # not loaded: the chain is chosen at load
    assert lib.i2v_flow_plan(h._h, 8, *r) == 0

