"""The float64 oracle, the error bound and the case matrix of tests/flow_units_common.py, checked on the CPU before tests/test_gpu_flow_units.py
relies on them:

* the oracle equals oracle/flow_ref run in float64 to 1e-12 for the switches flow_ref covers, and the reference's own modules' outputs
  in tests/golden/flow_units.npz at that file's accuracy (fp32 outputs: rel-L2 2e-5, the pin of tests/test_oracle_golden.py);
* for every pass of every case, oracle/flow_ref in plain fp32 torch (under ``linear_f16_emulation()`` in fp16 mode) passes the gate.  Worst
  fraction of the bound it uses, measured with torch's CPU BLAS: 0.31 in exact mode (groups: matrix 0.12, edges 0.12, depth 0.12,
  embed 0.20, sparse 0.23, generic 0.31), 0.36 in fp16 mode (matrix 0.14, depth 0.17, embed 0.21, flags 0.08, sparse 0.36);
* every deliberate error of ``MUTATIONS`` fails the gate in at least one case, in each precision it applies to.  The operand-rounding
  mutation (one Linear's input left unrounded) shows only where an output depends on few operands: the bound of a dense Linear allows
  gamma(K + 2) sum |w| |x|, more than one rounding of each operand moves the sum, so the matrix holds one case with one weight per row;
* what a wrong GEMM would do -- one 16-wide k-block of a hidden Linear lost, one output row of a hidden Linear lost, one wave's partial
  tile of the last Linear lost -- fails the gate in EVERY pass at hidden 128, 256, 384 and 512 in both precisions (smallest |err| /
  bound: 124 / 43 / 1118 in exact mode, 12 / 4.3 / 122 with fp16 operands), and a dropped last embedding element in every pass of
  every E and control in both precisions (274 / 32);
* no sample of any case has a LeakyReLU / InvLeakyRelu input within its own bound of 0, in the exact-mode oracle and in the
  fp16-operand oracle alike, and at least half of the candidates of every pool qualify (smallest kept fraction: 0.92)."""
import numpy as np
import pytest
import torch

import flow_units_common as fu
import i2v_native
import i2v_synth as synth
from conftest import load_golden, rel_l2

torch.set_grad_enabled(False)


def test_plan_symbol_is_declared_listed_and_exported():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "i2v_hip.h")).read()
    assert re.search(r"\bint i2v_flow_plan\(const i2v_flow\* f, int32_t batch, int32_t\* chain", hdr)
    assert "i2v_flow_plan" in i2v_native.SYMBOLS and hasattr(i2v_native.lib(), "i2v_flow_plan")
    assert callable(i2v_native.NativeFlow.plan)
    # refusals that need no device: null handle, null outputs, batch <= 0
    import ctypes
    lib, v = i2v_native.lib(), [ctypes.c_int32() for _ in range(4)]
    refs = [ctypes.byref(i) for i in v]
    assert lib.i2v_flow_plan(None, 4, *refs) == -1
    assert "null argument" in lib.i2v_last_error().decode()


def test_case_matrix_covers_what_the_kernels_branch_on():
    cs = fu.CASES
    m = [c for c in cs if c["group"] == "matrix"]
    assert {(c["hidden"] // 128, c["ns"], c["fold"]) for c in m} == {(k, n, f) for k in (1, 2, 3, 4) for n in (1, 2, 4) for f in (0, 1)}
    assert all(c["precisions"] == (0, 1) and c["depth"] == 2 and c["E"] == 64 for c in m)
    assert all(c["batches"] == fu.NS_BATCHES[c["ns"]] for c in m) and fu.NS_BATCHES == {1: (1, 17), 2: (35,), 4: (147,)}
    assert [c["batches"] for c in cs if c["group"] == "edges"] == [(64, 65, 128, 129)]
    assert {(c["hidden"], c["depth"]) for c in cs if c["group"] == "depth"} == {(128, 1), (128, 3), (384, 1), (384, 3)}
    assert {(c["E"], c["control"]) for c in cs if c["group"] == "embed"} == {(E, k) for E in (1, 15, 16, 17, 94, 128) for k in (0, 1, 2)}
    assert {(c["skip_an"], c["skip_sh"], c["act"]) for c in cs if c["group"] == "flags"} == set(fu.FLAG_SETS)
    g = [c for c in cs if c["group"] == "generic"]
    assert {(c["hidden"], c["depth"]) for c in g if c["chain"] == "generic"} == {(h, d) for h in (64, 192, 320, 448, 512) for d in (0, 1, 2)}
    assert {(c["hidden"], c["depth"]) for c in g if c["chain"] == "auto"} == {(64, 1), (192, 2), (128, 0)}
    assert {(c["E"], c["control"]) for c in g} == {(E, k) for E in (1, 17, 94) for k in (0, 2)}
    assert {(c["depth"], c["E"]) for c in g if c["chain"] == "generic"} == {(d, E) for d in (0, 1, 2) for E in (1, 17, 94)}
    assert all(c["batches"] == (1, 63, 64, 65, 130) for c in g)


PIN_CASES = [c for c in fu.CASES if c["control"] in (0, 1) and not c["skip_an"] and not c["skip_sh"] and c["act"] == "lrelu"
             and c["group"] in ("embed", "depth", "generic") and not c["sparse"]]


def test_oracle_equals_flow_ref_in_float64():
    from oracle import flow_ref
    assert {c["control"] for c in PIN_CASES} == {0, 1} and {0, 1, 2, 3} <= {c["depth"] for c in PIN_CASES}
    for c in PIN_CASES:
        sd = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in fu.tensors(fu.state_dict(c)).items()}
        x, e = fu.candidates(c, 5)
        o = fu.Oracle(c).run(x, e)
        zt, ld = flow_ref.flow_forward(sd, x.double(), e.double(), n_flows=fu.NFL, depth=c["depth"], control=bool(c["control"]))
        assert float((o.z - zt.reshape(5, 64)).abs().max()) <= 1e-12 * float(zt.abs().max()), c["id"]
        assert float((o.ld - ld).abs().max()) <= 1e-12 * float(ld.abs().max()), c["id"]
        z = flow_ref.flow_reverse(sd, x.double(), e.double(), n_flows=fu.NFL, depth=c["depth"], control=bool(c["control"]))
        assert float((fu.Oracle(c, reverse=True).run(x, e).z - z.reshape(5, 64)).abs().max()) <= 1e-12 * float(z.abs().max()), c["id"]


def test_oracle_equals_the_reference_modules_outputs():
    """tests/golden/flow_units.npz: one full block (ActNorm, InvLeakyRelu, coupling, Shuffle) and the bare 'normal' and 'cond' couplings
    of the reference's own modules at hidden 512, depth 2."""
    g, meta = load_golden("flow_units")
    x = torch.from_numpy(g["cpl_x"])
    full = dict(hidden=512, depth=2, E=64, control=0, skip_an=False, skip_sh=False, act="lrelu")
    bare = dict(full, skip_an=True, skip_sh=True, act="none")
    bare_c = dict(bare, E=94, control=2)
    for case, sd, e, keys in ((full, synth.flow_state_dict(**meta["synth"]), g["cpl_e"], ("blk_fwd", "blk_logdet", "blk_rev")),
                              (bare, synth.flow_state_dict(**meta["synth"]), g["cpl_e"], ("cpl_fwd", "cpl_logdet", "cpl_rev")),
                              (bare_c, synth.flow_state_dict(**meta["synth_cond"]), g["cplc_e"], ("cplc_fwd", "cplc_logdet", "cplc_rev"))):
        e = torch.from_numpy(e)
        o = fu.Oracle(case, sd=sd, blocks=(1,)).run(x, e)
        assert rel_l2(o.z, g[keys[0]].reshape(6, 64)) < 2e-5 and np.allclose(o.ld, g[keys[1]], atol=1e-5), keys
        assert rel_l2(fu.Oracle(case, reverse=True, sd=sd, blocks=(1,)).run(x, e).z, g[keys[2]].reshape(6, 64)) < 2e-5, keys


def test_pools_are_free_of_kinks_and_keep_at_least_half():
    worst = 1.0
    for c in fu.CASES:
        for reverse in (False, True):
            x, e, kept, drawn = fu.pool(c, reverse)
            worst = min(worst, kept / drawn)
            assert drawn == fu.POOL_FACTOR * c["Bmax"] and 2 * kept >= drawn, (c["id"], reverse, kept, drawn)
            for f16 in (False, True):
                assert float(fu.Oracle(c, f16, reverse).run(x[:c["Bmax"]], e[:c["Bmax"]]).margin.min()) > 0, (c["id"], reverse, f16)
    print(f"smallest kept fraction of a pool: {worst:.2f}")


def test_fp32_reference_passes_the_gate_in_every_case():
    worst, seen = {}, set()
    for c in fu.CASES:
        for B, f16, reverse in fu.runs(c):
            key = (fu.geometry_key(c), B, f16, reverse)
            if key in seen:
                continue
            seen.add(key)
            x, e = fu.inputs(c, B, reverse)
            z, ld = fu.reference_fp32(c, x, e, f16, reverse)
            ok, ratio, l2 = fu.gate(fu.oracle(c, B, f16, reverse), z, ld, f16)
            k = (c["group"], "fp16" if f16 else "fp32")
            worst[k] = max(worst.get(k, (0.0, 0.0)), (ratio, l2))
            assert ok, (c["id"], B, f16, reverse, ratio, l2)
    print("CPU fp32 reference vs float64, worst (|err| / bound, rel-L2) per group:", {k: (f"{r:.3f}", f"{l:.2e}") for k, (r, l) in worst.items()})
    assert max(r for r, _ in worst.values()) < 0.5


MUTATION_CASES = [c for c in fu.CASES if c["group"] in ("embed", "flags", "sparse")]   # hidden 128, B = 17: quick, and every switch occurs
WIDTH_CASES = [c for c in fu.CASES if c["group"] == "matrix" and (c["ns"], c["fold"]) == (1, 1)]   # hidden 128 / 256 / 384 / 512


def _caught(mutation, f16, case_list, batches=None):
    """[(case id, B, reverse, caught)] of every pass of ``case_list`` in one precision that the mutation applies to"""
    out = []
    for c in case_list:
        for B, f, reverse in fu.runs(c):
            if f != f16 or (batches and B not in batches) or not fu.mutation_applies(mutation, c, f16, reverse, B):
                continue
            x, e = fu.inputs(c, B, reverse)
            m = fu.Oracle(c, f16, reverse, mutation).run(x, e)
            ok, ratio, _ = fu.gate(fu.oracle(c, B, f16, reverse), m.z.float(), None if reverse else m.ld.float(), f16)
            out.append((c["id"], B, reverse, not ok, ratio))
    return out


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("mutation", list(fu.MUTATIONS))
def test_mutation_fails_the_gate(mutation, f16):
    if mutation == "f16_unrounded" and not f16:
        assert not any(fu.mutation_applies(mutation, c, False, r, 17) for c in MUTATION_CASES for r in (False, True))
        return
    got = _caught(mutation, f16, MUTATION_CASES)
    print(f"{mutation} ({'fp16' if f16 else 'fp32'}): caught in {sum(g[3] for g in got)} of {len(got)} passes")
    assert any(g[3] for g in got), f"{mutation} survives every case: the case list is too weak"


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("mutation", fu.WEIGHT_MUTATIONS)
def test_a_wrong_gemm_fails_the_gate_at_every_hidden_width(mutation, f16):
    """A lost k-block, output row or wave partial of ONE Linear is rejected in every pass, forward and reverse, at each of the four
    hidden widths (KPW 1 .. 4) in both precisions: the gate sees the hidden-layer GEMMs that the instantiation matrix covers."""
    assert {c["hidden"] for c in WIDTH_CASES} == {128, 256, 384, 512}
    got = _caught(mutation, f16, WIDTH_CASES, batches=(17,))
    print(f"{mutation} ({'fp16' if f16 else 'fp32'}): smallest |err| / bound {min(g[4] for g in got):.1f}")
    assert len(got) == 8 and all(g[3] for g in got), [g for g in got if not g[3]]


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
def test_a_dropped_embedding_element_fails_the_gate_at_every_width_and_control(f16):
    """E in {1, 15, 16, 17, 94, 128} x control {0, 1, 2}: the ragged fragments of the embedding part of the first Linear"""
    got = _caught("drop_last_embed", f16, [c for c in fu.CASES if c["group"] == "embed"])
    print(f"drop_last_embed ({'fp16' if f16 else 'fp32'}): smallest |err| / bound {min(g[4] for g in got):.1f}")
    assert len(got) == 36 and all(g[3] for g in got), [g for g in got if not g[3]]
