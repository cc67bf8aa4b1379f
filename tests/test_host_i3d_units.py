"""The float64 oracles of tests/i3d_units_common.py and the gate of tests/test_gpu_i3d_units.py, checked on the CPU:

* the oracles equal the outputs of the reference's own layer modules in ``.double()`` (fixture tests/golden/i3d_units.npz, made by
  tests/golden/make_golden_i3d_units.py) to 1e-12 relative;
* the gate discriminates: every deliberate error of ``MUTATIONS`` applied to the oracle fails it in at least one case of the GPU
  test's own case list, and the unmutated fp32 torch computation passes it in every case.  A mutation that survived would mean the case
  list is too weak."""
import numpy as np
import pytest
import torch

import i3d_units_common as uc
from fvd_common import load_fixture


@pytest.fixture(scope="module")
def golden():
    arrays, meta = load_fixture("i3d_units")
    assert meta["weights"] == uc.WEIGHT_SEED and meta["classes"] == uc.CLASSES
    return arrays


def _close(got, want):
    want = torch.from_numpy(want)
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_unit_oracle_equals_reference_modules(golden):
    units, _, _ = uc.fixture_cases()
    assert {c["variant"] for c in units} == {"kin", "dt"}
    for c in units:
        _close(uc.unit_oracle(c["variant"], c["unit"], uc.unit_input(c))[0], golden["unit/" + c["id"]])


def test_mixed_oracle_equals_reference_modules(golden):
    _, mixed, _ = uc.fixture_cases()
    for c in mixed:
        cin = uc.fc.MIXED[uc.BLOCKS.index(c["block"])][1]
        x = uc.randn(c["seed"], (c["shape"][0], cin, *c["shape"][1:]))
        got = torch.cat([y for y, _, _ in uc.mixed_oracle(c["variant"], c["block"], x)], 1)
        _close(got, golden["mixed/" + c["id"]])


def test_maxpool_oracle_equals_reference_modules(golden):
    _, _, pools = uc.fixture_cases()
    assert len(pools) == 2 * len(uc.POOLS) * 2
    for c in pools:
        got = uc.maxpool_oracle(c["variant"], uc.pool_input(c).double(), c["kernel"], c["stride"])
        want = torch.from_numpy(golden["pool/" + c["id"]])
        assert tuple(got.shape) == tuple(want.shape) and torch.equal(got, want), c["id"]


def test_fixture_has_no_other_entries(golden):
    units, mixed, pools = uc.fixture_cases()
    want = {"unit/" + c["id"] for c in units} | {"mixed/" + c["id"] for c in mixed} | {"pool/" + c["id"] for c in pools}
    assert set(golden) == want


def test_case_list_covers_every_path_the_issue_names():
    cases = uc.unit_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    specs = [uc.unit_spec(c["variant"], c["unit"]) for c in cases]
    # column templates 32 / 64 / 128 by the packer's rule (the tile that pads Cout least, the wider on a tie)
    def bn(cout):
        best = 128
        for b in (64, 32):
            if -(-cout // b) * b < -(-cout // best) * best:
                best = b
        return best
    assert {bn(s[2]) for s in specs} == {32, 64, 128}
    assert {16, 24, 48, 96, 112, 144, 192} <= {s[1] for s in specs if s[3] == 3}            # cin of the 3x3x3 units
    assert {16, 24, 96, 112, 144, 384, 18, 400} <= {s[2] for s in specs if s[3] == 1}       # ragged cout of the 1x1 units
    assert {208, 288, 48} <= {s[2] for s in specs if s[3] == 3}
    for c in cases:
        B, T, H, W = c["shape"]
        assert H != W or c["unit"] == uc.UNIT_HEAD or c["shape"] in uc.M_LADDER[:2], c["id"]
    ms = sorted({int(np.prod(c["shape"])) for c in cases if c["shape"] in uc.M_LADDER})
    assert ms == [50, 128, 130, 378]


@pytest.fixture(scope="module")
def clean_units():
    """(case, x, ref, S, n) of every unit case, the float64 oracle computed once."""
    out = []
    for c in uc.unit_cases():
        x = uc.unit_input(c)
        out.append((c, x) + uc.unit_oracle(c["variant"], c["unit"], x))
    return out


def test_clean_fp32_computation_passes_the_gate(clean_units):
    worst = {}
    for c, x, ref, S, n in clean_units:
        ok, ratio, l2 = uc.gate(uc.unit_fp32(c["variant"], c["unit"], x), ref, S, n)
        k = uc.unit_spec(c["variant"], c["unit"])[3]
        worst[k] = max(worst.get(k, (0, 0)), (ratio, l2))
        assert ok, (c["id"], ratio, l2)
    print("CPU fp32 vs float64, worst (|err| / bound, rel-L2) per kernel size:", {k: (f"{r:.3e}", f"{e:.3e}") for k, (r, e) in worst.items()})
    assert max(r for r, _ in worst.values()) < 0.25   # no slack factor over the derived bound is needed, let alone 4 x this deviation


@pytest.mark.parametrize("mutation", [m for m, kinds in uc.MUTATIONS.items() if "conv" in kinds])
def test_conv_mutation_fails_the_gate(clean_units, mutation):
    caught = []
    for c, x, ref, S, n in clean_units:
        got = uc.unit_oracle(c["variant"], c["unit"], x, mutate=mutation)[0]
        if not uc.gate(got.float(), ref, S, n)[0]:
            caught.append(c["id"])
    print(f"{mutation}: caught in {len(caught)} of {len(clean_units)} unit cases")
    assert caught, f"{mutation} survives every unit case: the case list is too weak"
    if mutation == "swap_hw_extent":     # a 1x1 unit does not see its neighbours; every 3x3x3 and 7x7x7 case with H != W must catch it
        need = [c["id"] for c, *_ in clean_units if uc.unit_spec(c["variant"], c["unit"])[3] > 1 and c["shape"][2] != c["shape"][3]]
        assert set(need) <= set(caught)
    if mutation == "kinetics_rule":      # the dynamic-texture stem at an odd extent
        assert caught and all(i.startswith("dt-Conv3d_1a_7x7") for i in caught)


@pytest.mark.parametrize("mutation", [m for m, kinds in uc.MUTATIONS.items() if "pool" in kinds])
def test_pool_mutation_fails_the_gate(mutation):
    caught, cases = [], uc.pool_cases(channels=(4,), batch=1)
    for c in cases:
        x = uc.pool_input(c)
        ref = uc.maxpool_oracle(c["variant"], x, c["kernel"], c["stride"])
        got = uc.maxpool_oracle(c["variant"], x, c["kernel"], c["stride"], mutate=mutation)
        if tuple(got.shape) != tuple(ref.shape) or not torch.equal(got, ref):
            caught.append(c["id"])
    print(f"{mutation}: caught in {len(caught)} of {len(cases)} pool cases")
    assert caught, f"{mutation} survives every pool case: the case list is too weak"
    if mutation == "neg_inf_padding":    # an all-negative input tells 0 from -inf in every padded window, a random one only by chance
        neg = [i[:-4] for i in caught if i.endswith("neg")]
        assert set(i[:-4] for i in caught if i.endswith("rnd")) <= set(neg) and len(neg) > len(caught) - len(neg)


def test_head_mutations_fail_the_gate():
    """Average pool and time mean: the fp32 computation passes; one dropped time step, one dropped map position and the two layouts
    mistaken for each other fail."""
    for c in uc.HEAD_CASES:
        B, T = c["shape"]
        x = uc.randn(c["seed"], (B, 1024, T, 7, 7))
        ref, S, n = uc.avgpool_oracle(x, c["pool_t"])
        fp32 = torch.nn.functional.avg_pool3d(x, (c["pool_t"], 7, 7), stride=1)[..., 0, 0]
        assert uc.gate(fp32, ref, S, n)[0], c["id"]
        x2 = x.clone()
        x2[:, :, -1, 6, 6] = 0
        assert not uc.gate(uc.avgpool_oracle(x2, c["pool_t"])[0].float(), ref, S, n)[0], c["id"]
        if ref.shape[2] > 1:
            assert not uc.gate(ref.transpose(1, 2).reshape(ref.shape).float(), ref, S, n)[0], c["id"]
            m, Sm, nm = uc.time_mean_oracle(ref)
            assert uc.gate(ref.float().mean(2), m, Sm, nm)[0]
            assert not uc.gate(ref[:, :, :-1].mean(2).float(), m, Sm, nm)[0]
