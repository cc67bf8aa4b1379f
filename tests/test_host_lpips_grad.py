"""CPU-side checks of the LPIPS backward surface: the float64 oracles of tests/lpips_grad_common.py against autograd and against the
fixture written from the reference's own module, the deliberate errors the gates have to catch, the seeds' distance from a mask flip,
and the new native symbols."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i2v_native
import lpips_grad_common as lg
import vgg_common as vc
from conftest import REPO

NEW_SYMBOLS = ["i2v_vgg_saved_bytes", "i2v_vgg_backward_workspace_bytes", "i2v_vgg_features_saved", "i2v_lpips_layer_backward", "i2v_vgg_backward",
               "i2v_vgg_dgrad_unit", "i2v_vgg_maxpool2_backward"]


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
    """Other modules of the suite switch grad mode off for the process; these tests are about gradients."""
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    declared = set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    lib = i2v_native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in i2v_native.SYMBOLS and hasattr(lib, name), name
    for ref in ("stage1_VAE/modules/loss.py:139", "stage2_cINN/AE/modules/loss.py:38"):
        assert ref in header, ref
    for method in ("backward", "lpips_backward"):
        assert callable(getattr(i2v_native.NativeVGG, method))


# ---------------------------------------------------------------------------------------------------------------- dgrad

@pytest.mark.parametrize("cin,cout,hw", [(64, 16, (5, 7)), (64, 64, (9, 17)), (128, 48, (8, 16))])
def test_dgrad_identity_and_what_its_gate_catches(cin, cout, hw):
    case = {"cin": cin, "cout": cout, "hw": hw, "batch": 2, "mask": 1, "add": 1, "seed": 17500 + cin + cout}
    g, w, add, y, other = lg.dgrad_inputs(case)
    x = torch.zeros(2, cin, *hw, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), padding=1).backward(g.double())
    plain, S, n = lg.dgrad_oracle(g, w)
    assert n == 9 * cout and float((plain - x.grad).abs().max()) <= 1e-12             # flipped + transposed = autograd
    ref, S, n = lg.dgrad_oracle(g, w, add, y)
    assert float((ref - (x.grad + add.double()) * (y > 0)).abs().max()) <= 1e-12
    fp32 = (F.conv2d(g, w.transpose(0, 1).flip(2, 3).contiguous(), padding=1) + add) * (y > 0)
    ok, ratio, l2 = lg.gate(fp32, ref, S, n)
    assert ok, (ratio, l2)
    for m in lg.DGRAD_MUTATIONS:
        if m == "kernel_not_transposed" and cin != cout:
            continue
        bad = lg.dgrad_oracle(g, w, add, y, mutate=m, other=other)[0]
        assert not lg.gate(bad.float(), ref, S, n)[0], m


def test_first_layer_form_divides_by_scale():
    case = lg.first_cases()[0]
    g, w, _, _, _ = lg.dgrad_inputs(case)
    x = torch.zeros(case["batch"], 3, *case["hw"], dtype=torch.float64, requires_grad=True)
    F.conv2d(vc.input_oracle(x, "lpips"), w.double(), padding=1).backward(g.double())  # through ScalingLayer: d/dx = d/dinput / scale
    ref, S, n = lg.dgrad_oracle(g, w, scale=vc.LPIPS_SCALE)
    assert n == 9 * 64 + 1 and float((ref - x.grad).abs().max()) <= 1e-12
    assert not lg.gate(lg.dgrad_oracle(g, w)[0].float(), ref, S, n)[0]                   # the scale left out


# ---------------------------------------------------------------------------------------------------------------- pool

def test_pool_backward_rule_is_the_first_maximum_in_row_major_order():
    g = torch.ones(1, 1, 1, 1)
    assert lg.pool_backward_torch(torch.tensor([[[[1., 1.], [1., 1.]]]]), g).flatten().tolist() == [1, 0, 0, 0]
    assert lg.pool_backward_torch(torch.tensor([[[[0., 2.], [2., 1.]]]]), g).flatten().tolist() == [0, 1, 0, 0]
    y = lg.pool_input("ties12", (1, 4, 7, 9), 5)
    got = lg.pool_backward_torch(y, torch.ones(1, 4, 3, 4))
    assert torch.equal(got[:, :, 0:6:2, 1:8:2], torch.ones(1, 4, 3, 4)) and float(got.sum()) == 4 * 3 * 4      # all at (0, 1); the odd row / column zero
    w = lg.windows(y)
    assert torch.equal(w.argmax(-1), torch.ones(1, 4, 3, 4, dtype=torch.long))                                    # torch.argmax: the first maximum too
    y = lg.pool_input("ties", (1, 4, 6, 10), 6)
    assert torch.equal(lg.windows(y).argmax(-1), torch.zeros(1, 4, 3, 5, dtype=torch.long))


# ---------------------------------------------------------------------------------------------------------------- head

@pytest.mark.parametrize("case", [c for c in lg.HEAD_CASES if c["c"] in (64, 512)], ids=lambda c: c["id"])
def test_head_closed_form_is_autograd_except_at_the_zero_vector(case):
    f0, f1, lin, u = lg.head_inputs(case)
    d0, d1, B0, B1 = lg.head_backward_oracle(f0, f1, lin, u)
    a0, a1 = lg.head_backward_autograd(f0, f1, lin, u)
    zero = (f0.double().pow(2).sum(1, keepdim=True) == 0).expand_as(f0)
    assert torch.isfinite(d0).all() and torch.isfinite(d1).all()
    if case["hw"] != (1, 1):
        assert int(zero.sum()) == case["c"] and torch.isnan(a0[zero]).all()           # torch's sqrt backward at 0: the kept-out quirk
    scale = float(d0[~zero].abs().max())
    assert float((d0 - a0)[~zero].abs().max()) <= 1e-12 * scale and float((d1 - a1).abs().max()) <= 1e-12 * scale
    assert (d0.abs() <= B0 * (1 + 1e-12)).all() and (d1.abs() <= B1 * (1 + 1e-12)).all()    # the bound's magnitude dominates the value
    ok, ratio, l2 = lg.head_gate(d0.float(), d0, B0, case["c"])
    assert ok, (ratio, l2)
    assert not lg.head_gate((1 + 1e-3) * d0.float(), d0, B0, case["c"])[0]                  # a 0.1 % error is caught


# ---------------------------------------------------------------------------------------------------------------- trunk

@pytest.mark.parametrize("hw", [(16, 16), (24, 40)])
def test_masked_oracle_is_plain_autograd_on_its_own_masks(hw):
    sd, lin = vc.vgg_state_dict(lg.SEED_W), vc.lin_state_dict(lg.SEED_LIN)
    a, b, wts = lg.e2e_frames({"hw": hw, "n": 2, "seed": 19500 + hw[0]})
    x0, x1 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    val, t0, t1 = lg.lpips_masked(sd, lin, x0, x1)
    assert float((val.detach() - vc.lpips_oracle(sd, lin, a, b)).abs().max()) <= 1e-12
    (wts * val).sum().backward()
    y0, y1 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    val2, _, _ = lg.lpips_masked(sd, lin, y0, y1, [t.detach() for t in t0[2]], [t.detach() for t in t1[2]])
    (wts * val2).sum().backward()
    assert torch.equal(val2, val)
    for p, q in ((x0, y0), (x1, y1)):
        assert float((p.grad - q.grad).norm() / p.grad.norm()) <= 1e-12
    assert lg.fragile_units(t0[1], [t.detach() for t in t0[2]]) == (0, 0.0)


def test_committed_seeds_have_no_fragile_unit():
    """torch fp32 against float64 on the CPU: the masks agree at every unit of all thirteen layers, for every end-to-end and fixture input."""
    sd = vc.vgg_state_dict(lg.SEED_W)
    frames = {}
    for case in lg.e2e_cases():
        frames[(case["hw"], case["n"])] = lg.e2e_frames(case)[:2]
    for tag in lg.GOLDEN:
        frames[tag] = lg.golden_frames(tag)[:2]
    for key, pair in frames.items():
        for x in pair:
            xn = lg.lpips_frames(x)
            _, pres, _ = lg.trunk_masked(sd, xn.double())
            count, worst = lg.fragile_units(pres, lg.fp32_activations(sd, xn))
            assert count == 0, (key, count, worst)


def test_fixture_matches_its_seeds_and_the_oracle():
    arr, meta = vc.load_fixture("vgg_lpips_grad")
    assert meta["weights"] == {"seed": lg.SEED_W, "lin_seed": lg.SEED_LIN} and meta["gate_rel_l2"] == lg.TOL_L2
    sd, lin = vc.vgg_state_dict(lg.SEED_W), vc.lin_state_dict(lg.SEED_LIN)
    for tag, g in lg.GOLDEN.items():
        sz = meta["sizes"][tag]
        assert (sz["h"], sz["w"], sz["seed"], sz["n"]) == (g["h"], g["w"], g["seed"], lg.GOLDEN_N) and sz["weights"] == lg.e2e_weights(lg.GOLDEN_N).tolist()
        a, b, wts = lg.golden_frames(tag)
        x0, x1 = a.double().requires_grad_(True), b.double().requires_grad_(True)
        val, _, _ = lg.lpips_masked(sd, lin, x0, x1)
        (wts * val).sum().backward()
        assert np.max(np.abs(val.detach().numpy() - arr[f"lpips64_{tag}"]) / arr[f"lpips64_{tag}"]) <= 1e-9
        for name, x in (("input", x0), ("target", x1)):
            ref = arr[f"grad_{name}_{tag}"]
            assert ref.shape == tuple(x.shape) and ref.dtype == np.float64
            assert abs(float(np.linalg.norm(ref)) - sz[f"grad_{name}_l2"]) <= 1e-12 * sz[f"grad_{name}_l2"]
            assert vc.rel_l2(x.grad, ref) <= 1e-9, (tag, name)
