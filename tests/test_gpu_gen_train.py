"""GPU checks of the Generator's training path (csrc/i2v_gen_train.hip, stage1_VAE/modules/decoder.py ``Generator.differentiable``): fc, the
nearest up-sampling and the image head against float64 at the derived bounds of tests/gen_train_common.py; the module against the float64
oracle per tensor and against the fixtures made from the reference's own Generator (tests/golden/gen_train_*.npz); the bit-level
properties, the agreement with the inference handle, four SGD steps and the refusals.  Run with ``-s`` to see the figures of
profiles/gen_train_gate.md."""
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_train_common as gt
import i2v_native
from stage1_VAE.modules.decoder import Generator

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _grad_mode_on():
    """Other modules of the suite switch grad mode off for the process; these tests are about gradients."""
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


@pytest.fixture(scope="module")
def golden():
    return gt.load_golden()


_ORACLE = {}


def oracle(tag):
    """The float64 oracle's result of a case, computed once and shared."""
    if tag not in _ORACLE:
        case = gt.CASES[tag]
        img, z, c = gt.inputs(case)
        _ORACLE[tag] = gt.generator(gt.synthetic_state(case), img, z, case, c)
    return _ORACLE[tag]


def module(case, differentiable=True, mma=None):
    net = Generator(dict(gt.dic_of(case), **({} if mma is None else {"mma": mma})))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gt.synthetic_state(case).items()})
    net = net.to(DEV)
    net.differentiable = differentiable
    return net


def dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def report(name, ok, ratio, l2):
    print(f"  {name}: |err|/bound {ratio:.3f}  rel-L2 {l2:.2e}")
    assert ok, (name, ratio, l2)


def run(net, case, need_z=True):
    img, z, c = dev(*gt.inputs(case))
    z.requires_grad_(need_z)
    out = net(img, z)
    (c * out).sum().backward()
    return out, z.grad


# ---------------------------------------------------------------------------------------------------------------- the units

@pytest.mark.parametrize("B, K, nf", [(1, 4, 16), (3, 8, 16), (2, 64, 64)])
def test_fc_units(B, K, nf):
    rng = np.random.default_rng(700 + B + K + nf)
    J = 256 * nf
    z, w, b, g = rnd(rng, B, K), rnd(rng, J, K), rnd(rng, J), rnd(rng, B, J)
    out = i2v_native.gen_train_fc_forward_unit(*dev(z, w, b))
    report("forward", *gt.gate(out.cpu(), *gt.fc_ref(z, w, b), 1))
    dw, db, dz = i2v_native.gen_train_fc_backward_unit(*dev(g, z, w))
    dw64, db64, dz64, Sw, Sb, Sz = gt.fc_ref(z, w, b, g)
    slices = i2v_native.gen_train_fc_slices(J)
    assert slices == -(-J // 256)
    report("dW", *gt.gate(dw.cpu(), dw64, Sw, 1))
    report("db", *gt.gate(db.cpu()[None], db64[None], Sb[None], 1))
    report(f"dz ({slices} slices)", *gt.gate(dz.cpu(), dz64, Sz, slices))
    none, none2, dz2 = i2v_native.gen_train_fc_backward_unit(*dev(g, z, w), want_params=False)      # each optional output NULL in turn
    assert none is None and none2 is None and torch.equal(dz2, dz)
    dw3, db3, none = i2v_native.gen_train_fc_backward_unit(*dev(g, z, w), want_dz=False)
    assert none is None and torch.equal(dw3, dw) and torch.equal(db3, db)


FACTORS = [(2, 2), (1, 2), (2, 1), (4, 1), (1, 4), (4, 4)]
# (3, 5, 6): a row of 6 is no multiple of 4, the scalar forms at us = 1; (2, 3, 5): an odd row, the scalar forms at us = 2 too
LOW_MAPS = [(1, 4, 4), (3, 5, 6), (2, 3, 5)]


@pytest.mark.parametrize("thw", LOW_MAPS, ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("ut, us", FACTORS)
def test_upsample_units(ut, us, thw):
    for C, B in ((16, 1), (48, 3), (16, 3), (48, 1)):
        rng = np.random.default_rng(800 + 10 * ut + us + C + B)
        x = rnd(rng, B, C, *thw).to(DEV)
        up = i2v_native.gen_train_upsample(x, ut, us)
        assert torch.equal(up, F.interpolate(x, scale_factor=(ut, us, us)))       # bit-exact
        g = rnd(rng, *up.shape)
        dx = i2v_native.gen_train_upsample_backward(g.to(DEV), ut, us)
        ok, ratio, l2 = gt.gate(dx.cpu(), gt.upsample_backward(g.double(), ut, us), gt.upsample_backward(g.double().abs(), ut, us), max(ut * us * us - 1, 1))
        assert ok, (C, B, ratio, l2)
    print(f"  up-sampling ({ut}, {us}, {us}) on {thw}: bit-exact forward; backward |err|/bound {ratio:.3f} (C 48, B 1)")


def test_upsample_refuses_other_factors():
    x = torch.zeros(1, 16, 1, 4, 4, device=DEV)
    with pytest.raises(i2v_native.I2VError, match="1, 2, 4"):
        i2v_native.gen_train_upsample(x, 3, 1)
    lib = i2v_native.lib()
    assert lib.i2v_gen_train_upsample_forward(x.data_ptr(), 16, 1, 4, 4, 1, 3, x.data_ptr(), None) == -1
    assert "1, 2 or 4" in lib.i2v_last_error().decode()


@pytest.mark.parametrize("thw", [(1, 4, 4), (3, 5, 6), (8, 32, 32)], ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("nf", [16, 48, 64])
def test_head_units(nf, B, thw):
    """The references take the kernel's own frames (the backward starts from them) and its LeakyReLU decisions: x holds exact zeros, where
    the slope is 0.2."""
    rng = np.random.default_rng(900 + nf + B + thw[0])
    x = rnd(rng, B, nf, *thw)
    x[torch.from_numpy(rng.uniform(size=tuple(x.shape)) < 0.1)] = 0.0
    w = rnd(rng, 3, nf, 3, 3, 3) * (0.5 / np.sqrt(27 * nf))
    b, g = 0.2 * rnd(rng, 3), rnd(rng, B, thw[0], 3, *thw[1:])
    n = 27 * nf + 4
    y, saved = i2v_native.gen_train_head_forward_unit(*dev(x, w, b))
    y64, S, _, pre = gt.head_forward_ref(x, w, b)
    report("frames", *gt.gate(y.cpu(), y64, S, n))          # (|tanh'| <= 1: the pre-activation's bound holds behind the tanh)
    y2, none = i2v_native.gen_train_head_forward_unit(*dev(x, w, b), save=False)
    assert none is None and torch.equal(y2, y)
    dx, dw, db = i2v_native.gen_train_head_backward_unit(g.to(DEV), saved, w.to(DEV), tuple(x.shape))
    r = gt.head_backward_ref(x, w, g, y.cpu())
    report("dx", *gt.gate(dx.cpu(), r["dx"], r["S_dx"], n))
    report("dW", *gt.gate(dw.cpu(), r["dw"], r["S_dw"], n))
    report("db", *gt.gate(db.cpu()[None], r["db"][None], r["S_db"][None], 1))
    zero = (x == 0) & (r["S_dx"] > 0)
    assert bool(zero.any()) and bool((dx.cpu()[zero] != 0).any())        # the slope at exactly 0 is 0.2, not 0
    dx2, none, none2 = i2v_native.gen_train_head_backward_unit(g.to(DEV), saved, w.to(DEV), tuple(x.shape), want_params=False)
    assert none is None and none2 is None and torch.equal(dx2, dx)
    none, dw3, db3 = i2v_native.gen_train_head_backward_unit(g.to(DEV), saved, w.to(DEV), tuple(x.shape), want_dx=False)
    assert none is None and torch.equal(dw3, dw) and torch.equal(db3, db)


# ---------------------------------------------------------------------------------------------------------------- the module

def check(name, got, want, gate, scale=None):
    r = gt.rel(got.detach().cpu(), want, scale)
    print(f"  {name}: rel-L2 {r:.2e}  (gate {gate:.1e}, {r / gate:.3f} of it)")
    assert r <= gate, (name, r, gate)
    return r / gate


@pytest.mark.parametrize("tag", sorted(gt.CASES))
def test_module_matches_the_float64_oracle_and_the_reference_fixture(golden, tag):
    case = gt.CASES[tag]
    net = module(case).train()
    out, dz = run(net, case)
    assert out.grad_fn is not None and tuple(out.shape) == gt.out_shape(case) and out.is_contiguous()
    ref = oracle(tag)
    print(f"case {tag} against the float64 oracle:")
    worst = [check("frames", out, ref["out"], gt.gate_of(golden, tag, "out")), check("motion.grad", dz, ref["dz"], gt.gate_of(golden, tag, "dz"))]
    params = dict(net.named_parameters())
    assert set(params) == set(ref["grads"])
    for k, p in params.items():
        worst.append(check("d " + k, p.grad, ref["grads"][k], gt.gate_of(golden, tag, "g." + k), ref["scale"].get(k)))
    for k, b in net.named_buffers():
        check(k, b, ref[k], gt.TOL_L2)
    print(f"case {tag}: the worst tensor uses {max(worst):.3f} of its gate")
    if tag not in gt.FIXTURES:
        return
    print(f"case {tag} against the reference's fixture:")
    check("frames", out, golden[f"{tag}.out"], gt.gate_of(golden, tag, "out"))
    check("motion.grad", dz, golden[f"{tag}.dz"], gt.gate_of(golden, tag, "dz"))
    for k, p in params.items():
        if f"{tag}.g.{k}" in golden:
            check("d " + k, p.grad, golden[f"{tag}.g.{k}"], gt.gate_of(golden, tag, "g." + k), ref["scale"].get(k))
        else:
            gt.check_summary(k, p.grad, golden, tag, gt.gate_of(golden, tag, "g." + k))


def test_two_runs_give_the_same_bits():
    case = gt.CASES["c"]
    res = []
    for _ in range(2):
        net = module(case).train()
        out, dz = run(net, case)
        res.append([out.detach(), dz] + [p.grad for p in net.parameters()] + list(net.buffers()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_eval_forward_against_the_inference_handle_at_mma_0(golden):
    """Two arithmetics (the training kernels against the packed decoder's fp32 convs): a distance, not an identity."""
    case = gt.CASES["a"]
    img, z, _ = dev(*gt.inputs(case))
    with torch.no_grad():
        a = module(case, differentiable=True).eval()(img, z)
        b = module(case, differentiable=False, mma=0).eval()(img, z)
    assert a.grad_fn is None and a.shape == b.shape
    check("training forward (eval) against the inference handle, mma = 0", a, b.cpu(), gt.gate_of(golden, "a", "out"))


def test_not_differentiable_is_the_inference_handle_in_grad_mode_too():
    case = gt.CASES["a"]
    img, z, _ = dev(*gt.inputs(case))
    net = module(case, differentiable=False).eval()
    assert net.differentiable is False and not any(b.differentiable for b in net._blocks())
    with torch.no_grad():
        base = net(img, z)
    out = net(img, z.clone().requires_grad_(True))
    assert out.grad_fn is None and torch.equal(out, base)


def test_train_iterates_u_and_v_once_per_forward_and_eval_leaves_them():
    case = gt.CASES["b"]
    net = module(case).eval()
    before = {k: b.clone() for k, b in net.named_buffers()}
    assert len(before) == 2 * (6 * 2 + 4)
    run(net, case)
    assert all(torch.equal(b, before[k]) for k, b in net.named_buffers())
    net.train()
    run(net, case)
    assert all(not torch.equal(b, before[k]) for k, b in net.named_buffers())


def test_four_sgd_steps_follow_the_float64_losses(golden):
    case = gt.CASES["a"]
    net = module(case).train()
    img, z, c = dev(*gt.inputs(case))
    opt = torch.optim.SGD(net.parameters(), lr=gt.SGD_LR)
    losses = []
    for _ in range(gt.SGD_STEPS):
        opt.zero_grad()
        loss = (c * net(img, z)).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    dist = np.abs(np.array(losses) - golden["a.sgd_losses"]) / golden["a.sgd_scale"]
    own = np.abs(golden["a.sgd_losses_f32"] - golden["a.sgd_losses"]) / golden["a.sgd_scale"]
    print("  SGD: |loss - float64| / sum |c frames| per step:", dist, " the reference's own fp32:", own)
    assert len(set(np.round(losses, 4))) == gt.SGD_STEPS
    assert dist.max() <= (gt.TOL_L2 if own.max() <= gt.TOL_L2 / 4 else 4 * own.max()), dist
    # after the steps the inference handle is rebuilt from the stepped parameters
    net.eval()
    with torch.no_grad():
        trained = net(img, z)
    net.differentiable = False
    assert not any(b.differentiable for b in net._blocks())
    with torch.no_grad():
        after = net(img, z)
        fresh = module(case, differentiable=False).eval()(img, z)
    assert not torch.equal(after, fresh)
    net.mma = 0
    net.refresh_native()
    with torch.no_grad():
        check("inference handle (mma = 0) after the steps against the training forward", net(img, z), trained.cpu(), gt.gate_of(golden, "a", "out"))


def test_frozen_module_returns_motion_grad_without_parameter_gradients():
    case = gt.CASES["b"]
    net = module(case).train().requires_grad_(False)
    out, dz = run(net, case)
    assert out.grad_fn is not None and all(p.grad is None for p in net.parameters())
    net2 = module(case).train()
    _, dz2 = run(net2, case)
    assert dz is not None and torch.equal(dz, dz2)


def test_refusals():
    case = gt.CASES["b"]
    net = module(case).train()
    img, z, c = dev(*gt.inputs(case))
    z.requires_grad_(True)
    out = net(img, z)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad((c * out).sum(), z, create_graph=True)
    with pytest.raises(NotImplementedError, match="start frame"):
        net(img.clone().requires_grad_(True), z)
    with pytest.raises(NotImplementedError, match="differentiable"):
        net(img, z, out=torch.empty_like(out))
    with pytest.raises(NotImplementedError, match="differentiable"):
        net(img, z, realizations=2)
    with pytest.raises(NotImplementedError, match="differentiable"):
        net.prepare(img)
    with pytest.raises(i2v_native.I2VError, match="CPU"):
        net(img.cpu(), z.detach().cpu())
    assert net.__dict__["_train_native"] is not None and net.g_0.__dict__["_train_native"] is not None
    clone = pickle.loads(pickle.dumps(net))                  # pickling drops the native handles and keeps the mode
    assert clone.__dict__["_train_native"] is None and clone.g_0.__dict__["_train_native"] is None and clone.__dict__["_native"] is None
    assert clone.differentiable and clone(img, z).grad_fn is not None and clone.__dict__["_train_native"] is not None
    with pytest.raises(i2v_native.I2VError, match="multiple of 16"):
        i2v_native.NativeGenTrain(24, 8, device=DEV)
    with pytest.raises(i2v_native.I2VError, match="multiple of 16"):
        i2v_native.NativeGenTrain(80, 8, device=DEV)
