"""GPU checks of the GeneratorBlock's training path (csrc/i2v_gblock_train.hip, stage1_VAE/modules/decoder.py
``GeneratorBlock.differentiable``): the new kernel families against float64 at the derived bounds of tests/gblock_train_common.py, the
module against the fixtures made from the reference's own module (tests/golden/gblock_train_*.npz), the bit-level properties, the
agreement with the inference handle and six SGD steps.  Run with ``-s`` to see the figures of profiles/gblock_train_gate.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gblock_train_common as gc
import i2v_native
from stage1_VAE.modules.decoder import GeneratorBlock

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
    return gc.load_golden()


def module(cfg, differentiable=True, sd=None, mma=None):
    net = GeneratorBlock(cfg["n_in"], cfg["n_out"], cfg["spectral"], cfg["z_dim"], mma=mma)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in (sd or gc.synthetic_state(cfg)).items()})
    net = net.to(DEV)
    net.differentiable = differentiable
    return net


def dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def report(name, ok, ratio, l2):
    print(f"  {name}: |err|/bound {ratio:.3f}  rel-L2 {l2:.2e}")
    assert ok, (name, ratio, l2)


def check(name, got, want, scale=None):
    r = gc.rel(got.detach().cpu(), want, scale)
    print(f"  {name}: rel-L2 {r:.2e}")
    assert r <= gc.TOL_L2, (name, r)
    return r


def run(net, cfg, need_x=True, need_z=True):
    x, z, img, c = dev(*gc.inputs(cfg))
    x.requires_grad_(need_x)
    z.requires_grad_(need_z)
    out = net(x, z, img)
    (c * out).sum().backward()
    return out, x.grad, z.grad


# ---------------------------------------------------------------------------------------------------------------- the kernel families

@pytest.mark.parametrize("case", gc.UNIT_CASES, ids=lambda c: f"c{c[0]}-b{c[1]}-{'x'.join(map(str, c[2]))}")
@pytest.mark.parametrize("mode", [i2v_native.GBLOCK_TRAIN_SPADE, i2v_native.GBLOCK_TRAIN_ADAIN], ids=["spade", "adain"])
def test_modnorm_backward_unit(mode, case):
    """The reference takes the kernel's own inputs and LeakyReLU decisions (some exact zeros in act: the slope there is 0.2)."""
    C, B, thw = case
    seed = 100 + gc.UNIT_CASES.index(case)
    g, act, x = gc.unit_inputs(seed, C, B, thw)
    rng = np.random.default_rng(seed + 50)
    mod_shape = (B, thw[1], thw[2], C) if mode == 0 else (B, 2 * C)
    mod = torch.from_numpy(rng.standard_normal(mod_shape).astype(np.float32))
    add = torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32))
    dx64, dg64, db64, S, (Sg, Sb) = gc.modnorm_ref(mode, g, act, x, mod, add)
    dx, dg, db = i2v_native.gblock_train_modnorm_backward_unit(mode, *dev(g, act, x, mod, add))
    report("dx", *gc.gate(dx.cpu(), dx64, S, 4))
    report("dgamma", *gc.gate(dg.cpu(), dg64, Sg, 2))
    if mode == 0:
        report("dbeta", *gc.gate(db.cpu(), db64, Sb, 2))
    # every optional pointer NULL in turn: the others keep their bits
    dx_n, dg2, _ = i2v_native.gblock_train_modnorm_backward_unit(mode, *dev(g, act, x, mod, None))
    dx64n = gc.modnorm_ref(mode, g, act, x, mod)
    report("dx without add", *gc.gate(dx_n.cpu(), dx64n[0], dx64n[3], 4))
    assert torch.equal(dg2, dg)
    none, dg3, _ = i2v_native.gblock_train_modnorm_backward_unit(mode, *dev(g, act, x, mod, add), want_dx=False)
    assert none is None and torch.equal(dg3, dg)
    dx4, none, none2 = i2v_native.gblock_train_modnorm_backward_unit(mode, *dev(g, act, x, mod, add), want_maps=False)
    assert none is None and none2 is None and torch.equal(dx4, dx)


@pytest.mark.parametrize("case", gc.UNIT_CASES, ids=lambda c: f"c{c[0]}-b{c[1]}-{'x'.join(map(str, c[2]))}")
def test_pointwise_conv_units(case):
    """conv_s: the 1x1x1 conv (and, with the transposed weight, its input gradient) and its weight gradient with the projection."""
    cin, B, thw = case
    idx = gc.UNIT_CASES.index(case)
    cout = (16, 48, 64, 128)[(idx + 1) % 4]
    rng = np.random.default_rng(300 + idx)
    x = torch.from_numpy(rng.standard_normal((B,) + thw + (cin,)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B,) + thw + (cout,)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32))
    add = torch.from_numpy(rng.standard_normal((B,) + thw + (cout,)).astype(np.float32))
    xd, gd, wd = x.double(), g.double(), w.double()
    out = i2v_native.gblock_train_pointwise_unit(*dev(x, w, add))
    report("forward", *gc.gate(out.cpu(), xd @ wd.t() + add.double(), xd.abs() @ wd.abs().t() + add.abs().double(), cin + 1))
    out2 = i2v_native.gblock_train_pointwise_unit(*dev(x, w))
    report("forward without add", *gc.gate(out2.cpu(), xd @ wd.t(), xd.abs() @ wd.abs().t(), cin + 1))
    dxg = i2v_native.gblock_train_pointwise_unit(*dev(g, w.t().contiguous()))
    report("input gradient", *gc.gate(dxg.cpu(), gd @ wd, gd.abs() @ wd.abs(), cout + 1))
    rows = x.numel() // cin
    slices, length = gc.wgrad1_plan(cout, cin, rows)
    dwn64 = gd.reshape(rows, cout).t() @ xd.reshape(rows, cin)
    S = gd.reshape(rows, cout).abs().t() @ xd.reshape(rows, cin).abs()
    dw = i2v_native.gblock_train_pointwise_wgrad_unit(*dev(g, x, w))
    report(f"weight gradient ({slices} slices of {length})", *gc.gate(dw.cpu(), dwn64, S, slices + length))
    u = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    v = torch.from_numpy(rng.standard_normal(cin).astype(np.float32))
    u, v = u / u.norm(), v / v.norm()
    sigma = torch.tensor([float(u.double() @ (wd @ v.double()))], dtype=torch.float32)
    ref, bound = gc.sn_finish_ref(dwn64, S, slices + length, wd, u.double(), v.double(), sigma[0])
    dwo = i2v_native.gblock_train_pointwise_wgrad_unit(*dev(g, x, w, u, v, sigma))
    report("weight gradient, projected", *gc.gate_bound(dwo.cpu(), ref, bound))
    acc = dwo.clone()
    i2v_native.gblock_train_pointwise_wgrad_unit(*dev(g, x, w, u, v, sigma), dweight=acc)
    assert torch.equal(acc, dwo + dwo)


@pytest.mark.parametrize("case", gc.UNIT_CASES[:4] + [gc.BIG_CASE], ids=lambda c: f"c{c[0]}-b{c[1]}-{'x'.join(map(str, c[2]))}")
def test_bias_gradient_and_linear_backward_units(case):
    C, B, thw = case
    rng = np.random.default_rng(400 + C + B)
    g = torch.from_numpy(rng.standard_normal((B,) + thw + (C,)).astype(np.float32))
    db = i2v_native.gblock_train_bias_grad_unit(g.to(DEV))
    flat = g.double().reshape(-1, C)
    report("bias gradient", *gc.gate(db.cpu()[None], flat.sum(0)[None], flat.abs().sum(0)[None], 1))
    acc = db.clone()
    i2v_native.gblock_train_bias_grad_unit(g.to(DEV), dbias=acc)
    assert torch.equal(acc, db + db)
    J, K = 2 * C, (8, 4, 64, 5)[B % 4]
    d_lin = torch.from_numpy(rng.standard_normal((B, J)).astype(np.float32))
    z = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal((J, K)).astype(np.float32))
    dw, dbl, dz = i2v_native.gblock_train_linear_backward_unit(*dev(d_lin, z, w))
    dl, zd, wd = d_lin.double(), z.double(), w.double()
    report("Linear dw", *gc.gate(dw.cpu(), dl.t() @ zd, dl.abs().t() @ zd.abs(), 1))
    report("Linear db", *gc.gate(dbl.cpu()[None], dl.sum(0)[None], dl.abs().sum(0)[None], 1))
    report("Linear dz", *gc.gate(dz.cpu(), dl @ wd, dl.abs() @ wd.abs(), 1))
    for i in range(3):   # each output NULL in turn
        want = tuple(j != i for j in range(3))
        got = i2v_native.gblock_train_linear_backward_unit(*dev(d_lin, z, w), want=want)
        for j, (a, b) in enumerate(zip(got, (dw, dbl, dz))):
            assert (a is None) if j == i else torch.equal(a, b)


@pytest.mark.parametrize("case", [(3, 128, 2, 5, 6), (128, 48, 1, 4, 4), (128, 16, 3, 8, 8), (128, 64, 2, 5, 6), (16, 128, 1, 8, 8)],
                         ids=lambda c: f"{c[0]}to{c[1]}-b{c[2]}-{c[3]}x{c[4]}")
def test_spade_branch_conv2d_on_the_trunk_kernels(case):
    """Spade's 2-D convs run as the trunk's conv with a (3, 1, 3) window on [H][1][W]: forward, input gradient, weight gradient."""
    cin, cout, B, H, W = case
    rng = np.random.default_rng(500 + cin + cout + B)
    cinp = 4 if cin == 3 else cin
    x = torch.from_numpy(rng.standard_normal((B, H, W, cinp)).astype(np.float32))
    if cin == 3:
        x[..., 3] = 0
    g = torch.from_numpy(rng.standard_normal((B, H, W, cout)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32))
    y, dx, dw = i2v_native.gblock_train_conv2d_unit(*dev(x, w, g), want=(True, cin != 3, True))
    xc, gc_ = x[..., :cin].permute(0, 3, 1, 2).double(), g.permute(0, 3, 1, 2).double()
    wd = w.double()
    nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
    K = -(-9 * cinp // 16) * 16
    report("forward", *gc.gate(y.cpu(), nhwc(F.conv2d(xc, wd, padding=1)), nhwc(F.conv2d(xc.abs(), wd.abs(), padding=1)), K))
    dx64, dw64, _ = gc.conv_grads(xc, wd, gc_, 1)
    Sx, Sw, _ = gc.conv_grads(xc.abs(), wd.abs(), gc_.abs(), 1)
    if cin != 3:
        report("input gradient", *gc.gate(dx.cpu(), nhwc(dx64), nhwc(Sx), 9 * cout + 1))
    slices, length = gc.wgrad_plan(cout, cin, 9, B * H * W)
    report(f"weight gradient ({slices} slices of {length})", *gc.gate(dw.cpu(), dw64, Sw, slices + length))
    y2, none, none2 = i2v_native.gblock_train_conv2d_unit(*dev(x, w, None))
    assert none is None and none2 is None and torch.equal(y2, y)
    none, none2, dw2 = i2v_native.gblock_train_conv2d_unit(*dev(x, w, g), want=(False, False, True))
    assert none is None and none2 is None and torch.equal(dw2, dw)


# ---------------------------------------------------------------------------------------------------------------- the module

@pytest.mark.parametrize("tag", sorted(gc.FIXTURES))
def test_module_matches_the_reference_fixture(golden, tag):
    cfg = gc.FIXTURES[tag]
    net = module(cfg).train()
    out, dx, dz = run(net, cfg)
    x, z, img, c = gc.inputs(cfg)
    scale = gc.block(gc.synthetic_state(cfg), x, z, img, cfg, c)["scale"]
    print(f"fixture {tag}:")
    check("out", out, golden[f"{tag}.out"])
    check("dx", dx, golden[f"{tag}.dx"])
    check("dz", dz, golden[f"{tag}.dz"])
    params = dict(net.named_parameters())
    want = {k[len(tag) + 3:]: v for k, v in golden.items() if k.startswith(tag + ".g.")}
    assert set(want) == set(params)
    for k, v in want.items():
        check("d " + k, params[k].grad, v, scale.get(k))
    for k, b in net.named_buffers():
        check(k, b, golden[f"{tag}.{'u' if k.endswith('_u') else 'v'}.{k.rsplit('.', 1)[0]}"])


def test_module_on_a_large_map_runs_the_128_row_workgroup_form():
    """16 channels at 4 x 16 x 32 x 32: rows_of picks the 128-row workgroups of the conv and the input-gradient kernels; against the
    float64 oracle."""
    C, B, thw = gc.BIG_CASE
    cfg = dict(n_in=C, n_out=C, spectral=True, z_dim=4, B=B, map=thw, img=(16, 16), seed=21)
    net = module(cfg).train()
    out, dx, dz = run(net, cfg)
    x, z, img, c = gc.inputs(cfg)
    ref = gc.block(gc.synthetic_state(cfg), x, z, img, cfg, c)
    check("out", out, ref["out"])
    check("dx", dx, ref["dx"])
    check("dz", dz, ref["dz"])
    for k, p in net.named_parameters():
        check("d " + k, p.grad, ref["grads"][k], ref["scale"].get(k))


def test_two_runs_give_the_same_bits():
    cfg = gc.FIXTURES["c"]
    res = []
    for _ in range(2):
        net = module(cfg).train()
        out, dx, dz = run(net, cfg)
        res.append([out.detach(), dx, dz] + [p.grad for p in net.parameters()] + list(net.buffers()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


# the inference handle tiles its maps into bricks: it runs on power-of-two maps only, so what involves it uses this block
CFG_INF = dict(n_in=64, n_out=32, spectral=True, z_dim=8, B=2, map=(2, 8, 8), img=(16, 16), seed=31)


def test_not_differentiable_is_the_inference_handle_bit_for_bit():
    cfg = CFG_INF
    x, z, img, _ = dev(*gc.inputs(cfg))
    net = module(cfg, differentiable=False).eval()
    with torch.no_grad():
        base = net(x, z, img)
    handle = i2v_native.NativeGBlock(cfg["n_in"], cfg["n_out"], cfg["z_dim"], cfg["spectral"], device=DEV)
    handle.load(net.state_dict())
    assert torch.equal(base, handle.forward(x, z, img))
    out = net(x.clone().requires_grad_(True), z, img)   # grad mode: the same handle, no graph
    assert out.grad_fn is None and torch.equal(out, base)


def test_eval_leaves_u_and_v_alone_and_train_iterates_them():
    cfg = gc.FIXTURES["a"]
    net = module(cfg).eval()
    before = {k: b.clone() for k, b in net.named_buffers()}
    run(net, cfg)
    assert all(torch.equal(b, before[k]) for k, b in net.named_buffers())
    net.train()
    run(net, cfg)
    assert all(not torch.equal(b, before[k]) for k, b in net.named_buffers())


def test_frozen_module_returns_dx_and_dz_without_parameter_gradients(golden):
    cfg = gc.FIXTURES["a"]
    net = module(cfg).train().requires_grad_(False)
    out, dx, dz = run(net, cfg)
    assert all(p.grad is None for p in net.parameters())
    check("dx", dx, golden["a.dx"])
    check("dz", dz, golden["a.dz"])
    net2 = module(cfg).train()
    _, dx2, dz2 = run(net2, cfg)
    assert torch.equal(dx, dx2) and torch.equal(dz, dz2)
    _, none, dz3 = run(module(cfg).train().requires_grad_(False), cfg, need_x=False)
    assert none is None and torch.equal(dz3, dz)


def test_create_graph_and_a_start_frame_that_requires_grad_raise():
    cfg = gc.FIXTURES["b"]
    net = module(cfg).train()
    x, z, img, c = dev(*gc.inputs(cfg))
    x.requires_grad_(True)
    out = net(x, z, img)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad((c * out).sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match="start frame"):
        net(x, z, img.clone().requires_grad_(True))


def test_switching_back_gives_the_inference_handle_the_new_weights():
    cfg = CFG_INF
    net = module(cfg, differentiable=False, mma=0).eval()
    x, z, img, c = dev(*gc.inputs(cfg))
    with torch.no_grad():
        before = net(x, z, img)
    net.differentiable = True
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    (c * net(x, z, img)).sum().backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        trained = net(x, z, img)
    net.differentiable = False
    with torch.no_grad():
        after = net(x, z, img)
    assert not torch.equal(after, before)
    check("inference handle after the step against the training forward", after, trained.cpu())


def test_training_forward_in_eval_against_the_inference_handle_at_mma_0():
    """Two arithmetics (the trunk's conv kernel against the decoder's fp32 conv): a distance, not an identity."""
    cfg = CFG_INF
    x, z, img, _ = dev(*gc.inputs(cfg))
    with torch.no_grad():
        a = module(cfg, differentiable=True).eval()(x, z, img)
        b = module(cfg, differentiable=False, mma=0).eval()(x, z, img)
    check("training forward (eval) against the inference handle, mma = 0", a, b.cpu())


def test_six_sgd_steps_follow_the_float64_sequence(golden):
    cfg = gc.FIXTURES["a"]
    net = module(cfg).train()
    x, z, img, c = dev(*gc.inputs(cfg))
    opt = torch.optim.SGD(net.parameters(), lr=gc.SGD_LR)
    losses = []
    for _ in range(gc.SGD_STEPS):
        opt.zero_grad()
        loss = (c * net(x, z, img)).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    dist = np.abs(np.array(losses) - golden["a.sgd_losses"]) / golden["a.sgd_scale"]
    print("  SGD: |loss - float64| / sum |c out| per step:", dist, " the reference's own fp32:",
          np.abs(golden["a.sgd_losses_f32"] - golden["a.sgd_losses"]) / golden["a.sgd_scale"])
    assert dist.max() <= gc.TOL_L2, dist
