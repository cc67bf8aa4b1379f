"""Training the cINN on the GPU (csrc/i2v_flow_train.hip, i2v_train.py): gradients of the differentiable forward, accumulation,
determinism, fused Adam, a 12-step trajectory and the hand-over to sampling.

Reference for all of them: ``oracle/flow_ref.flow_forward`` under torch autograd on the CPU in float64 with ``i2v_synth``
weights, and ``torch.optim.Adam`` on the CPU.  Gates: per-tensor relative L2 <= 1e-4 (the project's standing fp32 gate; the
reference's own fp32 gradients sit at <= 1e-6 from the fp64 oracle) on EVERY gradient tensor; relative loss difference <= 1e-4 on
every step of the trajectory; the fused Adam update within 3x the fp32-vs-fp64 noise of torch's own CPU Adam."""
import numpy as np
import pytest
import torch

import i2v_synth as synth
from flow_train_common import load_grad_fixture, oracle_grads, rel

pytestmark = pytest.mark.gpu
TOL = 1e-4


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


def _flow(sd_np, emb, hid, nf, control, differentiable=True):
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    flow = ConditionalFlow(64, emb, hid, 2, nf, conditioning_option="None", control=control)
    flow.load_state_dict(T(sd_np))
    flow = flow.cuda()
    flow.differentiable = differentiable
    return flow


def _run(flow, x, e, d_zt=None, d_logdet=None, need_input_grads=True):
    """differentiable forward + backward on the GPU -> (zt, logdet, {"x", "embed", parameter name: grad}) on the CPU."""
    xg = x.cuda().requires_grad_(need_input_grads)
    eg = e.cuda().requires_grad_(need_input_grads)
    flow.zero_grad(set_to_none=True)
    zt, logdet = flow(xg, eg)
    assert zt.shape == (x.shape[0], 64, 1, 1) and logdet.shape == (x.shape[0],) and zt.grad_fn is not None and logdet.grad_fn is not None
    zt2 = zt.reshape(x.shape[0], -1)
    if d_zt is None:
        loss = (0.5 * zt2.pow(2).sum(1)).mean() - logdet.mean()
    else:
        loss = (zt2 * d_zt.cuda()).sum() + (logdet * d_logdet.cuda()).sum()
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in flow.named_parameters()}
    if need_input_grads:
        grads["x"], grads["embed"] = xg.grad.cpu(), eg.grad.cpu()
    return zt2.detach().cpu(), logdet.detach().cpu(), grads


def _compare(got, want, what, failures=None):
    """every tensor of `want` (none may be left out) against `got`; prints the worst figure before asserting (with `failures`
    the assertion is left to the caller, who collects every case first)"""
    errs = {k: rel(got[k], want[k]) for k in want}
    assert set(got) == set(want), set(got) ^ set(want)
    worst = max(errs, key=errs.get)
    bad = {k: v for k, v in errs.items() if v > TOL}
    print(f"{what}: {len(errs)} tensors, worst rel-L2 {errs[worst]:.3e} ({worst}), {len(bad)} above the gate")
    if failures is not None and bad:
        failures.append((what, len(bad), errs[worst], worst))
        return
    assert errs[worst] <= TOL, bad


def test_gradients_fixture_geometry():
    arrays, meta = load_grad_fixture()
    s = meta["synth"]
    flow = _flow(synth.flow_state_dict(**s), s["embedding_dim"], s["hidden_dim"], s["n_flows"], s["control"])
    zt, logdet, grads = _run(flow, torch.from_numpy(arrays["x"]), torch.from_numpy(arrays["embed"]))
    want = {k[5:]: v for k, v in arrays.items() if k.startswith("grad.")}
    want.update(x=arrays["d_x"], embed=arrays["d_embed"])
    assert len(want) == 70
    _compare({**grads, "zt": zt, "logdet": logdet}, {**want, "zt": arrays["zt"], "logdet": arrays["logdet"]}, "fixture")


KINK_MARGIN = 1e-5


def _kink_free_pool(sd, emb, control, n=1536):
    """Samples for the shipped-geometry cases.  The flow is piecewise smooth (LeakyReLU(0.01), InvLeakyRelu(0.9)); a sample with
    one of its 124 k pre-activations within fp32 rounding of 0 puts ANY fp32 evaluation on either side of that kink, and the
    two one-sided gradients differ by a finite amount (seen: the reference's own fp32 gradients 1e-4 ... 6e-3 from fp64 on about
    1 % of the samples, i.e. on most batches of 130).  The 1e-4 gate is a statement about smooth points, so the cases are built
    from smooth points, by a rule that looks at the float64 oracle alone and is decided on the CPU before the code under test
    runs: candidates are drawn from one seeded stream, and a sample is kept when every LeakyReLU / InvLeakyRelu input of the fp64
    oracle is at least 1e-5 away from 0.  Where 1e-5 comes from: the largest fp32-vs-fp64 difference of those inputs in the
    oracle's own fp32 run (measured 9.7e-6 over 1200 samples with one BLAS, up to 1.6e-5 with another, reached at the LARGE
    inputs; printed per case) -- an fp32 evaluation
    whose error stays inside the reference's own cannot cross a kink that far away.  Asserted for the kept samples: the oracle's
    own fp32 run changes none of those inputs by more than half its size.  About a quarter of the candidates are kept."""
    from flow_train_common import kink_margins
    x, e = rnd(1000 + emb, n, 64), rnd(2000 + emb, n, emb)
    margin = torch.cat([kink_margins(sd, x[i:i + 512], e[i:i + 512], 20, control)[0] for i in range(0, n, 512)])
    keep = (margin >= KINK_MARGIN).nonzero().flatten()
    print(f"kink-free pool: {len(keep)} of {n} candidates are >= {KINK_MARGIN} away from every kink")
    assert len(keep) >= 1 + 7 + 50 + 64 + 130
    return x[keep], e[keep]


@pytest.mark.parametrize("emb,control", [(64, False), (128, False), (94, True)])
def test_gradients_shipped_geometries(emb, control):
    from flow_train_common import kink_margins
    sd = synth.flow_state_dict(seed=7, n_flows=20, embedding_dim=emb, hidden_dim=512, control=control)
    flow = _flow(sd, emb, 512, 20, control)
    px, pe = _kink_free_pool(sd, emb, control)
    failures, first = [], 0
    for B in (1, 7, 50, 64, 130):
        x, e = px[first:first + B].contiguous(), pe[first:first + B].contiguous()
        first += B
        margin, err, crossing = kink_margins(sd, x, e, 20, control)
        print(f"B={B}: kink margin {float(margin.min()):.2e}, the oracle's own fp32 input error: absolute {float(err.max()):.2e}, "
              f"relative {float(crossing.max()):.2e}")
        assert float(margin.min()) >= KINK_MARGIN and float(crossing.max()) <= 0.5, (float(margin.min()), float(crossing.max()))
        for case in ("flowloss", "random"):
            d_zt, d_ld = (None, None) if case == "flowloss" else (rnd(300 + B, B, 64), rnd(400 + B, B))
            zt_r, ld_r, _, want = oracle_grads(sd, x, e, torch.float64, 20, control, d_zt, d_ld)
            _, _, _, w32 = oracle_grads(sd, x, e, torch.float32, 20, control, d_zt, d_ld)
            own = max(rel(w32[k], want[k]) for k in want)
            assert own <= 1e-5, f"the reference's own fp32 gradients are {own:.3e} from fp64 at a point chosen to be smooth"
            zt, logdet, grads = _run(flow, x, e, d_zt, d_ld)
            assert len(want) == 682
            _compare({**grads, "zt": zt, "logdet": logdet}, {**want, "zt": zt_r, "logdet": ld_r},
                     f"E={emb} control={control} B={B} {case} (kink margin {float(margin.min()):.1e}, reference fp32 {own:.1e})", failures)
    assert not failures, failures


@pytest.mark.parametrize("kind", ["coupling_normal", "coupling_cond", "block_normal", "block_cond_noact"])
def test_gradients_leaf_classes(kind):
    from oracle import flow_ref
    from stage2_cINN.modules.flow_blocks import ConditionalDoubleVectorCouplingBlock, ConditionalFlatDoubleCouplingFlowBlock
    sd_np = synth.flow_state_dict(seed=11, n_flows=1, embedding_dim=64, hidden_dim=256, control=False)
    mode = "cond" if "cond" in kind else "normal"
    if mode == "cond":   # first layers that see the embedding only
        sd_np = {k: (v[:, 32:].copy() if k.endswith("main.0.weight") else v) for k, v in sd_np.items()}
    B = 9
    x, e = rnd(1, B, 64), rnd(2, B, 64)
    d_zt, d_ld = rnd(3, B, 64), rnd(4, B)
    if kind.startswith("coupling"):
        pre = "sub_layers.0.coupling."
        mod = ConditionalDoubleVectorCouplingBlock(64, 64, 256, 2, mode=mode)
        fwd = lambda sd, xx, ee: flow_ref.coupling_forward(sd, "", xx, ee, mode, 2)                         # noqa: E731
    else:
        pre = "sub_layers.0."
        act = "none" if kind.endswith("noact") else "lrelu"
        mod = ConditionalFlatDoubleCouplingFlowBlock(64, 64, 256, 2, activation=act, mode=mode)
        fwd = lambda sd, xx, ee: flow_ref.block_forward(sd, "", xx, ee, mode, 2, act)                       # noqa: E731
    sub = {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items() if k.startswith(pre)}
    if not kind.startswith("coupling"):
        sub["norm_layer.initialized"] = torch.tensor(1, dtype=torch.uint8)
    mod.load_state_dict(sub)
    mod = mod.cuda()
    mod.differentiable = True
    xg, eg = x.cuda().requires_grad_(True), e.cuda().requires_grad_(True)
    out, ld = mod(xg[:, :, None, None], eg[:, :, None, None])
    ((out.reshape(B, -1) * d_zt.cuda()).sum() + (ld * d_ld.cuda()).sum()).backward()
    got = {k: p.grad.cpu() for k, p in mod.named_parameters()}
    got.update(x=xg.grad.cpu(), embed=eg.grad.cpu(), out=out.detach().reshape(B, -1).cpu(), logdet=ld.detach().cpu())
    ref = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sub.items()}
    xr, er = x.double().requires_grad_(True), e.double().requires_grad_(True)
    o_r, ld_r = fwd(ref, xr, er)
    ((o_r * d_zt.double()).sum() + (ld_r * d_ld.double()).sum()).backward()
    want = {k: v.grad for k, v in ref.items() if v.is_floating_point() and v.dtype == torch.float64}
    want.update(x=xr.grad, embed=er.grad, out=o_r.detach(), logdet=ld_r.detach())
    assert all(v is not None for v in want.values())
    _compare(got, want, kind)


def test_accumulation_and_set_to_none():
    sd = synth.flow_state_dict(seed=7, n_flows=4, embedding_dim=94, hidden_dim=256, control=True)
    flow = _flow(sd, 94, 256, 4, True)
    x1, e1, x2, e2 = rnd(1, 7, 64), rnd(2, 7, 94), rnd(3, 5, 64), rnd(4, 5, 94)
    _, _, _, w1 = oracle_grads(sd, x1, e1, torch.float64, 4, True)
    _, _, _, w2 = oracle_grads(sd, x2, e2, torch.float64, 4, True)
    names = [k for k, _ in flow.named_parameters()]

    def backward(x, e):
        zt, ld = flow(x.cuda(), e.cuda())
        ((0.5 * zt.reshape(x.shape[0], -1).pow(2).sum(1)).mean() - ld.mean()).backward()

    flow.zero_grad(set_to_none=True)
    backward(x1, e1)
    backward(x2, e2)                      # no zero_grad in between: the sum
    _compare({k: p.grad.cpu() for k, p in flow.named_parameters()}, {k: w1[k] + w2[k] for k in names}, "two backwards")
    flow.zero_grad(set_to_none=False)     # zeroed in place, then filled again
    assert all(float(p.grad.abs().max()) == 0 for p in flow.parameters())
    backward(x2, e2)
    _compare({k: p.grad.cpu() for k, p in flow.named_parameters()}, {k: w2[k] for k in names}, "after zero_grad")
    flow.zero_grad(set_to_none=True)      # gradient tensors are re-created
    assert all(p.grad is None for p in flow.parameters())
    backward(x1, e1)
    _compare({k: p.grad.cpu() for k, p in flow.named_parameters()}, {k: w1[k] for k in names}, "after set_to_none")


def test_step_is_deterministic():
    sd = synth.flow_state_dict(seed=7, n_flows=20, embedding_dim=64, hidden_dim=512)
    x, e = rnd(1, 50, 64), rnd(2, 50, 64)
    outs = []
    for _ in range(2):
        flow = _flow(sd, 64, 512, 20, False)
        opt = torch.optim.Adam(flow.parameters(), lr=1e-5, betas=(0.9, 0.99), amsgrad=True)
        zt, ld = flow(x.cuda(), e.cuda())
        ((0.5 * zt.reshape(50, -1).pow(2).sum(1)).mean() - ld.mean()).backward()
        grads = [p.grad.clone() for p in flow.parameters()]
        opt.step()
        outs.append((grads, [p.detach().clone() for p in flow.parameters()]))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][0], outs[1][0])), "gradients differ between two identical runs"
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1])), "updated parameters differ between two identical runs"
    from i2v_train import FlowTrainer
    ps = []
    for _ in range(2):
        flow = _flow(sd, 64, 512, 20, False)
        tr = FlowTrainer(flow)
        tr.step(x.cuda(), e.cuda())
        tr.step(x.cuda(), e.cuda())
        ps.append([p.detach().clone() for p in flow.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*ps)), "FlowTrainer: parameters differ between two identical runs"


@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_fused_adam_vs_fp64(amsgrad, weight_decay):
    """5 steps on seeded gradients over the flow's real parameter shapes.  The update p_k - p_0 is a few thousand ulps of the
    weights, so its gate is measured, not fixed: 3x the relative L2 of torch's own fp32 CPU Adam against fp64 Adam."""
    from i2v_train import FusedAdam
    sd = synth.flow_state_dict(seed=7, n_flows=20, embedding_dim=64, hidden_dim=512)
    p0 = [torch.from_numpy(np.asarray(v)) for v in sd.values() if np.asarray(v).dtype.kind == "f"]
    gen = torch.Generator().manual_seed(5)
    grads = [[torch.randn(p.shape, generator=gen) * 0.3 for p in p0] for _ in range(5)]
    kw = dict(lr=1e-5, betas=(0.9, 0.99), weight_decay=weight_decay, amsgrad=amsgrad)

    def run(opt_cls, dtype, device):
        ps = [p.clone().to(dtype).to(device).requires_grad_(True) for p in p0]
        opt = opt_cls(ps, **kw)
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g.to(dtype).to(device)
            opt.step()
        return torch.cat([(p.detach().cpu().double() - q.double()).reshape(-1) for p, q in zip(ps, p0)])

    u64 = run(torch.optim.Adam, torch.float64, "cpu")
    u32 = run(torch.optim.Adam, torch.float32, "cpu")
    ugpu = run(FusedAdam, torch.float32, "cuda")
    noise, err = rel(u32, u64), rel(ugpu, u64)
    print(f"adam amsgrad={amsgrad} wd={weight_decay}: torch fp32 vs fp64 {noise:.3e}, fused kernel vs fp64 {err:.3e}")
    assert err <= 3 * noise, (err, noise)


def _cpu_trajectory(sd_np, x, e, steps):
    """fp64 oracle + torch.optim.Adam on the CPU, the reference's hyper-parameters -> (losses, trained state dict)"""
    sd = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in T(sd_np).items()}
    from oracle import flow_ref
    opt = torch.optim.Adam([v for v in sd.values() if v.is_floating_point()], lr=1e-5, betas=(0.9, 0.99), weight_decay=0, amsgrad=True)
    losses = []
    for _ in range(steps):
        zt, ld = flow_ref.flow_forward(sd, x.double(), e.double(), n_flows=20)
        loss = (0.5 * zt.reshape(x.shape[0], -1).pow(2).sum(1)).mean() - ld.mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses, {k: v.detach() for k, v in sd.items()}


@pytest.fixture(scope="module")
def trajectory():
    sd = synth.flow_state_dict(seed=7, n_flows=20, embedding_dim=64, hidden_dim=512)
    x, e = rnd(21, 50, 64), rnd(22, 50, 64)
    losses, trained = _cpu_trajectory(sd, x, e, 12)
    return sd, x, e, losses, trained


def _check_losses(got, want, what):
    errs = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print(f"{what}: losses {[round(v, 4) for v in got]}\n  reference {[round(v, 4) for v in want]}\n  worst relative difference {max(errs):.3e}")
    assert len(got) == len(want) == 12 and max(errs) <= TOL, errs
    assert all(b < a for a, b in zip(got, got[1:])), "the loss must fall monotonically"


def test_trajectory_torch_adam_and_reference_loop(trajectory):
    """The reference's loop, verbatim, on a SupervisedTransformer whose flow is differentiable, with torch.optim.Adam."""
    from stage2_cINN.modules.INN import SupervisedTransformer
    from stage2_cINN.modules.loss import FlowLoss, LossLogger
    sd, x, e, want, _ = trajectory
    cINN = SupervisedTransformer(flow_in_channels=64, flow_mid_channels=512, flow_hidden_depth=2, n_flows=20,
                                 flow_conditioning_option="None", control=False)
    cINN.flow.load_state_dict(T(sd))
    cINN = cINN.cuda()
    cINN.differentiable = True
    optimizer = torch.optim.Adam(cINN.parameters(), lr=1e-5, betas=(0.9, 0.99), weight_decay=0, amsgrad=True)
    logger, loss_func = LossLogger(), FlowLoss()
    z, embed = x.cuda(), e.cuda()
    for _ in range(12):
        gauss, logdet = cINN(z, None, embed=embed)
        loss = loss_func(gauss, logdet, logger, mode="train")
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
    _check_losses([en["Loss"] for en in logger.entries], want, "autograd + torch.optim.Adam")


def test_trajectory_flow_trainer_and_handover_to_sampling(trajectory):
    """FlowTrainer / FusedAdam on the same batch; then sampling uses the TRAINED weights: reverse against the oracle on the trained
    state_dict, and with differentiable off again a forward has the bits of i2v_flow_forward on a freshly loaded handle."""
    from i2v_train import FlowTrainer
    from oracle import flow_ref
    sd, x, e, want, trained = trajectory
    flow = _flow(sd, 64, 512, 20, False)
    z, embed = x.cuda(), e.cuda()
    with torch.no_grad():
        before = flow(z, embed, reverse=True)            # packs the UNTRAINED parameters into the inference handle
    tr = FlowTrainer(flow, lr=1e-5, betas=(0.9, 0.99), weight_decay=0, amsgrad=True)
    got = [tr.step(z, embed) for _ in range(12)]
    assert all(set(g) == {"Loss", "reference_nll_loss", "nlogdet_loss", "nll_loss"} and g["Loss"].is_cuda for g in got)
    _check_losses([float(g["Loss"]) for g in got], want, "FlowTrainer + FusedAdam")
    with torch.no_grad():
        res = rnd(31, 50, 64)
        zs = flow(res.cuda(), embed, reverse=True).reshape(50, -1).cpu()
        ref = flow_ref.flow_reverse({k: (v.float() if v.is_floating_point() else v) for k, v in trained.items()}, res, e, n_flows=20).reshape(50, -1)
        err = rel(zs, ref)
        print(f"reverse after training vs oracle on the trained state_dict: {err:.3e}")
        assert err <= TOL and not torch.equal(before, flow(z, embed, reverse=True))
        flow.differentiable = False
        a, la = flow(z, embed)
        fresh = _flow({k: v.detach().cpu().numpy() for k, v in flow.state_dict().items()}, 64, 512, 20, False, differentiable=False)
        b, lb = fresh(z, embed)
        assert a.grad_fn is None and torch.equal(a, b) and torch.equal(la, lb)


def test_model_sampling_uses_trained_flow(tmp_path):
    """get_model.Model: train its cINN a few steps, then Model-level sampling against the oracle on the trained state_dict."""
    from conftest import load_golden
    from get_model import Model
    from i2v_train import FlowTrainer
    from oracle import decoder_ref, model_ref
    from test_gpu_parity import _write_checkpoints
    _, meta = load_golden("model_nf8")
    model = Model(_write_checkpoints(tmp_path, meta), 16, mma=0)
    x0, residual, embed = synth.bench_inputs(2, 64, 64)
    with torch.no_grad():
        y0 = model.synthesize(x0.cuda(), residual=residual.cuda(), embed=embed.cuda()).clone()
    tr = FlowTrainer(model.flow, lr=1e-4)
    zb, eb = rnd(41, 50, 64).cuda(), rnd(42, 50, 64).cuda()
    for _ in range(3):
        tr.step(zb, eb)
    with torch.no_grad():
        y1 = model.synthesize(x0.cuda(), residual=residual.cuda(), embed=embed.cuda())
    fsd = {k: v.detach().cpu() for k, v in model.flow.flow.state_dict().items()}
    dsd = decoder_ref.fold_spectral_norm(T(synth.decoder_state_dict(**meta["synth_dec"])))
    ref = model_ref.synthesize(fsd, dsd, x0, residual, embed, faithful=False)
    err = rel(y1.cpu(), ref)
    print(f"Model.synthesize after training vs oracle on the trained state_dict: {err:.3e}")
    assert err <= TOL and not torch.equal(y0, y1)


def test_refusals():
    import i2v_native
    sd = synth.flow_state_dict(seed=7, n_flows=2, embedding_dim=64, hidden_dim=128)
    x, e = rnd(1, 4, 64).cuda(), rnd(2, 4, 64).cuda()
    flow = _flow(sd, 64, 128, 2, False)
    flow.record_intermediates = True
    with pytest.raises(i2v_native.I2VError, match="record_intermediates"):
        flow(x, e)
    flow.record_intermediates = False
    flow.linear_f16 = 1
    with pytest.raises(i2v_native.I2VError, match="linear_f16"):
        flow(x, e)
    flow.linear_f16 = None
    zt, _ = flow(x, e)
    assert zt.grad_fn is not None
    assert flow(x, e, reverse=True).grad_fn is None            # reverse is never differentiable
    with torch.no_grad():
        assert flow(x, e)[0].grad_fn is None
    with pytest.raises(i2v_native.I2VError, match="linear_f16"):
        i2v_native.NativeFlowTrain(64, 64, 128, 2, 2, linear_f16=1)
    for bad in (dict(hidden_dim=192), dict(hidden_dim=640), dict(in_channels=32), dict(embedding_dim=160), dict(hidden_depth=0)):
        kw = dict(in_channels=64, embedding_dim=64, hidden_dim=128, hidden_depth=2, n_flows=2)
        kw.update(bad)
        with pytest.raises(i2v_native.I2VError, match="unsupported geometry"):
            i2v_native.NativeFlowTrain(**kw)
