"""The cINN training kernels (csrc/i2v_flow_train.hip) unit by unit against float64 at a derived element-wise bound: ``chain_gemm<0>`` with
and without VEC, ``chain_gemm<1>`` with one and two segments, the three ``dw_gemm`` launch groups, ``actnorm_grad``, ``fwd_link``,
``bwd_link`` and ``adam_kernel``, on two-block flows at every hidden width and depth, ragged embedding widths in every control mode,
every flag set and the batch tile edges.

Cases, unit references, bounds, gate and inputs: tests/flow_train_units_common.py (checked on the CPU by
tests/test_host_flow_train_units.py: plain fp32 torch uses at most half of every bound, and every listed deliberate error fails).  One
forward and one backward per case run on ``saved`` and gradient buffers pre-filled with NaN; every unit is then recomputed in float64
from the inputs the GPU itself saved.  What has no unit reference (``d_embed``, the overwritten ``part`` / ``dcin``) is covered by the
end-to-end check against float64 autograd through the oracle at rel-L2 <= 1e-4 per tensor.  The measured maxima are in
profiles/flow_train_units_gate.md."""
import pytest
import torch

import flow_train_units_common as tu
import flow_units_common as fu

pytestmark = pytest.mark.gpu
LEDGER = set()
WORST = {}
_DONE = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(prev)
    # the source of profiles/flow_train_units_gate.md: whatever ran in this session, printed once at its end
    print("\nFLOWTRAINUNITS worst |err| / bound per unit kind:", {k: f"{v:.3f}" for k, v in sorted(WORST.items())})


def _handle(case, grads=None):
    import i2v_native
    h = i2v_native.NativeFlowTrain(64, case["E"], case["hidden"], case["depth"], fu.NFL, control=case["control"], activation=case["act"],
                                   skip_actnorm=case["skip_an"], skip_shuffle=case["skip_sh"])
    P = {k: v.cuda() for k, v in fu.tensors(fu.state_dict(case)).items()}
    h.bind(P, None if grads is None else grads(P))
    return h


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pass(h, case, inp, fill, flat=None, accumulate=False, need=True):
    """forward + backward on buffers filled with ``fill`` -> (saved fp32 [total], zt, logdet, d_x, d_embed, flat gradients), on the CPU"""
    x, e, d_zt, d_ld = (t.cuda() for t in inp)
    B = x.shape[0]
    L = h.saved_layout(B)
    saved = torch.full((L["total"],), fill, dtype=torch.float32, device="cuda")
    if flat is None and h.flat_numel:
        flat = torch.full((h.flat_numel,), fill, dtype=torch.float32, device="cuda")
    zt, ld, sv = h.forward(x, e, saved=saved.view(torch.uint8))
    assert sv.data_ptr() == saved.data_ptr()
    dx, de = h.backward(d_zt, d_ld, sv, flat, accumulate=accumulate, need_dx=need, need_dembed=need)
    return (saved.cpu(), zt.cpu(), ld.cpu(), None if dx is None else dx.cpu(), None if de is None else de.cpu(),
            None if flat is None else flat.cpu()), flat


def _run_of(h, case, out):
    saved, zt, ld, dx, de, flat = out
    B = zt.shape[0]
    grads = {k: flat[h.flat_slices[k][0]:h.flat_slices[k][0] + h.flat_slices[k][1]] for k in tu.grad_keys(case)}
    return tu.Run.from_saved(case, B, h.saved_layout(B), saved, zt, ld, dx, de, grads)


def _unwritten(h, case, flat):
    """The floats of the flat gradient buffer no backward of the case writes: the pads between slices (and ActNorm's slices without ActNorm)"""
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    for k in tu.grad_keys(case):
        keep[h.flat_slices[k][0]:h.flat_slices[k][0] + h.flat_slices[k][1]] = False
    return flat[keep]


def run_case(case):
    """Everything the issue lists for one case, once per process; the failures of the case are collected and asserted once"""
    if case["id"] in _DONE:
        return _DONE[case["id"]]
    fails = []
    x, e, d_zt, d_ld, ref, own, _ = tu.reference(case)
    inp = (x, e, d_zt, d_ld)
    assert own <= tu.OWN_FP32, f"the reference's own fp32 gradients are {own:.3e} from fp64 at a point chosen to be smooth"
    h = _handle(case)
    nan, gflat = _pass(h, case, inp, float("nan"))
    zero, _ = _pass(h, case, inp, 0.0)
    run = _run_of(h, case, nan)
    # NaN-filled buffers: everything finite, the same bits as on zero-filled ones, the unwritten floats keep the sentinel
    names = ("saved", "zt", "logdet", "d_x", "d_embed")
    for name, a, b in zip(names, nan, zero):
        if not bool(torch.isfinite(a).all()):
            fails.append((name, "not finite on NaN-filled buffers"))
        if not torch.equal(_bits(a), _bits(b)):
            fails.append((name, "differs between NaN-filled and zero-filled buffers (or between two runs)"))
    for k in tu.grad_keys(case):
        o, n = h.flat_slices[k]
        if not (bool(torch.isfinite(nan[5][o:o + n]).all()) and torch.equal(_bits(nan[5][o:o + n]), _bits(zero[5][o:o + n]))):
            fails.append((k, "gradient not finite or differs between NaN-filled and zero-filled buffers"))
    if not (bool(torch.isnan(_unwritten(h, case, nan[5])).all()) and bool((_bits(_unwritten(h, case, zero[5])) == 0).all())):
        fails.append(("flat", "a float outside the written gradient slices lost its sentinel"))
    # every unit at its bound
    worst, bad = tu.check_units(run, *inp)
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    fails += bad
    # end to end
    errs, bad = tu.check_e2e(case, run, ref)
    fails += bad
    print(f"FLOWTRAINUNITS {case['id']}: units {({k: round(v, 3) for k, v in sorted(worst.items())})}, end to end worst rel-L2 "
          f"{max(errs.values()):.2e} ({max(errs, key=errs.get)}), reference fp32 {own:.1e}")
    # need_dx / need_dembed off: the same parameter gradients
    off, _ = _pass(h, case, inp, float("nan"), need=False)
    if off[3] is not None or off[4] is not None or not torch.equal(_bits(off[5]), _bits(nan[5])):
        fails.append(("flat", "parameter gradients differ with need_dx / need_dembed off"))
    # bound gradient tensors: the same bits as the flat route
    bound = {}

    def grads(P):
        bound.update({k: torch.full((v.numel(),), float("nan"), dtype=torch.float32, device="cuda") for k, v in P.items() if v.dtype == torch.float32})
        return bound
    hb = _handle(case, grads)
    _pass(hb, case, inp, float("nan"))
    for k in tu.grad_keys(case):
        if not torch.equal(_bits(bound[k].cpu()), _bits(run.grads[k])):
            fails.append((k, "bound gradient tensor differs from the flat route"))
    # accumulate = 1: a second backward of another batch into the same buffer
    inp2 = tu.inputs(case, 1)
    acc, _ = _pass(h, case, inp2, float("nan"), flat=gflat, accumulate=True)
    run2 = _run_of(h, case, acc)
    w, bad = tu.check_accumulate(run, run2, run2.grads, d_ld, inp2[3])
    WORST["accumulate"] = max(WORST.get("accumulate", 0.0), w)
    fails += bad
    if not bool(torch.isnan(_unwritten(h, case, acc[5])).all()):
        fails.append(("flat", "accumulate wrote outside the gradient slices"))
    # rows of a batch against the sample run alone
    if case["group"] == "batch" and case["B"] > 1:
        for b in range(case["B"]):
            one, _ = _pass(h, case, tuple(t[b:b + 1].contiguous() for t in inp), float("nan"))
            if not all(torch.equal(_bits(one[i][0]), _bits(nan[i][b])) for i in (1, 2, 3, 4)):
                fails.append(("rows", f"row {b} of zt / logdet / d_x / d_embed differs from the sample run alone"))
                break
    assert not fails, (case["id"], fails[:8], len(fails))
    LEDGER.update(tu.branches(case))
    _DONE[case["id"]] = True
    return True


def _ids(name):
    return [c["id"] for c in tu.group(name)]


@pytest.mark.parametrize("case", tu.group("hidden"), ids=_ids("hidden"))
def test_hidden_width(case):
    run_case(case)


@pytest.mark.parametrize("case", tu.group("depth"), ids=_ids("depth"))
def test_depth(case):
    run_case(case)


@pytest.mark.parametrize("case", tu.group("embed"), ids=_ids("embed"))
def test_embedding_width_and_control(case):
    run_case(case)


@pytest.mark.parametrize("case", tu.group("flags"), ids=_ids("flags"))
def test_flags(case):
    run_case(case)


@pytest.mark.parametrize("case", tu.group("batch"), ids=_ids("batch"))
def test_batch_tile_edges_and_row_independence(case):
    run_case(case)


def test_ledger_every_branch_ran():
    for name in ("flags", "embed"):
        for case in tu.group(name):
            run_case(case)
    assert tu.LEDGER_WANT <= LEDGER, sorted(tu.LEDGER_WANT - LEDGER)
    print("FLOWTRAINUNITS ledger:", sorted(LEDGER))


def test_misaligned_gradient_tensor_is_refused():
    import i2v_native
    case = tu.group("flags")[0]
    key = tu.lin_key(1, 0, 0) + ".bias"

    def grads(P):
        g = {k: torch.zeros(v.numel(), dtype=torch.float32, device="cuda") for k, v in P.items() if v.dtype == torch.float32}
        g[key] = torch.zeros(g[key].numel() + 4, dtype=torch.float32, device="cuda")[1:1 + g[key].numel()]
        return g
    with pytest.raises(i2v_native.I2VError, match="not 16-byte aligned"):
        _handle(case, grads)


# ---------------------------------------------------------------------------------------------------------------- Adam

@pytest.mark.parametrize("layout,shifts", [("aligned", (0, 0)), ("param_off_4_bytes", (1, 0)), ("grad_off_4_bytes", (0, 1))])
def test_adam_kernel_unit(layout, shifts):
    """``i2v_adam_step`` on a table of tensors of numel 1 .. 4099 cut out of flat buffers with guard floats between them: three
    consecutive steps and one launch at step 1000, each against ``adam_one`` in float64 on the state the GPU itself left.  Without
    amsgrad the table's max_exp_avg_sq is null."""
    import i2v_native
    from i2v_train import _adam_plan
    worst, fails = 0.0, []
    for amsgrad in (False, True):
        for wd in (0.0, 1e-2):
            state, slices = tu.adam_state(*shifts)
            if not amsgrad:
                del state["vm"]
            dev = {k: t.cuda() for k, t in state.items()}
            rows = [tuple(dev[k][slices[k][i][0]:slices[k][i][0] + n] if k in dev else None for k in ("p", "g", "m", "v", "vm"))
                    for i, (_, n) in enumerate(slices["p"])]
            assert all((r[0].data_ptr() % 16 == 4 * shifts[0]) and (r[1].data_ptr() % 16 == 4 * shifts[1]) for r in rows)
            table, chunks = _adam_plan(rows, torch.device("cuda"))
            for step in tu.ADAM_STEPS:
                i2v_native.adam_step(table, chunks, tu.ADAM_HYPER["lr"], tu.ADAM_HYPER["beta1"], tu.ADAM_HYPER["beta2"], tu.ADAM_HYPER["eps"], wd,
                                     amsgrad, step)
                after = {k: t.cpu() for k, t in dev.items()}
                r, bad = tu.adam_check(state, after, slices, tu.adam_scalars(step, wd, **tu.ADAM_HYPER), amsgrad)
                worst, state = max(worst, r), after
                fails += [(amsgrad, wd, step) + tuple(b) for b in bad]
    print(f"FLOWTRAINUNITS adam {layout}: worst |err| / bound {worst:.3f}")
    WORST["adam/" + layout] = worst
    assert not fails, fails[:8]


@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_fused_adam_on_odd_offset_views_and_several_step_counts(amsgrad, weight_decay):
    """``FusedAdam`` over parameters that are views at odd offsets of one flat buffer (7-element tensors among them), gradients
    likewise, one parameter without ``.grad`` on the first step (so the group holds two step counts afterwards): three steps
    against float64 ``torch.optim.Adam``, at the gate of test_fused_adam_vs_fp64 (3 x torch's own fp32-vs-fp64 figure)."""
    from flow_train_common import rel
    from i2v_train import FusedAdam
    shapes = [(7,), (3, 5), (7,), (2049,), (16, 8), (1,), (4099,)]
    gen = torch.Generator().manual_seed(11)
    offs, off = [], 1
    for s in shapes:
        n = int(torch.tensor(s).prod())
        offs.append((off, n))
        off += n + (2 if (off + n) % 2 else 1)          # the next start is odd again
    assert all(o % 2 == 1 for o, _ in offs)
    flat0 = torch.randn(off + 3, generator=gen)
    grads = [[0.3 * torch.randn(s, generator=gen) for s in shapes] for _ in range(3)]
    kw = dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=weight_decay, amsgrad=amsgrad)

    def run(opt_cls, dtype, device):
        flat = flat0.clone().to(dtype).to(device)
        gflat = torch.zeros_like(flat)
        ps = [flat[o:o + n].view(s).requires_grad_(True) for (o, n), s in zip(offs, shapes)]
        opt = opt_cls(ps, **kw)
        for it, gs in enumerate(grads):
            for i, (p, g, (o, n), s) in enumerate(zip(ps, gs, offs, shapes)):
                gflat[o:o + n] = g.reshape(-1).to(dtype).to(device)
                p.grad = None if (it == 0 and i == 2) else gflat[o:o + n].view(s)
            opt.step()
        return flat.detach().cpu(), opt

    f64, _ = run(torch.optim.Adam, torch.float64, "cpu")
    f32, _ = run(torch.optim.Adam, torch.float32, "cpu")
    fgpu, opt = run(FusedAdam, torch.float32, "cuda")
    assert any(k[1] != 0 for k in opt._plans), "the launch per distinct step count did not run"
    inside = torch.zeros(flat0.numel(), dtype=torch.bool)
    for o, n in offs:
        inside[o:o + n] = True
    assert torch.equal(_bits(fgpu[~inside]), _bits(flat0[~inside])), "a float between the parameters changed"
    upd = lambda f: (f.double() - flat0.double())[inside]   # noqa: E731
    noise, err = rel(upd(f32), upd(f64)), rel(upd(fgpu), upd(f64))
    print(f"FLOWTRAINUNITS FusedAdam odd views amsgrad={amsgrad} wd={weight_decay}: torch fp32 vs fp64 {noise:.3e}, fused kernel vs fp64 {err:.3e}")
    assert err <= 3 * noise, (err, noise)
