"""Every native entry on poisoned, guard-banded caller buffers (the contract of DESIGN.md, "Caller-owned buffers"; the harness is
tests/buffer_hygiene_common.py, tried on the CPU by tests/test_host_buffer_hygiene.py).

Each case is a callable that builds a FRESH handle where the entry has one, runs the entry through the binding and returns the tensors the
binding allocated.  It runs three times: plain, with every allocation of the binding guard-banded and pre-filled with 0x00, and with 0xFF
(a NaN in fp16, fp32 and fp64, -1 in an integer).  Asserted per case: no guard byte changed, the three runs return the same bits, nothing
is non-finite on 0xFF that is finite in the plain run; where the family's common module has a float64 oracle for the case, the 0xFF run's
outputs also pass that gate.  Poison is applied at allocation only: nothing is refilled between calls that depend on each other (a decoder
``prepare`` and its ``forward``, a forward with ``save`` and its backward) -- so a backward case also pins that a ``saved`` buffer written into
arbitrary bits gives the bits of one written into zeros, padding and all.

The shapes are the existing case lists' (first and most ragged case per unit list, the smallest fixture per handle); nothing here is
workload-sized.  The heavy read-only inference handles (I3D, Inception, VGG) are loaded once per process and get a fresh workspace cache per
run instead of a fresh handle.  The cINN handles are covered on NaN-filled buffers by test_gpu_flow_units.py and
test_gpu_flow_train_units.py; here they get one guarded run each, for the guard bands only.

``test_reuse_*`` (contract item 4): shape A, a larger shape B, then A again on ONE live handle, the cached workspace refilled with 0xFF
between the steps, each step compared bit for bit with a fresh handle at that shape.  The training modules run in eval() there, so that
the comparison concerns buffers and not the power iteration.  The ledger test at the end keeps the file from passing by guarding nothing."""
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import buffer_hygiene_common as bh
import encoder_cfgs
import encoder_train_common as ec
import fid_common as fc
import flow_train_units_common as tu
import flow_units_common as fu
import gblock_train_common as gc
import i2v_native
import i2v_synth as synth
import i3d_units_common as uc
import lpips_grad_common as lg
import patch_disc_common as pc
import recon_common as rc
import temporal_disc_common as tc
import vgg_common as vc
from stage1_VAE.modules.decoder import GeneratorBlock
from stage1_VAE.modules.patch_disc import NLayerDiscriminator
from stage1_VAE.modules.resnet3D import Discriminator, Encoder
from test_gpu_decoder_configs import CONFIGS as DEC_CONFIGS, ZD as DEC_ZD, _handle as dec_handle, _inputs as dec_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = []            # pytest.param(family, callable, gate or None, number of returned tensors the CALLER owns (updated in place))
STATS = {}            # family -> what run_guarded collected
EXPECT_FOREIGN = {}   # family -> returned tensors that no allocation of the binding holds (the in-place updated inputs), over the guarded runs
FAMILIES = ("patchdisc", "disc3d", "enc3d_train", "gblock_train", "vgg", "inception", "i3d", "decoder", "inference", "recon", "frames", "cinn")
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(prev)


def add(family, name, fn, gate=None, inplace=0):
    assert family in FAMILIES
    CASES.append(pytest.param(family, fn, gate, inplace, id=f"{family}-{name}"))


def by_id(cases, ident):
    return next(c for c in cases if c["id"] == ident)


def dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def ok(name, res):
    passes, ratio, l2 = res
    assert passes, f"float64 gate on the 0xFF run: {name}: |err| / bound {ratio:.3f}, rel-L2 {l2:.2e}"


def own(*shape, dtype=torch.float32, fill=None):
    """A buffer the CALLER hands to an entry (an accumulator, an output slice): taken through the binding's ``torch``, so that under the
    proxy it is guard-banded and poisoned like the binding's own allocations."""
    if fill is None:
        return i2v_native.torch.empty(*shape, dtype=dtype, device=DEV)
    return i2v_native.torch.full(tuple(shape), fill, dtype=dtype, device=DEV)


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


# ================================================================================================================ patch discriminator

def _pd_conv(case):
    x, w, bias, loc, scale = pc.conv_inputs(case)
    ep = case["epilogue"]
    norm, lrelu = ep == "actnorm_lrelu", ep != "bias"

    def run():
        return i2v_native.patchdisc_conv_unit(pc.cl(x).to(DEV), w.to(DEV), bias.to(DEV), loc.to(DEV) if norm else None, scale.to(DEV) if norm else None,
                                              stride=case["stride"], lrelu=lrelu, want_pre=True)

    def gate(outs):
        ref, pre, S, n = pc.conv_oracle(x, w, bias, loc if norm else None, scale if norm else None, case["stride"], lrelu)
        ok("conv", pc.gate(pc.uncl(outs[0].cpu()), ref, S, n))
        Sp = F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=case["stride"], padding=1)
        ok("pre", pc.gate(pc.uncl(outs[1].cpu()), pre, Sp, 16 * case["cin"] + 1))
    return run, gate


def _pd_dgrad(case, frames):
    g, w, act, scale = pc.dgrad_inputs(case)

    def run():
        return i2v_native.patchdisc_dgrad_unit(pc.cl(g).to(DEV), w.to(DEV), case["hw"], pc.cl(act).to(DEV), scale.to(DEV), stride=case["stride"], frames=frames)

    def gate(outs):
        ref, S, n = pc.dgrad_oracle(g, w, act, scale, case["hw"], case["stride"])
        out = outs[0].cpu()
        if not frames:
            out = pc.uncl(out[..., :3] if case["cin"] == 3 else out)
        ok("dgrad", pc.gate(out, ref, S, n))
    return run, gate


def _pd_wgrad(case):
    x, w, _, _, _ = pc.conv_inputs(case)
    g, _, act, scale = pc.dgrad_inputs(case)
    u, v, sigma = pc.power_iteration(w.double().reshape(w.shape[0], -1), pc.randn(case["seed"] + 7, (w.shape[0],)).double(),
                                     pc.randn(case["seed"] + 8, (w[0].numel(),)).double())
    u, v, sigma = u.float(), v.float(), sigma.float().reshape(1)

    def run():
        return i2v_native.patchdisc_wgrad_unit(pc.cl(g).to(DEV), pc.cl(x).to(DEV), w.to(DEV), pc.cl(act).to(DEV), scale.to(DEV), *dev(u, v, sigma),
                                               stride=case["stride"])

    def gate(outs):
        ref, refb, bound, boundb = pc.wgrad_oracle(g, x, w, act, scale, case["stride"], u, v, sigma)
        ok("dW", pc.gate_bound(outs[0].cpu(), ref, bound))
        ok("db", pc.gate_bound(outs[1].cpu().view(1, -1), refb.view(1, -1), boundb.view(1, -1)))
    return run, gate


def _pd_head(case):
    cin, (h, w_), b = case["cin"], case["hw"], case["batch"]
    x = pc.randn(case["seed"], (b, cin, h, w_))
    w = pc.randn(case["seed"] + 1, (1, cin, 4, 4)) * float(np.sqrt(1.0 / (16 * cin)))
    bias, g = pc.randn(case["seed"] + 2, (1,)), pc.randn(case["seed"] + 3, (b, 1, h - 1, w_ - 1))

    def run():
        return i2v_native.patchdisc_head_unit(pc.cl(x).to(DEV), w.to(DEV), bias.to(DEV), g.reshape(b, h - 1, w_ - 1).contiguous().to(DEV))

    def gate(outs):
        ref, _, S, n = pc.conv_oracle(x, w, bias, None, None, 1, False)
        ok("head out", pc.gate(outs[0].cpu().unsqueeze(1), ref, S, n))
        rx, Sx, nx = pc.dgrad_oracle(g, w, None, None, (h, w_), 1)
        ok("head dx", pc.gate(pc.uncl(outs[1].cpu()), rx, Sx, nx))
    return run, gate


def _pd_power(shape):
    rows, cols = shape
    W = pc.randn(44000 + rows, (rows, cols)) * float(np.sqrt(1.0 / cols))
    u0 = F.normalize(pc.randn(44001 + rows, (rows,)), dim=0)
    v0 = F.normalize(pc.randn(44002 + rows, (cols,)), dim=0)

    def run():
        u, v = u0.clone().to(DEV), v0.clone().to(DEV)
        sigma = i2v_native.patchdisc_power_iteration_unit(W.to(DEV), u, v, iterate=True)
        return [sigma, u, v]        # u and v are the caller's, updated in place
    return run


def _pd_actnorm(shape):
    n, h, w, c = shape
    pre = pc.randn(45000 + c, (n * h * w, c)) * 1.7 + 0.4
    return lambda: i2v_native.patchdisc_actnorm_init_unit(pre.to(DEV))


@functools.lru_cache(maxsize=None)
def _pd_state():
    torch.manual_seed(pc.SEED_MODULE)
    return {k: v.clone() for k, v in NLayerDiscriminator(dict(pc.FIXTURE_CFG)).state_dict().items()}


def _pd_net(train):
    net = NLayerDiscriminator(dict(pc.FIXTURE_CFG))
    net.load_state_dict(_pd_state())
    net = net.to(DEV)
    return net.train() if train else net.eval()


def _pd_step(net, x):
    """One saved forward and its backward through the handle -> [pred, dx, parameter gradients]"""
    x = x.to(DEV)
    pred, saved = net._run(x, save=True)
    grads = i2v_native.flat_param_grads(net, DEV)
    d_pred = (torch.cos(torch.arange(pred.numel(), dtype=torch.float64)).view(pred.shape) / pred.numel()).float().to(DEV)
    dx = net._handle(grads).backward(d_pred, saved, tuple(x.shape), need_dx=True, param_grads=True, accumulate=False)
    return [pred, dx, *grads.values()]


_c = pc.conv_cases()
for _case in (_c[0], by_id(_c, "c64-48-s2-33x17-b3")):
    add("patchdisc", "conv-" + _case["id"], *_pd_conv(_case))
add("patchdisc", "dgrad-frames", *_pd_dgrad(by_id(_c, "c3-16-s2-33x17-b3"), True))
add("patchdisc", "dgrad-ragged", *_pd_dgrad(by_id(_c, "c64-48-s2-33x17-b3"), False))
add("patchdisc", "wgrad-ragged", *_pd_wgrad(by_id(pc.wgrad_cases(), "ragged")))
for _case in (pc.HEAD_CASES[0], pc.HEAD_CASES[-1]):
    add("patchdisc", _case["id"], *_pd_head(_case))
for _shape in (pc.POWER_SHAPES[0], pc.POWER_SHAPES[-1]):
    add("patchdisc", f"power-{_shape[0]}x{_shape[1]}", _pd_power(_shape), inplace=2)
for _shape in ((1, 6, 7, 16), (3, 8, 8, 48)):
    add("patchdisc", "actnorm-init-" + "x".join(map(str, _shape)), _pd_actnorm(_shape))
add("patchdisc", "handle-train-step", lambda: _pd_step(_pd_net(True), pc.train_inputs()[0]))


# ================================================================================================================ temporal discriminator

def _st(case):
    return dict(stride_t=case["st"], stride_s=case["ss"])


def _tc_conv(case):
    x, w, _, _ = tc.conv_case_inputs(case)

    def gate(outs):
        ref, S, n = tc.conv_oracle(x, w, case["st"], case["ss"])
        ok("conv", tc.gate(tc.uncl(outs[0].cpu()), ref, S, n))
    return (lambda: i2v_native.disc3d_conv_unit(tc.cl(x).to(DEV), w.to(DEV), **_st(case))), gate


def _tc_dgrad(case):
    _, w, g, act = tc.conv_case_inputs(case)
    in_shape = (case["batch"], case["cin"]) + tuple(case["thw"])
    addt = tc.randn(case["seed"] + 4, in_shape) if case["add"] else None
    add_mask = tc.randn(case["seed"] + 5, in_shape) if case["add_mask"] else None

    def run():
        return i2v_native.disc3d_dgrad_unit(tc.cl(g).to(DEV), w.to(DEV), case["thw"], tc.cl(act).to(DEV) if case["act"] else None,
                                            None if addt is None else tc.cl(addt).to(DEV), None if add_mask is None else tc.cl(add_mask).to(DEV),
                                            frames=case["frames"], **_st(case))

    def gate(outs):
        ref, S, n = tc.dgrad_oracle(g, w, act if case["act"] else None, case["thw"], case["st"], case["ss"], addt, add_mask)
        out = outs[0].cpu()
        if not case["frames"]:
            out = tc.uncl(out[..., :3] if case["cin"] == 3 else out)
        ok("dgrad", tc.gate(out, ref, S, n))
    return run, gate


def _tc_wgrad(case, project):
    x, w, g, act = tc.conv_case_inputs(case)
    u0, v0 = tc.randn(case["seed"] + 6, (w.shape[0],)).double(), tc.randn(case["seed"] + 7, (w[0].numel(),)).double()
    u, v, sigma = tc.power_iteration(w.double().reshape(w.shape[0], -1), u0 / u0.norm(), v0 / v0.norm())
    sn = (u.float(), v.float(), sigma.float()) if project else (None, None, None)

    def run():
        args = dict(act=tc.cl(act).to(DEV), **_st(case))
        if project:
            args.update(u=sn[0].to(DEV), v=sn[1].to(DEV), sigma=sn[2].reshape(1).to(DEV))
        return i2v_native.disc3d_wgrad_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), w.to(DEV), **args)

    def gate(outs):
        ref, bound = tc.wgrad_oracle(g, x, w, act, case["st"], case["ss"], *sn)
        ok("wgrad", tc.gate_bound(outs[0].cpu(), ref, bound))
    return run, gate


def _tc_groupnorm(c, thw, b, res, relu, seed):
    shape = (b, c) + thw
    x = tc.randn(seed, shape) * 2 + 0.5
    w, bias = 1 + 0.3 * tc.randn(seed + 1, (c,)), 0.2 * tc.randn(seed + 2, (c,))
    r = tc.randn(seed + 3, shape) if res else None
    g = tc.randn(seed + 4, shape)

    def run():
        out, stats = i2v_native.disc3d_groupnorm_unit(tc.cl(x).to(DEV), w.to(DEV), bias.to(DEV), None if r is None else tc.cl(r).to(DEV), relu=relu)
        dx, dw, db = i2v_native.disc3d_groupnorm_backward_unit(tc.cl(g).to(DEV), tc.cl(x).to(DEV), stats, w.to(DEV), mask=out if relu else None)
        return [out, stats, dx, dw, db]

    def gate(outs):
        y64, xhat, _ = tc.group_norm(x.double(), w.double(), bias.double())
        S = (xhat * w.double().view(1, -1, 1, 1, 1)).abs() + bias.double().abs().view(1, -1, 1, 1, 1)
        if r is not None:
            y64, S = y64 + r.double(), S + r.double().abs()
        ok("groupnorm", tc.gate(tc.uncl(outs[0].cpu()), torch.relu(y64) if relu else y64, S, 3))
    return run, gate


def _tc_maxpool(thw):
    x = tc.randn(56000 + thw[0], (2, 16) + thw)
    x[0, 0, :, 0:3, 0:3] = 5.0
    ref, idx = F.max_pool3d(x, 3, (1, 2, 2), 1, return_indices=True)
    g = tc.randn(56100 + thw[0], tuple(ref.shape))

    def run():
        out, arg = i2v_native.disc3d_maxpool_unit(tc.cl(x).to(DEV))
        return [out, arg, i2v_native.disc3d_maxpool_backward_unit(tc.cl(g).to(DEV), arg, tuple(tc.cl(x).shape))]

    def gate(outs):
        assert torch.equal(tc.uncl(outs[0].cpu()), ref) and torch.equal(tc.uncl(outs[1].cpu()).long(), idx), "max pool on 0xFF: not torch's bits"
    return run, gate


def _tc_head(c, b):
    x, w, g = tc.randn(57000 + c, (b, c, 1, 4, 4)), tc.randn(57001 + c, (1, c)) * float(c ** -0.5), tc.randn(57002 + c, (b, 1))
    return lambda: i2v_native.disc3d_head_unit(tc.cl(x).to(DEV), w.to(DEV), g.to(DEV))


def _tc_fmap():
    shapes = [(2, 6, 16, 16, 16), (2, 3, 16, 16, 16), (2, 2, 8, 8, 32), (2, 1, 4, 4, 32)]
    a = [tc.randn(58000 + i, s) for i, s in enumerate(shapes)]
    b = [tc.randn(58010 + i, s) for i, s in enumerate(shapes)]

    def run():
        out, grads = i2v_native.disc3d_fmap_loss(dev(*a), dev(*b), "L1", grad_scale=10.0)
        return [out, *grads]
    return run


def _d3_net(cfg, sd, train):
    net = Discriminator(dict(cfg))
    net.load_state_dict(dict(sd))
    net = net.to(DEV)
    return net.train() if train else net.eval()


def _d3_step(net, x, d_pred, d_fmaps):
    x = x.to(DEV)
    grads = i2v_native.flat_param_grads(net, DEV)
    pred, fmaps, saved = net._run(x, save=True, grads=grads)
    dx = net._handle(grads).backward(None if d_pred is None else d_pred.to(DEV), None if d_fmaps is None else [tc.cl(g).to(DEV) for g in d_fmaps], saved, tuple(x.shape),
                                     need_dx=True, param_grads=True, accumulate=False)
    return [pred, *fmaps, dx, *grads.values()]


_c = tc.conv_cases()
for _case in (_c[0], _c[-1], tc.STEM_CASES[1]):
    add("disc3d", "conv-" + _case["id"], *_tc_conv(_case))
_d = tc.dgrad_cases()
add("disc3d", "dgrad-s22-add-addmask", *_tc_dgrad(next(c for c in _d if c["st"] == 2 and c["ss"] == 2 and c["add"] and c["add_mask"])))
add("disc3d", "dgrad-stem-frames", *_tc_dgrad(by_id(_d, "stem-3x10x12-b2-frames-mask")))
add("disc3d", "wgrad-three-ragged", *_tc_wgrad(by_id(tc.wgrad_cases(), "three-ragged"), True))
add("disc3d", "wgrad-stem", *_tc_wgrad(by_id(tc.wgrad_cases(), "stem"), False))
add("disc3d", "groupnorm-c48", *_tc_groupnorm(48, (3, 5, 7), 2, True, True, 55010))
add("disc3d", "groupnorm-multi-slice", *_tc_groupnorm(16, (12, 32, 32), 2, False, True, 55040))
for _thw in ((3, 6, 6), (1, 5, 7)):
    add("disc3d", "maxpool-" + "x".join(map(str, _thw)), *_tc_maxpool(_thw))
for _cb in ((32, 1), (48, 3)):
    add("disc3d", f"head-c{_cb[0]}-b{_cb[1]}", _tc_head(*_cb))
add("disc3d", "fmap-loss", _tc_fmap())
add("disc3d", "sumsq", lambda: i2v_native.disc3d_sumsq(tc.randn(59000, (3, 3, 5, 33, 31)).to(DEV)))
add("disc3d", "handle-train-step",
    lambda: _d3_step(_d3_net(tc.CFG_B, tc.synthetic_state(tc.CFG_B, tc.SEED_B), True), tc.clips_b(), *tc.upstream_b()))
# without d_pred the backward clears the head's gradient buffer (hipMemsetAsync) and the blocks add into it
add("disc3d", "handle-feature-map-gradients-alone",
    lambda: _d3_step(_d3_net(tc.CFG_B, tc.synthetic_state(tc.CFG_B, tc.SEED_B), True), tc.clips_b(), None, tc.upstream_b()[1]))


# ================================================================================================================ encoder training

def _ec_head(case):
    emb, w_mu, b_mu, w_var, b_var, eps, d_s, d_m, d_l = ec.head_inputs(case)

    def run():
        sample, mu, logvar = i2v_native.enc3d_head_forward_unit(*dev(emb, w_mu, b_mu, w_var, b_var, eps))
        back = i2v_native.enc3d_head_backward_unit(*dev(emb, w_mu, w_var), mu, logvar, *dev(eps, d_s, d_m, d_l), kl_scale=0.7)
        return [sample, mu, logvar, *back]

    def gate(outs):
        (mu64, S_mu, n), (lv64, S_lv, _) = ec.head_forward_oracle(emb, w_mu, b_mu, w_var, b_var)
        ok("mu", ec.gate(outs[1].cpu(), mu64, S_mu, n))
        ok("logvar", ec.gate(outs[2].cpu(), lv64, S_lv, n))
        ok("sample", ec.gate(outs[0].cpu(), *ec.sample_oracle(eps, outs[1].cpu(), outs[2].cpu())))
    return run, gate


def _ec_kl():
    _, _, _, _, _, mu, logvar, _, _ = ec.head_inputs(ec.head_cases()[0])
    return lambda: i2v_native.enc3d_kl_backward(*dev(mu, 0.5 * logvar), 1.0)


def _enc_net(cfg, seed):
    net = Encoder(dict(cfg))
    net.load_state_dict(dict(ec.synthetic_state(cfg, seed)))
    net = net.to(DEV)
    net.differentiable = True
    return net


def _enc_step(net, x, eps, coefs):
    """``eps`` None: no sample, the saved eps is cleared on the stream (hipMemsetAsync), the backward gets no d_sample"""
    x, eps = dev(x, eps)
    if eps is None:
        coefs = (None, *coefs[1:])
    grads = i2v_native.flat_param_grads(net, DEV)
    h = net._train_handle(grads)
    sample, mu, logvar, saved = h.forward(x, eps, save=True)
    dx = h.backward(*dev(*coefs), saved, tuple(x.shape), kl_scale=ec.KL_WEIGHT, need_dx=True, param_grads=True, accumulate=False)
    return [sample, mu, logvar, dx, *grads.values()]


def _enc_fixture_a(with_eps=True):
    x, eps, *coefs = ec.inputs(ec.CFG_A, ec.CLIP_A, ec.SEED_A)
    return _enc_step(_enc_net(ec.CFG_A, ec.SEED_A), x, eps if with_eps else None, coefs)


for _case in (ec.head_cases()[0], ec.head_cases()[-1]):
    add("enc3d_train", "head-" + _case["id"], *_ec_head(_case))
add("enc3d_train", "kl-backward", _ec_kl())
add("enc3d_train", "handle-fixture-a", _enc_fixture_a)
add("enc3d_train", "handle-fixture-a-without-eps", lambda: _enc_fixture_a(False))


# ================================================================================================================ GeneratorBlock training

def _gb_modnorm(mode):
    C, B, thw = gc.UNIT_CASES[1]
    g, act, x = gc.unit_inputs(101, C, B, thw)
    rng = np.random.default_rng(151)
    mod = torch.from_numpy(rng.standard_normal((B, thw[1], thw[2], C) if mode == 0 else (B, 2 * C)).astype(np.float32))
    addt = torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32))

    def gate(outs):
        dx64, dg64, db64, S, (Sg, Sb) = gc.modnorm_ref(mode, g, act, x, mod, addt)
        ok("dx", gc.gate(outs[0].cpu(), dx64, S, 4))
        ok("dgamma", gc.gate(outs[1].cpu(), dg64, Sg, 2))
    return (lambda: i2v_native.gblock_train_modnorm_backward_unit(mode, *dev(g, act, x, mod, addt))), gate


def _gb_pointwise():
    cin, B, thw = gc.UNIT_CASES[1]
    cout = 64
    rng = np.random.default_rng(301)
    x = torch.from_numpy(rng.standard_normal((B,) + thw + (cin,)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B,) + thw + (cout,)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32))
    addt = torch.from_numpy(rng.standard_normal((B,) + thw + (cout,)).astype(np.float32))
    u = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    v = torch.from_numpy(rng.standard_normal(cin).astype(np.float32))
    u, v = u / u.norm(), v / v.norm()
    sigma = torch.tensor([float(u.double() @ (w.double() @ v.double()))], dtype=torch.float32)

    def fwd_gate(outs):
        ok("pointwise", gc.gate(outs[0].cpu(), x.double() @ w.double().t() + addt.double(), x.double().abs() @ w.double().abs().t() + addt.abs().double(), cin + 1))
    return ((lambda: i2v_native.gblock_train_pointwise_unit(*dev(x, w, addt))), fwd_gate,
            (lambda: i2v_native.gblock_train_pointwise_wgrad_unit(*dev(g, x, w, u, v, sigma))),
            (lambda: i2v_native.gblock_train_bias_grad_unit(g.to(DEV))))


def _gb_linear():
    C, B = 48, 2
    rng = np.random.default_rng(400 + C + B)
    J, K = 2 * C, 64
    d_lin = torch.from_numpy(rng.standard_normal((B, J)).astype(np.float32))
    z = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal((J, K)).astype(np.float32))
    return lambda: i2v_native.gblock_train_linear_backward_unit(*dev(d_lin, z, w))


def _gb_conv2d(case):
    cin, cout, B, H, W = case
    rng = np.random.default_rng(500 + cin + cout + B)
    x = torch.from_numpy(rng.standard_normal((B, H, W, 4 if cin == 3 else cin)).astype(np.float32))
    if cin == 3:
        x[..., 3] = 0
    g = torch.from_numpy(rng.standard_normal((B, H, W, cout)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32))
    return lambda: i2v_native.gblock_train_conv2d_unit(*dev(x, w, g), want=(True, cin != 3, True))


def _gb_net(cfg, train):
    net = GeneratorBlock(cfg["n_in"], cfg["n_out"], cfg["spectral"], cfg["z_dim"])
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in gc.synthetic_state(cfg).items()})
    net = net.to(DEV)
    net.differentiable = True
    return net.train() if train else net.eval()


def _gb_step(net, cfg):
    x, z, img, c = dev(*gc.inputs(cfg))
    grads = i2v_native.flat_param_grads(net, DEV)
    h = net._train_handle(grads)
    out, saved = h.forward(x, z, img, train=net.training, save=True)
    dx, dz = h.backward(c, z, saved, tuple(x.shape), tuple(img.shape), need_dx=True, need_dz=True, param_grads=True, accumulate=False)
    return [out, dx, dz, *grads.values()]


def _gb_module(tag):
    cfg = gc.FIXTURES[tag]

    def gate(outs):
        golden = gc.load_golden()
        for name, got in zip(("out", "dx", "dz"), outs):
            r = gc.rel(got.cpu(), golden[f"{tag}.{name}"])
            assert r <= gc.TOL_L2, f"float64 gate on the 0xFF run: fixture {tag} {name}: rel-L2 {r:.2e}"
    return (lambda: _gb_step(_gb_net(cfg, True), cfg)), gate


for _mode, _name in ((i2v_native.GBLOCK_TRAIN_SPADE, "spade"), (i2v_native.GBLOCK_TRAIN_ADAIN, "adain")):
    add("gblock_train", "modnorm-backward-" + _name, *_gb_modnorm(_mode))
_pw = _gb_pointwise()
add("gblock_train", "pointwise", _pw[0], _pw[1])
add("gblock_train", "pointwise-wgrad-projected", _pw[2])
add("gblock_train", "bias-grad", _pw[3])
add("gblock_train", "linear-backward", _gb_linear())
for _case in ((3, 128, 2, 5, 6), (128, 48, 1, 4, 4)):
    add("gblock_train", f"conv2d-{_case[0]}to{_case[1]}", _gb_conv2d(_case))
for _tag in ("a", "c"):
    add("gblock_train", "module-fixture-" + _tag, *_gb_module(_tag))


# ================================================================================================================ VGG / LPIPS

@functools.lru_cache(maxsize=None)
def _vgg_loaded():
    h = i2v_native.NativeVGG(device=DEV)
    sd = T(vc.vgg_state_dict(lg.SEED_W))
    sd.update(T(vc.lin_state_dict(lg.SEED_LIN)))
    h.load(sd)
    return h


def _vgg():
    """The process's loaded handle with fresh workspace caches: what a fresh handle would allocate, without packing 15 M weights per run."""
    h = _vgg_loaded()
    h._ws, h._bws = i2v_native._Workspace(), i2v_native._Workspace()
    return h


def _vgg_conv(case):
    x, (w, b) = vc.conv_input(case), vc.conv_params(case)

    def gate(outs):
        ref, S, n = vc.conv_oracle(x, w, b)
        ok("vgg conv", vc.gate(outs[0].cpu().permute(0, 3, 1, 2), ref, S, n))
    return (lambda: i2v_native.vgg_conv_unit(vc.to_cl(x, pad4=case["cin"] == 3).to(DEV), w, b)), gate


def _vgg_pool():
    y = vc.randn(8008, (2, 8, 6, 10))
    g = vc.randn(8009, (2, 8, 3, 5))

    def run():
        yc = vc.to_cl(y).to(DEV)
        return [i2v_native.vgg_maxpool2(yc), i2v_native.vgg_maxpool2_backward(vc.to_cl(g).to(DEV), yc)]

    def gate(outs):
        assert torch.equal(outs[0].cpu().permute(0, 3, 1, 2), vc.maxpool_oracle(y)), "max pool on 0xFF: not torch's bits"
    return run, gate


def _vgg_inputs():
    x = torch.from_numpy(vc.clips(8120, 2, 1, 20, 24))[:, 0].contiguous()
    x2 = torch.from_numpy(vc.clips(8230, 2, 1, 30, 40))[:, 0].contiguous()
    return lambda: [i2v_native.vgg_input_stage(x.to(DEV), i2v_native.VGG_INPUT_LPIPS),
                    i2v_native.vgg_input_stage(x2.to(DEV), i2v_native.VGG_INPUT_DIVERSITY, (17, 23), False)]


def _lpips_layer():
    k, c = 1, vc.CHNS[1]
    f0, f1 = torch.relu(vc.randn(8301, (3, c, 5, 7))), torch.relu(vc.randn(8311, (3, c, 5, 7)))
    f0[0, :, 0, 0] = 0
    lin = torch.from_numpy(vc.lin_state_dict(9)[f"lin{k}.model.1.weight"]).flatten()
    up = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)

    def run():
        a, b = vc.to_cl(f0).to(DEV), vc.to_cl(f1).to(DEV)
        out = own(3, dtype=torch.float64, fill=0.0)
        i2v_native.lpips_layer(a, b, lin.to(DEV), out)
        g0, g1 = i2v_native.lpips_layer_backward(a, b, lin.to(DEV), up.to(DEV))
        return [out, g0, g1]

    def gate(outs):
        ref = vc.lpips_layer_oracle(f0, f1, lin)
        assert float(((outs[0].cpu() - ref).abs() / ref).max()) <= 1e-12, "lpips layer on 0xFF against float64"
    return run, gate


def _pairdiff():
    f = vc.randn(8405, (5, 64 * 9 * 11))

    def run():
        acc = own(2, dtype=torch.float64, fill=0.0)
        i2v_native.vgg_pairdiff_update(f.to(DEV), acc)
        return [acc]
    return run


def _vgg_trunk():
    frames = torch.from_numpy(vc.clips(8600, 2, 1, 16, 16))[:, 0].contiguous()
    frames2 = torch.from_numpy(vc.clips(8601, 2, 1, 16, 16))[:, 0].contiguous()
    tap_grads = [vc.randn(8610 + k, s) for k, s in enumerate(i2v_native.NativeVGG.tap_shapes(2, 16, 16))]

    def run():
        h = _vgg()
        x = i2v_native.vgg_input_stage(frames.to(DEV), i2v_native.VGG_INPUT_LPIPS)
        taps, saved = h.features(x, save=True)
        dx = h.backward(dev(*tap_grads), saved, frames=True)
        taps2 = h.features(i2v_native.vgg_input_stage(frames2.to(DEV), i2v_native.VGG_INPUT_LPIPS))
        return [*taps, dx, h.lpips(taps, taps2)]
    return run


def _vgg_dgrad():
    case = lg.dgrad_cases()[0]
    g, w, addt, y, _ = lg.dgrad_inputs(case)
    cl = lambda t: None if t is None else vc.to_cl(t).to(DEV)  # noqa: E731

    def gate(outs):
        ref, S, n = lg.dgrad_oracle(g, w, addt, y)
        ok("vgg dgrad", vc.gate(lg.to_nchw(outs[0]), ref, S, n))
    return (lambda: i2v_native.vgg_dgrad_unit(cl(g), w, cl(addt), cl(y))), gate


_c = vc.conv_cases()
for _case in (_c[0], max(_c, key=lambda c: (c["hw"] == (17, 33), c["batch"], c["cin"] == 48))):
    add("vgg", "conv-" + _case["id"], *_vgg_conv(_case))
add("vgg", "maxpool-and-backward", *_vgg_pool())
add("vgg", "input-stages", _vgg_inputs())
add("vgg", "lpips-layer-and-backward", *_lpips_layer())
add("vgg", "pairdiff-update", _pairdiff())
add("vgg", "features-saved-backward-lpips-16x16", _vgg_trunk())
add("vgg", "dgrad-unit", *_vgg_dgrad())


# ================================================================================================================ Inception

@functools.lru_cache(maxsize=None)
def _inception_loaded():
    h = i2v_native.NativeInception(device=DEV)
    h.load(T(fc.fid_state_dict(91)))
    return h


def _inc_conv():
    case = next(c for c in fc.conv_cases() if c["slices"])
    x = fc.conv_input(case)
    w, bn = fc.conv_params(case)
    xc = fc.to_cl(x, pad4=case["cin"] == 3)
    wide = torch.full((*xc.shape[:3], xc.shape[3] + 20), 1e30)
    wide[..., 8:8 + xc.shape[3]] = xc
    (kh, kw), s, (ph, pw), (h, wd) = case["kernel"], case["stride"], case["padding"], case["hw"]
    oshape = (x.shape[0], (h + 2 * ph - kh) // s + 1, (wd + 2 * pw - kw) // s + 1, case["cout"] + 16)

    def run():
        out = own(*oshape, fill=-777.0)
        full = i2v_native.inception_conv_unit(wide.to(DEV), w, bn, case["stride"], case["padding"], in_off=8, out=out, out_off=12)
        return [full]

    def gate(outs):
        ref, S, n = fc.conv_oracle(x, w, bn, case["stride"], case["padding"])
        ok("inception conv", fc.gate(outs[0][..., 12:12 + case["cout"]].cpu().permute(0, 3, 1, 2), ref, S, n))
        rest = torch.cat([outs[0][..., :12], outs[0][..., 12 + case["cout"]:]], -1)
        assert bool((rest == -777.0).all()), "the unit wrote outside its channel slice"
    return run, gate


def _inc_pools():
    x = fc.randn(12079, (2, 8, 7, 9))
    xa = fc.randn(12256, (2, 12, 5, 6))
    xg = fc.randn(13068, (2, 768, 5, 7))

    def run():
        return [i2v_native.inception_pool(fc.to_cl(x).to(DEV), fc.POOL_MAX_S2), i2v_native.inception_pool(fc.to_cl(x).to(DEV), fc.POOL_MAX_S1),
                i2v_native.inception_pool(fc.to_cl(xa).to(DEV), fc.POOL_AVG), i2v_native.inception_global_avg(fc.to_cl(xg).to(DEV))]

    def gate(outs):
        assert torch.equal(outs[0].cpu().permute(0, 3, 1, 2), fc.pool_oracle(x, fc.POOL_MAX_S2)[0])
        ok("avg pool", fc.gate(outs[2].cpu().permute(0, 3, 1, 2), *fc.pool_oracle(xa, fc.POOL_AVG)))
        ok("global average", fc.gate(outs[3].cpu(), *fc.global_avg_oracle(xg)))
    return run, gate


def _inc_mixed(block, batch, hw):
    bi = fc.BLOCK_NAMES.index(block)
    x = fc.randn(13000 + bi, (batch, fc.MIXED[bi][2], *hw))
    return lambda: _inception_loaded().mixed(bi, fc.to_cl(x).to(DEV))


add("inception", "conv-unit-sliced", *_inc_conv())
add("inception", "pools-and-global-average", *_inc_pools())
_seen = set()
for (_block, _batch, _hw), _m in zip(fc.MIXED_CASES, fc.MIXED):
    if _m[1] not in _seen:            # one Mixed block per kind A .. E
        _seen.add(_m[1])
        add("inception", f"mixed-{_m[1]}-{_block}", _inc_mixed(_block, _batch, _hw))


# ================================================================================================================ I3D

@functools.lru_cache(maxsize=None)
def _i3d_loaded(variant):
    n = i2v_native.NativeI3D(uc.CLASSES[variant], dt_length=None if variant == "kin" else 16, device=DEV)
    n.load(uc.state_dict(variant))
    return n


def _i3d(variant):
    n = _i3d_loaded(variant)
    n._ws = i2v_native._Workspace()
    return n


def _cl5(x):
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def _i3d_unit(case):
    x = uc.unit_input(case)
    xc = x
    if case["unit"] == uc.UNIT_STEM:
        xc = torch.cat([x, uc.randn(case["seed"] + 7, (x.shape[0], 1, *x.shape[2:]))], 1)

    def gate(outs):
        ref, S, nb = uc.unit_oracle(case["variant"], case["unit"], x)
        ok("i3d unit", uc.gate(outs[0].permute(0, 4, 1, 2, 3).cpu(), ref, S, nb))
    return (lambda: _i3d(case["variant"]).unit_forward(case["unit"], _cl5(xc))), gate


def _i3d_mixed(case):
    i = uc.BLOCKS.index(case["block"])
    B, Tt, H, W = case["shape"]
    x = uc.randn(case["seed"], (B, uc.fc.MIXED[i][1], Tt, H, W))
    return lambda: _i3d(case["variant"]).mixed_forward(i, _cl5(x))


def _i3d_pool(case):
    x = uc.pool_input(case)

    def gate(outs):
        assert torch.equal(outs[0].permute(0, 4, 1, 2, 3).cpu(), uc.maxpool_oracle(case["variant"], x, case["kernel"], case["stride"]))
    return (lambda: _i3d(case["variant"]).maxpool_forward(_cl5(x), case["kernel"], case["stride"])), gate


def _i3d_head(case):
    B, Tt = case["shape"]
    x = uc.randn(case["seed"], (B, 1024, Tt, 7, 7))

    def gate(outs):
        ok("i3d average pool", uc.gate(outs[1].cpu(), *uc.avgpool_oracle(x, case["pool_t"])))
    return (lambda: _i3d(case["variant"]).head_forward(_cl5(x))), gate


_c = uc.unit_cases()
for _case in (_c[0], next(c for c in _c if c["shape"] == uc.M_LADDER[3]), next(c for c in _c if c["unit"] == uc.UNIT_STEM)):
    add("i3d", "unit-" + _case["id"], *_i3d_unit(_case))
add("i3d", "mixed-" + uc.MIXED_CASES[0]["id"], _i3d_mixed(uc.MIXED_CASES[0]))
add("i3d", "maxpool-" + uc.pool_cases()[0]["id"], *_i3d_pool(uc.pool_cases()[0]))
add("i3d", "head-" + uc.HEAD_CASES[1]["id"], *_i3d_head(uc.HEAD_CASES[1]))


# ================================================================================================================ decoder

DEC_MODES = {"mma1": 1, "mma0": 0, "fp16": 3}


@functools.lru_cache(maxsize=None)
def _dec_case(name):
    sd, img, z = dec_inputs(name)
    z2 = torch.randn(2 * img.shape[0], DEC_ZD, generator=torch.Generator().manual_seed(DEC_CONFIGS[name][4] + 2))
    return sd, img, z, z2


def _decoder(name, mode):
    """One fresh handle: forward; two realizations per start frame (a larger workspace: the cache regrows); prepare, then forward on the
    prepared branches.  Nothing is refilled in between.  The range guard must stay clear: the fused-statistics atomics and the range-flag
    slots are where stale workspace contents would show."""
    def run():
        sd, img, z, z2 = _dec_case(name)
        h = dec_handle({"name": name, "sd": sd}, DEC_MODES[mode])
        img_d, z_d, z2_d = dev(img, z, z2)
        out = h.forward(img_d, z_d)
        real = h.forward(img_d, z2_d, realizations=2)
        h.prepare(img_d)
        prepared = h.forward(img_d, z_d)
        torch.cuda.synchronize()
        assert h.status() == 0, (name, mode, "the range guard is set")
        return [out, real, prepared]

    def gate(outs):
        assert bh.same_bits(outs[0], outs[2]), "the forward on prepared SPADE branches differs from the plain forward"
    return run, gate


for _name in ("nf8_s4", "nf24_p11"):
    for _mode in DEC_MODES:
        add("decoder", f"{_name}-{_mode}", *_decoder(_name, _mode))


# ================================================================================================================ other inference handles

CFG_INF = dict(n_in=64, n_out=32, spectral=True, z_dim=8, B=2, map=(2, 8, 8), img=(16, 16), seed=31)     # test_gpu_gblock_train.CFG_INF
ENC3D_CASE = encoder_cfgs.CASES["c0_16"]                                                                  # the minimum width everywhere


def _gblock_inf(cfg=CFG_INF):
    h = i2v_native.NativeGBlock(cfg["n_in"], cfg["n_out"], cfg["z_dim"], cfg["spectral"], device=DEV)
    h.load(T(gc.synthetic_state(cfg)))
    x, z, img, _ = dev(*gc.inputs(cfg))
    out = h.forward(x, z, img)
    assert h.status() == 0
    return [out]


@functools.lru_cache(maxsize=None)
def _embedder_sd():
    return T(synth.embedder_state_dict(seed=3, z_dim=64, norm="in"))


def _embedder(batch=1, hw=(64, 64)):
    h = i2v_native.NativeEmbedder(64, False, device=DEV)
    h.load(_embedder_sd())
    x = 2 * torch.rand(batch, 3, *hw, generator=torch.Generator().manual_seed(9)) - 1
    return [h.forward(x.to(DEV))]


@functools.lru_cache(maxsize=None)
def _enc3d_sd():
    return T(synth.encoder3d_state_dict(**ENC3D_CASE["synth"]))


def _encoder3d(batch=1, frames=16):
    a = ENC3D_CASE["synth"]
    h = i2v_native.NativeEncoder3D(a["z_dim"], a["channels"], a["stride_s"], ENC3D_CASE["stride_t"], device=DEV)
    h.load(_enc3d_sd())
    g = torch.Generator().manual_seed(7)
    x = torch.randn(batch, 3, frames, 64, 64, generator=g).tanh()
    eps = torch.randn(batch, a["z_dim"], generator=g)
    return list(h.forward(x.to(DEV), eps.to(DEV)))


def _mlp():
    g = torch.Generator().manual_seed(11)
    sd = {f"main.{2 * i}.{p}": torch.randn(*s, generator=g) * 0.3
          for i, (o, k) in enumerate(((16, 8), (16, 16), (8, 16))) for p, s in (("weight", (o, k)), ("bias", (o,)))}
    h = i2v_native.NativeMLP(8, 16, 1, 8, device=DEV)
    h.load(sd)
    return [h.forward(torch.randn(5, 8, generator=torch.Generator().manual_seed(1)).to(DEV))]


add("inference", "gblock", _gblock_inf)
add("inference", "embedder", _embedder)
add("inference", "encoder3d", _encoder3d)
add("inference", "mlp", _mlp)


# ================================================================================================================ recon, KL, frames

def _recon_strided():
    real, gen = rc.pair(77, (2, 5, 3, 16, 23), 0.1)

    def run():
        seq, out = real.to(DEV), gen.to(DEV)
        return list(i2v_native.recon_stats(seq[:, 1:], out[:, :4], 2.0)[:2])
    return run


def _recon_range():
    shape = (1, 1, 3, 11, 11)
    name, real, gen = rc.families(100 + shape[-1], shape)[0]

    def gate(outs):
        ref = rc.oracle(real, gen, None)
        s = outs[0].cpu()
        assert rc.all_ok(rc.check_scalars({"l1": s[0], "mse": s[1], "psnr": s[2], "ssim": s[3]}, ref, verbose=False)), "recon scalars on 0xFF against float64"
    return (lambda: list(i2v_native.recon_stats(real.to(DEV), gen.to(DEV)))), gate


def _kl():
    g = torch.Generator().manual_seed(603)
    mu, lv = torch.randn(3, 64, generator=g), 0.5 * torch.randn(3, 64, generator=g) - 0.3

    def gate(outs):
        want, bound = rc.kl_oracle(mu, lv)
        assert rc.gate("KL", outs[0], want, bound, verbose=False)[0], "KL on 0xFF against float64"
    return (lambda: [i2v_native.kl_normal(mu.to(DEV), lv.to(DEV))]), gate


def _frames():
    n, k, t, h, w = 2, 1, 2, 4, 1                        # the smallest geometry of test_gpu_frames.GEOMS
    x = torch.tanh(3.0 * torch.randn(n, t, 3, h, w, generator=torch.Generator().manual_seed(n + k)))

    def run():
        xd = x.to(DEV)
        peak = i2v_native.frames_peak(xd)
        return [peak, i2v_native.frames_to_u8(xd, peak), i2v_native.frames_to_u8(xd), i2v_native.frames_to_u8(xd, mode="unit", layout="clips")]

    def gate(outs):
        assert float(outs[0]) == float(x.max()) and torch.equal(outs[1], outs[2])
        want = torch.clamp(x * 0.5 + 0.5, 0.0, 1.0).mul(255).add(0.5).clamp(0, 255).movedim(-3, -1).to(torch.uint8)
        assert torch.equal(outs[3].cpu(), want), "unit-mode bytes on 0xFF"
    return run, gate


add("recon", "stats-strided-view", _recon_strided())
add("recon", "stats-range-from-the-data", *_recon_range())
add("recon", "kl-normal", *_kl())
add("frames", "peak-and-u8-smallest-geometry", *_frames())


# ================================================================================================================ cINN (guard bands only)

FLOW_CASE = min(fu.CASES, key=lambda c: (c["hidden"], c["depth"], c["E"]))


def _flow():
    c = FLOW_CASE
    h = i2v_native.NativeFlow(64, c["E"], c["hidden"], c["depth"], fu.NFL, control=c["control"], device=DEV)
    h.load(fu.tensors(fu.state_dict(c)))
    g = torch.Generator().manual_seed(2)
    x, e = torch.randn(5, 64, generator=g).to(DEV), torch.randn(5, c["E"], generator=g).abs().to(DEV)
    zt, logdet = h.forward(x, e)
    return [zt, logdet, h.inverse(zt, e)]


def _flow_train():
    c = tu.CASES[0]
    h = i2v_native.NativeFlowTrain(64, c["E"], c["hidden"], c["depth"], fu.NFL, control=c["control"], activation=c["act"], skip_actnorm=c["skip_an"],
                                   skip_shuffle=c["skip_sh"], device=DEV)
    h.bind({k: v.to(DEV) for k, v in fu.tensors(fu.state_dict(c)).items()})
    x, e, d_zt, d_ld = dev(*tu.inputs(c, 0))
    zt, logdet, saved = h.forward(x, e)
    flat = own(h.flat_numel, fill=0.0)       # the pads between the gradient slices stay as they are: zeros here, so that they compare
    dx, de = h.backward(d_zt, d_ld, saved, flat, need_dx=True, need_dembed=True)
    return [zt, logdet, dx, de, flat]


add("cinn", "flow-forward-inverse", _flow)
add("cinn", "flow-train-forward-backward", _flow_train)


# ================================================================================================================ the tests

FAULT_WORDS = ("illegal memory access", "hipErrorIllegalAddress", "hipErrorLaunchFailure", "unspecified launch failure", "HSA_STATUS_ERROR")


def stops_on_fault(test):
    """After a GPU fault the context is gone and every later launch on it is noise: the session ends at the first one."""
    @functools.wraps(test)
    def wrapper(*args, **kwargs):
        try:
            return test(*args, **kwargs)
        except (RuntimeError, i2v_native.I2VError) as e:
            if any(w in str(e) for w in FAULT_WORDS):
                pytest.exit(f"GPU fault in {test.__name__}, nothing more is started: {e}", returncode=3)
            raise
    return wrapper


@pytest.mark.parametrize("family,fn,gate,inplace", CASES)
@stops_on_fault
def test_entry_on_poisoned_guard_banded_buffers(family, fn, gate, inplace, monkeypatch, request):
    stats = STATS.setdefault(family, {})
    outs = bh.run_three(fn, i2v_native, monkeypatch, request.node.callspec.id, stats)
    EXPECT_FOREIGN[family] = EXPECT_FOREIGN.get(family, 0) + 2 * inplace
    if gate is not None:
        gate(outs)
    print(f"  HYGIENE {request.node.callspec.id}: {len(outs)} tensors, 3 runs agree bit for bit, guards intact; workspace / saved bytes as reported "
          f"{stats['last_uint8']}{'; float64 gate passed on the 0xFF run' if gate is not None else ''}")


def _poison(handle):
    """Refill the cached workspaces of a live handle between two independent calls"""
    for ws in (getattr(handle, "_ws", None), getattr(handle, "_bws", None)):
        if ws is not None and ws.buf is not None:
            ws.buf.fill_(0xFF)


def _reuse(make, step, shapes, handle_of):
    """A, B, A on one live handle (its workspace poisoned before each step) against a fresh handle per step."""
    live = make()
    for tag in ("A", "B", "A"):
        _poison(handle_of(live))
        got = [t.clone() for t in bh.flat(step(live, shapes[tag]))]
        want = bh.flat(step(make(), shapes[tag]))
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert bh.same_bits(a, b), f"handle reuse across shapes: step {tag}, output {i} {tuple(a.shape)} differs from a fresh handle's"


@stops_on_fault
def test_reuse_patch_discriminator():
    """A = e32 (2 x 32 x 32), B = e24x40 (3 x 24 x 40): one more sample, the larger workspace."""
    shapes = {"A": pc.eval_inputs("e32"), "B": pc.eval_inputs("e24x40")}
    _reuse(lambda: _pd_net(False), _pd_step, shapes, lambda net: net._handle())


@stops_on_fault
def test_reuse_temporal_discriminator():
    """CFG_A ends on [1, 4, 4] for every clip length at 64 x 64: A = 2 clips of 5 frames, B = 3 clips of 12 (with the fixture's parameters
    replaced by the seeded synthetic ones: the comparison is between handles, not with a fixture)."""
    sd = tc.synthetic_state(tc.CFG_A, tc.SEED_A)
    shapes = {"A": tc.clips_a_eval(5), "B": tc.randn(tc.SEED_A_DATA + 40, (3, 3, 12, 64, 64))}

    def step(net, x):
        n = x.shape[0]
        return _d3_step(net, x, tc.randn(5150 + n, (n, 1)), None)
    _reuse(lambda: _d3_net(tc.CFG_A, sd, False), step, shapes, lambda net: net._handle())


@stops_on_fault
def test_reuse_encoder_training():
    """CFG_B takes 8 x 8 frames from two frames on: A = CLIP_B2 (2 clips of 2 frames), B = 3 clips of 4 frames."""
    shapes = {"A": ec.CLIP_B2, "B": (3, 3, 4, 8, 8)}

    def step(net, clip):
        x, eps, *coefs = ec.inputs(ec.CFG_B, clip, ec.SEED_B)
        return _enc_step(net, x, eps, coefs)
    _reuse(lambda: _enc_net(ec.CFG_B, ec.SEED_B), step, shapes, lambda net: net._train_handle())


@stops_on_fault
def test_reuse_generator_block_training():
    """A = fixture a's geometry (2 x 3 x 5 x 6), B = 3 samples on the next larger map of UNIT_CASES (2 x 8 x 8)."""
    cfg = gc.FIXTURES["a"]
    shapes = {"A": cfg, "B": dict(cfg, B=3, map=(2, 8, 8))}
    _reuse(lambda: _gb_net(cfg, False), _gb_step, shapes, lambda net: net._train_handle())


@stops_on_fault
def test_reuse_decoder():
    """nf8_s4 in split-fp16 mode: B = 2, then 3 samples with two realizations each (the larger workspace), then B = 2 again; no prepare is
    outstanding when the workspace is refilled."""
    sd, img, z, _ = _dec_case("nf8_s4")
    g = torch.Generator().manual_seed(4)
    img3, z6 = 2 * torch.rand(3, *img.shape[1:], generator=g) - 1, torch.randn(6, DEC_ZD, generator=g)

    def step(h, which):
        out = h.forward(*dev(img, z)) if which == "A" else h.forward(*dev(img3, z6), realizations=2)
        torch.cuda.synchronize()
        assert h.status() == 0
        return [out]
    _reuse(lambda: dec_handle({"name": "nf8_s4", "sd": sd}, 1), step, {"A": "A", "B": "B"}, lambda h: h)


@stops_on_fault
def test_reuse_inference_gblock():
    shapes = {"A": CFG_INF, "B": dict(CFG_INF, B=3, map=(4, 8, 8))}

    def make():
        h = i2v_native.NativeGBlock(CFG_INF["n_in"], CFG_INF["n_out"], CFG_INF["z_dim"], CFG_INF["spectral"], device=DEV)
        h.load(T(gc.synthetic_state(CFG_INF)))
        return h

    def step(h, cfg):
        x, z, img, _ = dev(*gc.inputs(cfg))
        return [h.forward(x, z, img)]
    _reuse(make, step, shapes, lambda h: h)


@stops_on_fault
def test_reuse_encoder3d_and_embedder():
    a = ENC3D_CASE["synth"]

    def make_enc():
        h = i2v_native.NativeEncoder3D(a["z_dim"], a["channels"], a["stride_s"], ENC3D_CASE["stride_t"], device=DEV)
        h.load(_enc3d_sd())
        return h

    def step_enc(h, shape):
        g = torch.Generator().manual_seed(70 + shape[0])
        x, eps = torch.randn(shape[0], 3, shape[1], 64, 64, generator=g).tanh(), torch.randn(shape[0], a["z_dim"], generator=g)
        return list(h.forward(x.to(DEV), eps.to(DEV)))
    _reuse(make_enc, step_enc, {"A": (1, 8), "B": (2, 16)}, lambda h: h)

    def make_emb():
        h = i2v_native.NativeEmbedder(64, False, device=DEV)
        h.load(_embedder_sd())
        return h

    def step_emb(h, shape):
        x = 2 * torch.rand(shape[0], 3, *shape[1:], generator=torch.Generator().manual_seed(90 + shape[0])) - 1
        return [h.forward(x.to(DEV))]
    _reuse(make_emb, step_emb, {"A": (1, 64, 64), "B": (2, 64, 128)}, lambda h: h)


@stops_on_fault
def test_reuse_vgg():
    """Features with save, backward and LPIPS at 16 x 16, then 3 images at 20 x 24, then 16 x 16 again, on one handle's two workspace caches."""
    def make():
        h = i2v_native.NativeVGG(device=DEV)
        sd = T(vc.vgg_state_dict(lg.SEED_W))
        sd.update(T(vc.lin_state_dict(lg.SEED_LIN)))
        h.load(sd)
        return h

    def step(h, shape):
        n, hh, w = shape
        frames = torch.from_numpy(vc.clips(8700 + n, n, 1, hh, w))[:, 0].contiguous()
        x = i2v_native.vgg_input_stage(frames.to(DEV), i2v_native.VGG_INPUT_LPIPS)
        taps, saved = h.features(x, save=True)
        grads = [vc.randn(8710 + k, s).to(DEV) for k, s in enumerate(h.tap_shapes(n, hh, w))]
        return [*taps, h.backward(grads, saved, frames=True)]
    live = make()
    fresh = make()        # packing the weights is the cost here: one second handle serves as "fresh" with new workspace caches per step
    for tag, shape in (("A", (2, 16, 16)), ("B", (3, 20, 24)), ("A", (2, 16, 16))):
        _poison(live)
        fresh._ws, fresh._bws = i2v_native._Workspace(), i2v_native._Workspace()
        got, want = [t.clone() for t in step(live, shape)], step(fresh, shape)
        for i, (a, b) in enumerate(zip(got, want)):
            assert bh.same_bits(a, b), f"handle reuse across shapes: step {tag}, output {i} differs from a fresh workspace's"


def test_ledger_every_family_was_guarded():
    """Run behind the cases above (the pattern of test_gpu_dec_units.test_ledger_every_unit_on_every_kernel): every family of FAMILIES
    contributed guarded runs, at least one uint8 allocation (a workspace or a ``saved`` buffer) lay between guard bands, and every
    returned tensor lived in an allocation the proxy made -- but the caller-owned vectors that the power-iteration unit updates in place."""
    print("HYGIENE ledger:", {f: dict(s, foreign_expected=EXPECT_FOREIGN.get(f, 0)) for f, s in sorted(STATS.items())})
    print(f"HYGIENE wall time of the module so far: {time.time() - T0:.1f} s")
    for family in FAMILIES:
        s = STATS.get(family)
        assert s and s["runs"] >= 2, f"{family}: no guarded run"
        assert s["uint8"] >= 1, f"{family}: no workspace or saved buffer was guarded"
        assert s["foreign"] == EXPECT_FOREIGN.get(family, 0), f"{family}: {s['foreign']} returned tensors outside the proxy's allocations"
