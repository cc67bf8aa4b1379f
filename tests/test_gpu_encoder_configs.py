"""The motion encoder (csrc/i2v_encoder.hip) and the conditioning embedder (csrc/i2v_embed.hip) through their public entry points, at the
configurations of tests/encoder_cfgs.py: every first-block kernel path, widths from 16 to 1024, batches of 1, 2, 3 and 5, single-frame
strided layers -- against the float64 oracle and, where the reference can build the configuration, its own module's outputs
(tests/golden/enc3d_cfgs.npz).  test_host_encoder_configs.py pins the oracle to the reference and shows that a dropped tap, channel or
image row moves mu by > 1e-3; the gate here is 1e-4."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import encoder_cfgs as ec
import i2v_native
import i2v_synth as synth
from conftest import load_golden, rel_l2
from i2v_native import I2VError
from test_host_encoder_configs import clip, oracle64

pytestmark = pytest.mark.gpu
TOL = 1e-4


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()  # fails loudly if libi2v_hip.so is missing
    torch.set_grad_enabled(False)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(clip fp32, mu float64, logvar float64) of a case: the float64 oracle, computed once and shared (never written to)."""
    case = ec.CASES[name]
    x = clip(case)
    mu, logvar = oracle64(case, x=x.double())
    return x, mu, logvar


def config(case, **over):
    a = case["synth"]
    dic = {"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": a["z_dim"], "channels": a["channels"],
           "stride_s": a["stride_s"], "stride_t": case["stride_t"]}
    dic.update(over)
    return dic


def encoder(name):
    from stage1_VAE.modules.resnet3D import Encoder
    case = ec.CASES[name]
    enc = Encoder(config(case))
    enc.load_state_dict(T(synth.encoder3d_state_dict(**case["synth"])))
    return enc.cuda().eval()


def handle(name, **over):
    """The raw native handle of a case (``over``: synthesiser / configuration arguments replaced)."""
    case = ec.CASES[name]
    a = dict(case["synth"], **{k: v for k, v in over.items() if k != "stride_t"})
    h = i2v_native.NativeEncoder3D(a["z_dim"], a["channels"], a["stride_s"], over.get("stride_t", case["stride_t"]))
    h.load(T(synth.encoder3d_state_dict(**a)))
    return h


def gate(what, got, want):
    """Relative L2 < TOL per batch row and over the whole tensor; returns the whole-tensor error."""
    got, want = got.detach().cpu().double(), want.double()
    rows = [rel_l2(got[b], want[b]) for b in range(want.shape[0])]
    whole = rel_l2(got, want)
    assert max(rows) < TOL and whole < TOL, (what, whole, rows)
    return whole


@pytest.mark.parametrize("name", ec.ALL_NAMES)
def test_encoder_parity(name):
    """mu and logvar vs the float64 oracle (all cases; c0_16 and c0_80 have no other pin: the reference's stem is 64 wide) and vs the
    reference module's fp32 outputs (cases 1-9)."""
    x, mu64, lv64 = reference(name)
    _, mu, logvar = encoder(name)(x.cuda())
    assert mu.shape == mu64.shape == (x.shape[0], ec.Z_DIM) and bool(torch.isfinite(mu).all() and torch.isfinite(logvar).all())
    e_mu, e_lv = rel_l2(mu.cpu(), mu64), rel_l2(logvar.cpu(), lv64)
    line = f"encoder {name}: HIP vs fp64 oracle  mu {e_mu:.2e}  logvar {e_lv:.2e}"
    g = None
    if name in ec.REF_NAMES:
        g, _ = load_golden("enc3d_cfgs")
        line += f"; vs reference module  mu {rel_l2(mu.cpu(), g[name + '_mu']):.2e}  logvar {rel_l2(logvar.cpu(), g[name + '_logvar']):.2e}"
    print(line)
    gate(name + " mu", mu, mu64)
    gate(name + " logvar", logvar, lv64)
    if g is not None:
        gate(name + " mu vs reference", mu, torch.from_numpy(g[name + "_mu"]))
        gate(name + " logvar vs reference", logvar, torch.from_numpy(g[name + "_logvar"]))


@pytest.mark.parametrize("name", ["nodown_l0", "t3"])
def test_encoder_sample(name):
    """sample = eps * exp(0.5 logvar) + mu (resnet3D.py:202-206), through the handle with a given eps and through Encoder.forward,
    which draws eps on the CPU generator."""
    x, mu64, lv64 = reference(name)
    B = x.shape[0]
    h = handle(name)
    eps = torch.randn(B, ec.Z_DIM, generator=torch.Generator().manual_seed(7))
    sample, mu, logvar = h.forward(x.cuda(), eps.cuda())
    e = gate(name + " sample", sample, mu64 + eps.double() * torch.exp(0.5 * lv64))
    print(f"encoder {name}: sample vs fp64 oracle {e:.2e}")
    none, mu_b, logvar_b = h.forward(x.cuda())
    assert none is None and torch.equal(mu_b, mu) and torch.equal(logvar_b, logvar)
    # Encoder.forward: the sample against the returned mu / logvar in float64.  The kernel evaluates fmaf(eps, expf(0.5f * logvar), mu):
    # the halving is exact, expf, the product and the fused add round once each -- 4 * 2^-24 of the magnitudes that meet covers them.
    enc = encoder(name)
    torch.manual_seed(1234 + B)
    sample, mu, logvar = enc(x.cuda())
    torch.manual_seed(1234 + B)
    eps = torch.randn(B, ec.Z_DIM).double()
    mu, logvar = mu.cpu().double(), logvar.cpu().double()
    std = torch.exp(0.5 * logvar)
    delta = (sample.cpu().double() - (mu + eps * std)).abs()
    bound = 4 * 2.0 ** -24 * (mu.abs() + eps.abs() * std)
    print(f"encoder {name}: Encoder.forward sample, max |delta| / bound {float((delta / bound).max()):.3f}")
    assert bool((delta <= bound).all())
    gate(name + " mu (forward)", mu, mu64)


def test_encoder_input_forms():
    """[B,T,3,H,W] is transposed like the reference does (resnet3D.py:209-210), and a strided view is read like its contiguous copy."""
    x, mu64, _ = reference("t8")
    enc = encoder("t8")
    _, mu, logvar = enc(x.cuda())
    gate("t8 mu", mu, mu64)
    _, mu_t, logvar_t = enc(x.transpose(1, 2).contiguous().cuda())
    assert x.shape[2] > 3 and torch.equal(mu_t, mu) and torch.equal(logvar_t, logvar)
    wide = torch.zeros(*x.shape[:-1], 2 * x.shape[-1], device="cuda")
    wide[..., ::2] = x.cuda()
    view = wide[..., ::2]
    assert not view.is_contiguous()
    _, mu_v, logvar_v = enc(view)
    assert torch.equal(mu_v, mu) and torch.equal(logvar_v, logvar)


def test_encoder_refusals():
    """What the encoder cannot run is an error before anything is launched, and leaves the process able to run what it can."""
    from stage1_VAE.modules.resnet3D import Encoder
    case = ec.CASES["t8"]
    x, mu64, lv64 = reference("t8")
    xc = x[:1].cuda()
    # a temporal stride without a downsample branch for the half-rate residual: refused when the handle is created (the reference
    # fails in `out += residual`), naming the layer -- and by the module's constructor
    bad = dict(channels=[64, 64, 32, 48, 64], stride_s=[1, 2, 2, 2], stride_t=[2, 2, 2, 1])
    with pytest.raises(I2VError, match="layer 0"):
        i2v_native.NativeEncoder3D(ec.Z_DIM, bad["channels"], bad["stride_s"], bad["stride_t"])
    with pytest.raises(ValueError, match="layer 0"):
        Encoder(config(case, **bad))
    with pytest.raises(I2VError, match="layer 2"):   # the same in a later layer; its T == 1 form is refused with it
        i2v_native.NativeEncoder3D(ec.Z_DIM, [64, 32, 48, 48, 64], [2, 2, 1, 2], [2, 2, 2, 2])
    enc = encoder("t8")
    with pytest.raises(I2VError, match="12 input frames"):        # stem T = 6
        enc(x[:1, :, :1].repeat(1, 1, 12, 1, 1).cuda())
    for frames in (1, 2):   # dim 1 (3) > dim 2: transposed like the reference does, which leaves a 1- or 2-channel clip
        with pytest.raises(I2VError, match="expected x"):
            enc(xc[:, :, :frames])
    for channels in ([96, 32, 32, 48, 64],    # stem weights beyond the LDS bound
                     [64, 24, 32, 48, 64]):   # not a multiple of 16
        with pytest.raises(I2VError, match="i2v_encoder3d_create"):
            i2v_native.NativeEncoder3D(ec.Z_DIM, channels, case["synth"]["stride_s"], case["stride_t"])
    with pytest.raises(I2VError, match="power of two >= 64"):
        enc(xc[..., :32, :32])
    with pytest.raises(I2VError, match=r"feature map is \[1,4,8\]"):
        enc(torch.cat((xc, xc), dim=-1))                              # 64 x 128 frames
    with pytest.raises(I2VError, match=r"feature map is \[1,8,8\]"):
        handle("t8", channels=[64, 32, 48, 64, 64], stride_s=[1, 1, 2, 2]).forward(xc)
    with pytest.raises(I2VError, match="expected eps"):
        enc.native().forward(xc, torch.zeros(1, ec.Z_DIM - 1, device="cuda"))
    # a workspace one byte short, through the raw C ABI
    lib = i2v_native.lib()
    a = case["synth"]
    cfg = i2v_native.Enc3dCfg(a["z_dim"], (ctypes.c_int32 * 5)(*a["channels"]), (ctypes.c_int32 * 4)(*a["stride_s"]),
                              (ctypes.c_int32 * 4)(*case["stride_t"]), 0)
    h = ctypes.c_void_p()
    assert lib.i2v_encoder3d_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.i2v_last_error()
    try:
        tensors, keep = i2v_native._pack_state_dict(synth.encoder3d_state_dict(**a))
        assert lib.i2v_encoder3d_load(h, tensors, len(tensors)) == 0, lib.i2v_last_error()
        B, _, Tn, H, W = x.shape
        nbytes = lib.i2v_encoder3d_workspace_bytes(h, B, Tn, H, W)
        assert nbytes > 0 and lib.i2v_encoder3d_workspace_bytes(h, 0, Tn, H, W) == 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        xg = x.cuda()
        mu, logvar = torch.empty(B, ec.Z_DIM, device="cuda"), torch.empty(B, ec.Z_DIM, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = (h, xg.data_ptr(), Tn, H, W, None, None, mu.data_ptr(), logvar.data_ptr(), ws.data_ptr())
        assert lib.i2v_encoder3d_forward(*args, nbytes - 1, B, st) != 0
        assert b"workspace" in lib.i2v_last_error()
        assert lib.i2v_encoder3d_forward(*args[:6], mu.data_ptr(), *args[7:], nbytes, B, st) != 0   # a sample without eps
        assert lib.i2v_encoder3d_forward(*args, nbytes, B, st) == 0, lib.i2v_last_error()
        torch.cuda.synchronize()
        gate("t8 mu (C ABI)", mu, mu64)
        gate("t8 logvar (C ABI)", logvar, lv64)
    finally:
        lib.i2v_encoder3d_destroy(h)
    # and the module that met the refusals still computes the case
    _, mu, logvar = enc(x.cuda())
    gate("t8 mu after the refusals", mu, mu64)
    gate("t8 logvar after the refusals", logvar, lv64)


@pytest.mark.parametrize("norm,h,w,batch", [("in", 64, 128, 2), ("bn", 128, 64, 1), ("in", 256, 256, 1), ("bn", 64, 64, 5), ("bn", 256, 64, 3)])
def test_embedder_shapes(norm, h, w, batch):
    """ResnetEncoder.encode(x).mode() at non-square frames (the bricks of the strided fp32 kernel: 7x7/2 stem, 3x3/2 conv, 1x1/2
    downsample), 256^2 and batches of 1, 2, 3, 5, vs the float64 evaluation of the (unpinned, see oracle/embedder_ref.py) restatement.
    BatchNorm (eval) is well conditioned: 1e-4 per row and whole (the oracle's own fp32 evaluation sits 4e-7 from fp64).  InstanceNorm
    over the small maps of the last stages is not: the rule of test_gpu_parity.test_embedder_vs_oracle, 1e-4 or 3x the oracle's own fp32
    noise."""
    from oracle import embedder_ref
    from stage2_cINN.AE.modules.AE import ResnetEncoder
    sd = T(synth.embedder_state_dict(seed=3, z_dim=64, norm=norm))
    enc = ResnetEncoder({"z_dim": 64, "deterministic": False, "in_size": h, "encoder_type": "resnet50", "norm": norm})
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    x = 2 * torch.rand(batch, 3, h, w, generator=torch.Generator().manual_seed(9)) - 1
    ref32 = embedder_ref.encode_mode(sd, x, norm)
    sd64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}
    ref64 = embedder_ref.encode_mode(sd64, x.double(), norm)
    out = enc.encode(x.cuda()).mode()
    assert out.shape == (batch, 64, 1, 1)
    noise, err = rel_l2(ref32, ref64), rel_l2(out.cpu(), ref64)
    rows = [rel_l2(out[b].cpu(), ref64[b]) for b in range(batch)]
    print(f"embedder {norm} {h}x{w} B={batch}: HIP vs fp64 oracle {err:.2e} (worst row {max(rows):.2e}); oracle fp32 vs fp64 {noise:.2e}")
    if norm == "bn":
        assert err < TOL and max(rows) < TOL, (err, rows, noise)
    else:
        assert err < max(TOL, 3 * noise), (err, noise)
