#!/usr/bin/env python
"""Generate the golden fixtures in this directory FROM THE REFERENCE'S OWN MODULES.

Run once in the build container (needs /root/reference; never runs on the GPU box):

    python tests/golden/make_golden.py

What it does: imports ``stage2_cINN.modules.{flow_blocks,modules}`` and
``stage1_VAE.modules.{decoder,normalization_layer}`` from /root/reference (torch-only, CPU),
loads deterministic synthetic weights from ``i2v_synth`` (numpy PCG64 -- the fixtures store only
the synthesiser arguments, inputs and expected outputs, never weights or reference text), runs
the reference modules and writes ``*.npz``.

``Spade.forward`` hard-codes ``.cuda()`` (normalization_layer.py:20); on this GPU-less host the
harness makes ``Tensor.cuda`` the identity before importing the reference.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("I2V_REFERENCE", "/root/reference")

torch.Tensor.cuda = lambda self, *a, **k: self  # see module docstring
sys.path.insert(0, REF)
from stage1_VAE.modules import decoder as ref_dec  # noqa: E402
from stage1_VAE.modules import normalization_layer as ref_norm  # noqa: E402
from stage2_cINN.modules import flow_blocks as ref_fb  # noqa: E402
from stage2_cINN.modules import modules as ref_mod  # noqa: E402

spec = importlib.util.spec_from_file_location(
    "i2v_synth", os.path.join(REPO, "image2video-synthesis-using-cinns_amd", "i2v_synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)

torch.set_grad_enabled(False)
torch.manual_seed(0)


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def save(name, meta, **arrays):
    arrays = {k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}.npz  {os.path.getsize(path) / 1e3:.0f} kB")


# ----------------------------------------------------------------------------- flow units
def flow_units():
    args = dict(seed=11, n_flows=2, embedding_dim=64)
    sd = T(synth.flow_state_dict(**args))
    out = {}
    # F1 ActNorm forward / reverse / logdet  (modules.py:33-104)
    an = ref_mod.ActNorm(64, logdet=True)
    an.load_state_dict(sub(sd, "sub_layers.0.norm_layer."))
    x = rnd(1, 5, 64)
    h, ld = an(x)
    out.update(an_x=x, an_fwd=h, an_logdet=ld, an_rev=an(x, reverse=True))
    # F12 ActNorm data-dependent init in eval mode (quirk Q1)
    an0 = ref_mod.ActNorm(64, logdet=True).eval()
    x0 = 1.7 * rnd(2, 9, 64) + 0.3
    h0, ld0 = an0(x0)
    out.update(an0_x=x0, an0_fwd=h0, an0_logdet=ld0, an0_loc=an0.loc.reshape(-1), an0_scale=an0.scale.reshape(-1))
    # F2 InvLeakyRelu (flow_blocks.py:172-187)
    act = ref_fb.InvLeakyRelu()
    xa = rnd(3, 5, 64)
    ha, lda = act(xa)
    out.update(act_x=xa, act_fwd=ha, act_logdet=np.float32(lda), act_rev=act(xa, reverse=True))
    # F3 Shuffle (flow_blocks.py:142-154)
    sh = ref_fb.Shuffle(64)
    sh.load_state_dict(sub(sd, "sub_layers.0.shuffle."))
    xs = rnd(4, 5, 64)
    out.update(sh_x=xs, sh_fwd=sh(xs)[0], sh_rev=sh(xs, reverse=True))
    # F4 BasicFullyConnectedNet [7,96] -> [7,32]  (modules.py:9-30)
    net = ref_mod.BasicFullyConnectedNet(dim=96, depth=2, hidden_dim=512, out_dim=32)
    net.load_state_dict(sub(sd, "sub_layers.0.coupling.s.0."))
    xm = rnd(5, 7, 96)
    out.update(mlp_x=xm, mlp_y=net(xm))
    # F5 coupling block, modes normal and cond (flow_blocks.py:63-105)
    cb = ref_fb.ConditionalDoubleVectorCouplingBlock(64, 64, 512, 2, mode="normal")
    cb.load_state_dict(sub(sd, "sub_layers.1.coupling."))
    xc, ec = rnd(6, 6, 64), rnd(7, 6, 64)
    yc, ldc = cb(xc[:, :, None, None], ec[:, :, None, None])
    rc = cb(xc[:, :, None, None], ec[:, :, None, None], reverse=True)
    out.update(cpl_x=xc, cpl_e=ec, cpl_fwd=yc, cpl_logdet=ldc, cpl_rev=rc.reshape(6, 64))
    args_c = dict(seed=12, n_flows=2, embedding_dim=94, control=True)
    sdc = T(synth.flow_state_dict(**args_c))
    cbc = ref_fb.ConditionalDoubleVectorCouplingBlock(64, 94, 512, 2, mode="cond")
    cbc.load_state_dict(sub(sdc, "sub_layers.1.coupling."))
    ecc = rnd(8, 6, 94)
    ycc, ldcc = cbc(xc[:, :, None, None], ecc[:, :, None, None])
    rcc = cbc(xc[:, :, None, None], ecc[:, :, None, None], reverse=True)
    out.update(cplc_e=ecc, cplc_fwd=ycc, cplc_logdet=ldcc, cplc_rev=rcc.reshape(6, 64))
    # one full block (flow_blocks.py:108-139)
    blk = ref_fb.ConditionalFlatDoubleCouplingFlowBlock(64, 64, 512, 2)
    blk.load_state_dict(sub(sd, "sub_layers.1."))
    yb, ldb = blk(xc[:, :, None, None], ec[:, :, None, None])
    rb = blk(xc[:, :, None, None], ec[:, :, None, None], reverse=True)
    out.update(blk_fwd=yb, blk_logdet=ldb, blk_rev=rb.reshape(6, 64))
    save("flow_units", dict(synth=args, synth_cond=args_c), **out)


# ----------------------------------------------------------------------------- full flows (F6)
def flow_full(name, emb, control):
    args = dict(seed=7, n_flows=20, embedding_dim=emb, control=control)
    sd = T(synth.flow_state_dict(**args))
    flow = ref_fb.ConditionalFlow(64, emb, 512, 2, 20, conditioning_option="None", control=control).eval()
    flow.load_state_dict(sd)
    x, e = rnd(21, 8, 64), rnd(22, 8, emb)
    zt, ld = flow(x, e)
    z = flow(x, e, reverse=True)
    rt = flow(zt.reshape(8, 64), e, reverse=True)
    save(name, dict(synth=args, roundtrip_maxabs=float((rt.reshape(8, 64) - x).abs().max())),
         x=x, e=e, fwd=zt.reshape(8, 64), fwd_shape=np.array(zt.shape), logdet=ld,
         rev=z.reshape(8, 64), rev_shape=np.array(z.shape))
    print("   round-trip max-abs", float((rt.reshape(8, 64) - x).abs().max()),
          " |fwd| max", float(zt.abs().max()), " |rev| max", float(z.abs().max()),
          " logdet", ld[:3].tolist())


# ----------------------------------------------------------------------------- decoder units
def dec_units():
    args = dict(seed=3, channel_factor=8, negative_sigma=["g_1.conv_0", "g_1.conv_s"])
    sd = T(synth.decoder_state_dict(**args))
    out = {}
    # F7 Spade / ADAIN / Norm3D at C = 32 on [2,32,2,8,8]; g_2 of nf=8 has n_in = 32... use g_3 (n_in=32)
    x = rnd(31, 2, 32, 2, 8, 8) * 1.3 + 0.2
    img = 2 * torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(32)) - 1
    z = rnd(33, 2, 64)
    sp = ref_norm.Spade(32)
    sp.load_state_dict(sub(sd, "g_3.norm_0."))
    out.update(u_x=x, u_img=img, u_z=z, spade=sp(x, img))
    # ADAIN(16, 64) lives at g_3.norm_1 (n_mid = 16); feed a 16-channel slice
    ad = ref_norm.ADAIN(16, 64)
    ad.load_state_dict(sub(sd, "g_3.norm_1."))
    out.update(adain=ad(x[:, :16].contiguous(), z))
    n3 = ref_norm.Norm3D(32)
    n3.load_state_dict(sub(sd, "g_3.norm_s."))
    out.update(norm3d=n3(x))
    # F8 GeneratorBlock: learned shortcut with negative sigma (g_1: 128 -> 64) and identity shortcut (g_0: 128->128)
    xb = rnd(34, 2, 128, 2, 8, 8)
    g1 = ref_dec.GeneratorBlock(128, 64, True, 64).eval()
    g1.load_state_dict(sub(sd, "g_1."))
    w = sd["g_1.conv_0.weight_orig"]
    sig = float(torch.dot(sd["g_1.conv_0.weight_u"], torch.mv(w.reshape(w.shape[0], -1), sd["g_1.conv_0.weight_v"])))
    assert sig < 0, sig
    out.update(b_x=xb, block_g1=g1(xb, z, img))
    g0 = ref_dec.GeneratorBlock(128, 128, True, 64).eval()
    g0.load_state_dict(sub(sd, "g_0."))
    out.update(block_g0=g0(xb, z, img))
    save("dec_units", dict(synth=args, sigma_g1_conv0=sig), **out)


def _gen(nf, ups, upt, seed, **extra):
    args = dict(seed=seed, channel_factor=nf, **extra)
    sd = T(synth.decoder_state_dict(**args))
    g = ref_dec.Generator({"channel_factor": nf, "z_dim": 64, "upsample_s": ups, "upsample_t": upt,
                           "spectral_norm": True}).eval()
    g.load_state_dict(sd)
    return g, args


def _pre_tanh(g, img, z):
    """Generator.forward up to conv_img (decoder.py:97-117), to store the pre-tanh tensor."""
    import torch.nn.functional as F
    x = g.fc(z).reshape(img.size(0), -1, 1, 4, 4)
    x = g.head_0(x, z, img)
    for blk in (g.g_0, g.g_1, g.g_2):
        x = blk(F.interpolate(x, scale_factor=2), z, img)
    x = g.g_3(F.interpolate(x, scale_factor=(g.upsample_t[0], g.upsample_s[0], g.upsample_s[0])), z, img)
    x = g.g_4(F.interpolate(x, scale_factor=(g.upsample_t[1], g.upsample_s[1], g.upsample_s[1])), z, img)
    return g.conv_img(F.leaky_relu(x, 2e-1))


def dec_small():
    # F9: smallest legal width nf = 8, both geometries
    g, args = _gen(8, [2, 1], [2, 1], 5)
    img = 2 * torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(41)) - 1
    z = rnd(42, 2, 64)
    y = g(img, z)
    pre = _pre_tanh(g, img, z)
    assert not y.is_contiguous() and tuple(y.shape) == (2, 16, 3, 64, 64)
    save("dec_nf8_bair", dict(synth=args, upsample_s=[2, 1], upsample_t=[2, 1],
                              sat=float((y.abs() > 0.999).float().mean())), img=img, z=z, out=y.contiguous(),
         pre_tanh=pre)
    print("   nf8 bair: |pre| mean", float(pre.abs().mean()), "max", float(pre.abs().max()))
    g, args = _gen(8, [2, 2], [2, 1], 6)
    img = 2 * torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(43)) - 1
    z = rnd(44, 1, 64)
    y = g(img, z)
    assert tuple(y.shape) == (1, 16, 3, 128, 128)
    save("dec_nf8_128", dict(synth=args, upsample_s=[2, 2], upsample_t=[2, 1], stride=2), img=img, z=z,
         out_s2=y[..., ::2, ::2].contiguous())


def dec_full():
    # F10: full-width anchors, B = 1 (outputs stored on a stride-2 pixel lattice)
    g, args = _gen(64, [2, 1], [2, 1], 7)
    img = 2 * torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(51)) - 1
    z = rnd(52, 1, 64)
    y = g(img, z)
    save("dec_nf64_bair", dict(synth=args, upsample_s=[2, 1], upsample_t=[2, 1], stride=2), img=img, z=z,
         out_s2=y[..., ::2, ::2].contiguous())
    print("   nf64 bair |y| mean", float(y.abs().mean()), "max", float(y.abs().max()))
    g, args = _gen(32, [2, 2], [2, 1], 7)
    img = 2 * torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(53)) - 1
    z = rnd(54, 1, 64)
    y = g(img, z)
    save("dec_nf32_128", dict(synth=args, upsample_s=[2, 2], upsample_t=[2, 1], stride=2), img=img, z=z,
         out_s2=y[..., ::2, ::2].contiguous())
    print("   nf32 128 |y| mean", float(y.abs().mean()), "max", float(y.abs().max()))


def model_small():
    # F11: Model.forward semantics (get_model.py:51-75) with the reference flow + decoder modules,
    # residual and embed supplied.  nf = 8, n_flows = 20.  The latents come out of the cINN (|z| ~ 5, not a unit normal), which
    # drives dec_small()'s weights into tanh saturation (21 % of yq3 above 0.99: a numeric check is blind there); conv_img is
    # therefore scaled by 0.25 (SURVEY 8c fixture requirement ii: < 1 % of the stored frames above 0.99).
    g, dargs = _gen(8, [2, 1], [2, 1], 5, conv_img_gain=0.25)
    fargs = dict(seed=7, n_flows=20, embedding_dim=64, control=False)
    flow = ref_fb.ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None").eval()
    flow.load_state_dict(T(synth.flow_state_dict(**fargs)))

    def forward(x_0, residual, embed, vid_length):
        z = flow(residual, embed, reverse=True).view(x_0.size(0), -1)   # get_model.py:65
        seq = g(x_0, z)                                                  # :68
        while seq.shape[1] < vid_length:                                 # :71-73
            seq1 = g(seq[:, -1], z)
            seq = torch.cat((seq, seq1), dim=1)
        return seq[:vid_length]                                          # :75 (quirk Q3)

    x1 = 2 * torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(61)) - 1
    r1, e1 = rnd(62, 1, 64), rnd(63, 1, 64)
    y32 = forward(x1, r1, e1, 32)
    assert tuple(y32.shape) == (1, 32, 3, 64, 64)
    x3 = 2 * torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(64)) - 1
    r3, e3 = rnd(65, 3, 64), rnd(66, 3, 64)
    yq3 = forward(x3, r3, e3, 2)          # B=3 > vid_length=2 -> only 2 samples come back, 16 frames each
    assert tuple(yq3.shape) == (2, 16, 3, 64, 64)
    y20 = forward(x1, r1, e1, 20)         # B=1 <= 20: T is NOT trimmed -> 32 frames
    assert tuple(y20.shape) == (1, 32, 3, 64, 64)
    sat = {k: [float((v.abs() > 0.99).float().mean()), float((v.abs() > 0.999).float().mean())] for k, v in (("y32", y32), ("yq3", yq3))}
    print("   model_nf8 saturation (fraction above 0.99 / 0.999):", sat)
    assert all(v[0] < 0.01 for v in sat.values()), sat
    save("model_nf8", dict(synth_dec=dargs, synth_flow=fargs, upsample_s=[2, 1], upsample_t=[2, 1], saturation=sat),
         x1=x1, r1=r1, e1=e1, y32=y32.contiguous(), x3=x3, r3=r3, e3=e3,
         yq3_shape=np.array(yq3.shape), yq3_t4=yq3[:, ::4].contiguous(), y20_shape=np.array(y20.shape))


def model_t32_128():
    # cfg5 geometry (128x128, nf = 32, E = 128, vid_length = 32): the get_model.py:65-75 sequence with the reference
    # flow + decoder, B = 2 -> two dependent decoder passes; frames stored on a stride-4 pixel lattice (all 32 frames)
    g, dargs = _gen(32, [2, 2], [2, 1], 7)
    fargs = dict(seed=7, n_flows=20, embedding_dim=128, control=False)
    flow = ref_fb.ConditionalFlow(64, 128, 512, 2, 20, conditioning_option="None").eval()
    flow.load_state_dict(T(synth.flow_state_dict(**fargs)))
    x0 = 2 * torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(81)) - 1
    r, e = rnd(82, 2, 64), rnd(83, 2, 128)
    z = flow(r, e, reverse=True).view(2, -1)
    seq = g(x0, z)
    while seq.shape[1] < 32:
        seq = torch.cat((seq, g(seq[:, -1], z)), dim=1)
    assert tuple(seq.shape) == (2, 32, 3, 128, 128)
    save("model_nf32_128_t32", dict(synth_dec=dargs, synth_flow=fargs, upsample_s=[2, 2], upsample_t=[2, 1], stride=4),
         x0=x0, r=r, e=e, z=z, out_s4=seq[..., ::4, ::4].contiguous())
    print("   nf32 128 T=32 |y| mean", float(seq.abs().mean()), "max", float(seq.abs().max()),
          "second pass |y| mean", float(seq[:, 16:].abs().mean()))


def encoder3d():
    # N3: the motion Encoder of the reference (stage1_VAE/modules/resnet3D.py:138-219), BAIR and landscape geometries
    from stage1_VAE.modules import resnet3D as ref_r3d
    for name, channels, stride_s, size, nfr in (("enc3d_bair", [64, 128, 256, 512, 512], [1, 2, 2, 2], 64, 16),
                                                ("enc3d_land", [64, 128, 128, 256, 512], [2, 2, 2, 2], 128, 15)):
        args = dict(seed=9, z_dim=64, channels=channels, stride_s=stride_s)
        enc = ref_r3d.Encoder({"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": 64, "channels": channels,
                               "stride_s": stride_s, "stride_t": [1, 2, 2, 2], "deterministic": False}).eval()
        enc.load_state_dict(T(synth.encoder3d_state_dict(**args)))
        # the clip is regenerated from its seed at test time (CPU generator); a checksum guards against RNG drift
        x = 2 * torch.rand(2, 3, nfr, size, size, generator=torch.Generator().manual_seed(71)) - 1
        _, mu, logvar = enc(x)
        save(name, dict(synth=args, stride_t=[1, 2, 2, 2], x_seed=71, x_shape=list(x.shape)), x_head=x.reshape(-1)[:16],
             x_sum=np.float64(x.double().sum()), mu=mu, logvar=logvar)
        print("   ", name, "|mu| mean", float(mu.abs().mean()), "|logvar| mean", float(logvar.abs().mean()))


def save_stable(name, meta, **arrays):
    """``save`` with a fixed member order and time stamp: the same arrays give the same file, byte for byte."""
    import io
    import zipfile
    arrays = {k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w") as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)
    print(f"{name}.npz  {os.path.getsize(path) / 1e3:.0f} kB")


def encoder3d_cfgs():
    # N3 at the configurations of tests/encoder_cfgs.py that the reference's Encoder can build (64-channel stem): one file,
    # <case>_mu / _logvar / _x_head / _x_sum per case, the cases' synthesiser arguments in the meta.  Runs only when named.
    from stage1_VAE.modules import resnet3D as ref_r3d
    spec = importlib.util.spec_from_file_location("encoder_cfgs", os.path.join(REPO, "tests", "encoder_cfgs.py"))
    cfgs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cfgs)
    out, meta = {}, {"cases": {}}
    for name in cfgs.REF_NAMES:
        c = cfgs.CASES[name]
        a = c["synth"]
        enc = ref_r3d.Encoder({"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": a["z_dim"], "channels": a["channels"],
                               "stride_s": a["stride_s"], "stride_t": c["stride_t"], "deterministic": False}).eval()
        enc.load_state_dict(T(synth.encoder3d_state_dict(**a)))
        x = 2 * torch.rand(*c["x_shape"], generator=torch.Generator().manual_seed(c["x_seed"])) - 1
        _, mu, logvar = enc(x)
        out.update({name + "_mu": mu, name + "_logvar": logvar, name + "_x_head": x.reshape(-1)[:16],
                    name + "_x_sum": np.float64(x.double().sum())})
        meta["cases"][name] = {k: c[k] for k in ("synth", "stride_t", "x_seed", "x_shape")}
        print("   ", name, "|mu| mean", float(mu.abs().mean()), "|logvar| mean", float(logvar.abs().mean()))
    save_stable("enc3d_cfgs", meta, **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["flow_units", "flow_full", "dec_units", "dec_small", "dec_full", "model_small", "encoder3d",
                             "model_t32_128"]
    if "flow_units" in which:
        flow_units()
    if "flow_full" in which:
        flow_full("flow_full_e64", 64, False)
        flow_full("flow_full_e128", 128, False)
        flow_full("flow_full_ctrl", 94, True)
    if "dec_units" in which:
        dec_units()
    if "dec_small" in which:
        dec_small()
    if "dec_full" in which:
        dec_full()
    if "model_small" in which:
        model_small()
    if "encoder3d" in which:
        encoder3d()
    if "model_t32_128" in which:
        model_t32_128()
    if "encoder3d_cfgs" in which:   # (not in the default list: the fixtures above are never rewritten by it)
        encoder3d_cfgs()
