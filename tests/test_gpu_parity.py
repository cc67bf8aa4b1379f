"""Parity of the HIP path (through the C ABI / the class-surface mirror) against the golden vectors generated from
the reference modules and against the CPU oracle.  Run on the GPU box: pytest -m gpu.

Tolerances (BASELINE.json north_star / SURVEY §8d): frames and z within 1e-4 relative L2, logdet within 1e-4
abs-rel, flow round trip <= 1e-4 max-abs on the synthetic (expansive) flow."""
import os

import numpy as np
import pytest
import torch

import i2v_synth as synth
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()  # fails loudly if libi2v_hip.so is missing
    torch.set_grad_enabled(False)


def test_flow_leaf_modules_vs_golden():
    from stage2_cINN.modules import flow_blocks as fb, modules as md
    g, meta = load_golden("flow_units")
    sd = T(synth.flow_state_dict(**meta["synth"]))
    an = md.ActNorm(64, logdet=True)
    an.load_state_dict(sub(sd, "sub_layers.0.norm_layer."))
    an = an.cuda()
    h, ld = an(cu(g["an_x"]))
    assert rel_l2(h.cpu(), g["an_fwd"]) < 1e-6 and np.allclose(ld.cpu(), g["an_logdet"], rtol=1e-5)
    assert rel_l2(an(cu(g["an_x"]), reverse=True).cpu(), g["an_rev"]) < 1e-6
    # quirk Q1: data-dependent init on the first forward, in eval mode
    an0 = md.ActNorm(64, logdet=True).cuda().eval()
    h0, ld0 = an0(cu(g["an0_x"]))
    assert int(an0.initialized.item()) == 1
    assert rel_l2(an0.loc.reshape(-1).cpu(), g["an0_loc"]) < 1e-5 and rel_l2(an0.scale.reshape(-1).cpu(), g["an0_scale"]) < 1e-5
    assert rel_l2(h0.cpu(), g["an0_fwd"]) < 1e-5 and np.allclose(ld0.cpu(), g["an0_logdet"], rtol=1e-4, atol=1e-4)
    act = fb.InvLeakyRelu()
    ha, lda = act(cu(g["act_x"]))
    assert lda == 0.0 and np.array_equal(ha.cpu().numpy(), g["act_fwd"])  # quirk Q2
    assert rel_l2(act(cu(g["act_x"]), reverse=True).cpu(), g["act_rev"]) < 1e-6
    sh = fb.Shuffle(64)
    sh.load_state_dict(sub(sd, "sub_layers.0.shuffle."))
    sh = sh.cuda()
    y, ld = sh(cu(g["sh_x"]))
    assert ld == 0 and np.array_equal(y.cpu().numpy(), g["sh_fwd"])
    assert np.array_equal(sh(cu(g["sh_x"]), reverse=True).cpu().numpy(), g["sh_rev"])
    net = md.BasicFullyConnectedNet(dim=96, depth=2, hidden_dim=512, out_dim=32)
    net.load_state_dict(sub(sd, "sub_layers.0.coupling.s.0."))
    assert rel_l2(net.cuda()(cu(g["mlp_x"])).cpu(), g["mlp_y"]) < TOL


def test_coupling_and_block_vs_golden():
    from stage2_cINN.modules import flow_blocks as fb
    g, meta = load_golden("flow_units")
    sd = T(synth.flow_state_dict(**meta["synth"]))
    x4, e4 = cu(g["cpl_x"])[:, :, None, None], cu(g["cpl_e"])[:, :, None, None]
    cb = fb.ConditionalDoubleVectorCouplingBlock(64, 64, 512, 2, mode="normal")
    cb.load_state_dict(sub(sd, "sub_layers.1.coupling."))
    cb = cb.cuda()
    y, ld = cb(x4, e4)
    assert y.shape == (6, 64) and rel_l2(y.cpu(), g["cpl_fwd"]) < TOL and np.allclose(ld.cpu(), g["cpl_logdet"], atol=1e-4)
    r = cb(x4, e4, reverse=True)
    assert r.shape == (6, 64, 1, 1) and rel_l2(r.reshape(6, 64).cpu(), g["cpl_rev"]) < TOL
    with pytest.raises(AssertionError):
        cb(x4.reshape(6, 64), e4)  # flow_blocks.py:78-79 asserts 4-D inputs
    sdc = T(synth.flow_state_dict(**meta["synth_cond"]))
    cbc = fb.ConditionalDoubleVectorCouplingBlock(64, 94, 512, 2, mode="cond")
    cbc.load_state_dict(sub(sdc, "sub_layers.1.coupling."))
    cbc = cbc.cuda()
    ec = cu(g["cplc_e"])[:, :, None, None]
    y, ld = cbc(x4, ec)
    assert rel_l2(y.cpu(), g["cplc_fwd"]) < TOL and np.allclose(ld.cpu(), g["cplc_logdet"], atol=1e-4)
    assert rel_l2(cbc(x4, ec, reverse=True).reshape(6, 64).cpu(), g["cplc_rev"]) < TOL
    blk = fb.ConditionalFlatDoubleCouplingFlowBlock(64, 64, 512, 2)
    blk.load_state_dict(sub(sd, "sub_layers.1."))
    blk = blk.cuda()
    y, ld = blk(x4, e4)
    assert rel_l2(y.cpu(), g["blk_fwd"]) < TOL and np.allclose(ld.cpu(), g["blk_logdet"], atol=1e-4)
    assert rel_l2(blk(x4, e4, reverse=True).reshape(6, 64).cpu(), g["blk_rev"]) < TOL


@pytest.mark.parametrize("name", ["flow_full_e64", "flow_full_e128", "flow_full_ctrl"])
def test_full_flow_vs_golden(name):
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    g, meta = load_golden(name)
    a = meta["synth"]
    flow = ConditionalFlow(64, a["embedding_dim"], 512, 2, 20, conditioning_option="None", control=a["control"])
    flow.load_state_dict(T(synth.flow_state_dict(**a)))
    flow = flow.cuda().eval()
    x, e = cu(g["x"]), cu(g["e"])
    zt, ld = flow(x, e)
    assert list(zt.shape) == list(g["fwd_shape"]) and ld.shape == (8,)
    assert rel_l2(zt.reshape(8, 64).cpu(), g["fwd"]) < TOL
    assert np.allclose(ld.cpu(), g["logdet"], rtol=1e-4, atol=1e-4)
    z = flow(x, e, reverse=True)
    assert list(z.shape) == list(g["rev_shape"])
    assert rel_l2(z.reshape(8, 64).cpu(), g["rev"]) < TOL
    assert rel_l2(flow.reverse(x, e).reshape(8, 64).cpu(), g["rev"]) < TOL
    rt = flow(zt, e, reverse=True).reshape(8, 64)
    assert float((rt - x).abs().max()) < 1e-4  # invertibility
    # second call replays the captured graph; results must be identical
    assert torch.equal(flow(x, e, reverse=True), z)


def test_flow_batch_sizes_and_sharding_property():
    """Full-width flow at the BASELINE batch (64) vs the oracle, ragged batches, and batch-permutation
    equivariance (proves shardability)."""
    from oracle import flow_ref
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    sd = T(synth.flow_state_dict(seed=7, embedding_dim=64))
    flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(sd)
    flow = flow.cuda().eval()
    _, residual, embed = synth.bench_inputs(64, 64, 64)
    ref = flow_ref.flow_reverse(sd, residual, embed).reshape(64, 64)
    z = flow(residual.cuda(), embed.cuda(), reverse=True).reshape(64, 64)
    assert rel_l2(z.cpu(), ref) < TOL
    for lo, hi in ((0, 1), (3, 10), (0, 37)):  # shards: same rows, any batch size incl. 1 and non-multiples of 64
        zs = flow(residual[lo:hi].cuda().contiguous(), embed[lo:hi].cuda().contiguous(), reverse=True).reshape(hi - lo, 64)
        assert rel_l2(zs.cpu(), ref[lo:hi]) < TOL
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0))
    zp = flow(residual[perm].cuda(), embed[perm].cuda(), reverse=True).reshape(64, 64)
    assert torch.equal(zp.cpu(), z.cpu()[perm])
    zt, ld = flow(residual[:11].cuda().contiguous(), embed[:11].cuda().contiguous())  # forward, ragged B = 11
    ztr, ldr = flow_ref.flow_forward(sd, residual[:11], embed[:11])
    assert rel_l2(zt.reshape(11, 64).cpu(), ztr.reshape(11, 64)) < TOL and np.allclose(ld.cpu(), ldr, rtol=1e-4, atol=1e-4)


def _gen(meta, **cfg):
    from stage1_VAE.modules.decoder import Generator
    gen = Generator({"channel_factor": meta["synth"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"],
                     "upsample_t": meta["upsample_t"], "spectral_norm": True, **cfg})
    gen.load_state_dict(T(synth.decoder_state_dict(**meta["synth"])))
    return gen.cuda().eval()


def test_decoder_nf8_bair_vs_golden():
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    out = gen(cu(g["img"]), cu(g["z"]))
    assert out.shape == (2, 16, 3, 64, 64) and out.is_contiguous()
    assert rel_l2(out.cpu(), g["out"]) < TOL
    assert float(out.abs().max()) < 1.0  # tanh range
    # batch-permutation equivariance and batch-size independence (B = 1 shard of a B = 2 batch): bit-identical
    perm = torch.tensor([1, 0])
    out2 = gen(cu(g["img"])[perm].contiguous(), cu(g["z"])[perm].contiguous())
    assert torch.equal(out2, out[perm])
    out1 = gen(cu(g["img"])[1:].contiguous(), cu(g["z"])[1:].contiguous())
    assert torch.equal(out1, out[1:])


def test_decoder_nf8_128_vs_golden():
    g, meta = load_golden("dec_nf8_128")
    out = _gen(meta)(cu(g["img"]), cu(g["z"]))
    assert out.shape == (1, 16, 3, 128, 128)
    assert rel_l2(out[..., ::2, ::2].cpu(), g["out_s2"]) < TOL


def test_decoder_full_width_bair_vs_golden():
    g, meta = load_golden("dec_nf64_bair")
    out = _gen(meta)(cu(g["img"]), cu(g["z"]))
    assert out.shape == (1, 16, 3, 64, 64)
    assert rel_l2(out[..., ::2, ::2].cpu(), g["out_s2"]) < TOL


def test_decoder_full_width_128_vs_golden():
    g, meta = load_golden("dec_nf32_128")
    out = _gen(meta)(cu(g["img"]), cu(g["z"]))
    assert out.shape == (1, 16, 3, 128, 128)
    assert rel_l2(out[..., ::2, ::2].cpu(), g["out_s2"]) < TOL


def test_decoder_negative_sigma_and_resized_start_frame():
    """Signed sigma (quirk D6) folded exactly, and a start frame whose size differs from the SPADE resolutions
    (bilinear resize path) -- vs the oracle."""
    from oracle import decoder_ref
    from stage1_VAE.modules.decoder import Generator
    args = dict(seed=3, channel_factor=8, negative_sigma=["g_1.conv_0", "g_1.conv_s", "g_3.conv_1"])
    sd = T(synth.decoder_state_dict(**args))
    gen = Generator({"channel_factor": 8, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True})
    gen.load_state_dict(sd)
    gen = gen.cuda().eval()
    img = 2 * torch.rand(3, 3, 48, 80, generator=torch.Generator().manual_seed(5)) - 1
    z = torch.randn(3, 64, generator=torch.Generator().manual_seed(6))
    ref = decoder_ref.generator(sd, img, z)
    out = gen(img.cuda(), z.cuda())
    assert rel_l2(out.cpu(), ref) < TOL


def test_decoder_submodules_vs_golden():
    """Spade / ADAIN / Norm3D / GeneratorBlock called on their own with the reference's [B,C,T,H,W] tensors (F7, F8),
    in both matrix-core modes; the negative-sigma block pins quirk D6."""
    from stage1_VAE.modules import decoder as dec, normalization_layer as nl
    g, meta = load_golden("dec_units")
    sd = T(synth.decoder_state_dict(**meta["synth"]))
    x, img, z = cu(g["u_x"]), cu(g["u_img"]), cu(g["u_z"])
    sp = nl.Spade(32)
    sp.load_state_dict(sub(sd, "g_3.norm_0."))
    assert rel_l2(sp.cuda()(x, img).cpu(), g["spade"]) < TOL
    ad = nl.ADAIN(16, 64)
    ad.load_state_dict(sub(sd, "g_3.norm_1."))
    assert rel_l2(ad.cuda()(x[:, :16].contiguous(), z).cpu(), g["adain"]) < TOL
    n3 = nl.Norm3D(32)
    n3.load_state_dict(sub(sd, "g_3.norm_s."))
    assert rel_l2(n3.cuda()(x).cpu(), g["norm3d"]) < TOL
    xb = cu(g["b_x"])
    assert meta["sigma_g1_conv0"] < 0
    for name, n_out, key in (("g_1", 64, "block_g1"), ("g_0", 128, "block_g0")):
        blk = dec.GeneratorBlock(128, n_out, True, 64)
        blk.load_state_dict(sub(sd, name + "."))
        out = blk.cuda()(xb, z, img)
        assert out.shape == (2, n_out, 2, 8, 8) and rel_l2(out.cpu(), g[key]) < TOL


@pytest.mark.parametrize("wino4", [None, "2"])
def test_generator_block_shape_sweep_winograd_and_fallback(wino4, monkeypatch):
    """Stand-alone GeneratorBlock over geometries on both sides of the Winograd kernel's tiling rule (csrc/i2v_conv16w.hip:
    bricks of TT x TH x 4 output pairs, halo brick <= 1024 staged rows): single frames and T = 2 (halo too large -> direct
    kernel; these raised I2V_E_INVALID before round 3), narrow / wide / tall maps, T = 4 and 8 (TT = 4, TH = 8 bricks), both
    the identity-shortcut (128 -> 128) and the learned-shortcut (128 -> 64) block, against the oracle."""
    from oracle import decoder_ref
    from stage1_VAE.modules import decoder as dec
    if wino4:   # I2V_DEC_WINO4=2: the F(4,3) kernel wherever its tiling allows (default: only where a sample fills 32 workgroups,
        monkeypatch.setenv("I2V_DEC_WINO4", wino4)   # which none of these small maps does) -- [.,4,16,16], [.,4,8,32], [.,8,32,16] here
    sd = T(synth.decoder_state_dict(seed=5, channel_factor=8))
    g = torch.Generator().manual_seed(31)
    for name, n_out in (("g_0", 128), ("g_1", 64)):
        blk = dec.GeneratorBlock(128, n_out, True, 64)
        blk.load_state_dict(sub(sd, name + "."))
        blk = blk.cuda().eval()
        for (B, Tn, H, W) in ((2, 1, 16, 16), (1, 2, 16, 16), (1, 4, 8, 8), (1, 4, 16, 16), (2, 4, 8, 32), (1, 8, 32, 16),
                              (1, 16, 16, 8), (1, 2, 8, 64)):
            x = torch.randn(B, 128, Tn, H, W, generator=g)
            img = 2 * torch.rand(B, 3, 24, 40, generator=g) - 1
            z = torch.randn(B, 64, generator=g)
            ref = decoder_ref.generator_block(sd, name, x, z, img)
            out = blk(x.cuda(), z.cuda(), img.cuda())
            assert out.shape == ref.shape and rel_l2(out.cpu(), ref) < TOL, (name, B, Tn, H, W, rel_l2(out.cpu(), ref))
        assert blk.native().status() == 0
    if wino4:   # the forced mode really ran another kernel on an eligible shape
        x = torch.randn(1, 128, 4, 16, 16, generator=g).cuda()
        img, z = (2 * torch.rand(1, 3, 16, 16, generator=g) - 1).cuda(), torch.randn(1, 64, generator=g).cuda()
        a = blk(x, z, img)
        monkeypatch.setenv("I2V_DEC_WINO4", "0")
        blk0 = dec.GeneratorBlock(128, 64, True, 64)
        blk0.load_state_dict(sub(sd, "g_1."))
        b = blk0.cuda().eval()(x, z, img)
        assert not torch.equal(a, b) and rel_l2(a.cpu(), b.cpu()) < 1e-5


def test_both_matrix_core_modes_agree():
    """mma = 0 (exact fp32 MFMA) and mma = 1 (split-fp16) against the same golden frames."""
    from stage1_VAE.modules.decoder import Generator
    g, meta = load_golden("dec_nf8_bair")
    for mma in (0, 1):
        gen = Generator({"channel_factor": 8, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True,
                         "mma": mma})
        gen.load_state_dict(T(synth.decoder_state_dict(**meta["synth"])))
        assert rel_l2(gen.cuda().eval()(cu(g["img"]), cu(g["z"])).cpu(), g["out"]) < TOL


@pytest.mark.parametrize("golden", ["dec_nf8_bair", "dec_nf64_bair", "dec_nf32_128"])
def test_exact_fp32_mode_winograd_and_direct(golden, monkeypatch):
    """mma = 0, the range-safe mode: from the 16x16 level on its 3x3x3 convs run Winograd F(4,3) on the fp32 matrix cores (round 5:
    csrc/i2v_wino32.hip; I2V_DEC_WINO32=0 keeps the 27-tap kernel).  Both must reproduce the reference-generated golden frames;
    the Winograd path against the direct one shows the transform's fp32 rounding (~1e-6), not a different result; the stand-alone
    sub-batches of the last two levels and the strided in-place sequence work in this mode too."""
    from stage1_VAE.modules.decoder import Generator
    g, meta = load_golden(golden)

    def make():
        gen = Generator({"channel_factor": meta["synth"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"],
                         "upsample_t": meta["upsample_t"], "spectral_norm": True, "mma": 0})
        gen.load_state_dict(T(synth.decoder_state_dict(**meta["synth"])))
        return gen.cuda().eval()

    img, z = cu(g["img"]), cu(g["z"])
    wino = make()(img, z)
    monkeypatch.setenv("I2V_DEC_WINO32", "0")
    direct = make()(img, z)
    monkeypatch.delenv("I2V_DEC_WINO32")
    key = "out" if "out" in g else "out_s2"
    sl = (lambda t: t) if key == "out" else (lambda t: t[..., ::2, ::2])
    e_w, e_d, e_wd = rel_l2(sl(wino).cpu(), g[key]), rel_l2(sl(direct).cpu(), g[key]), rel_l2(wino.cpu(), direct.cpu())
    print(f"exact-fp32 mode ({golden}): Winograd vs golden {e_w:.2e}, direct vs golden {e_d:.2e}, Winograd vs direct {e_wd:.2e}")
    assert e_w < TOL and e_d < TOL and e_wd < 2e-5 and not torch.equal(wino, direct)
    # rows of a larger batch equal the small run (every op is per sample), and the decoder's in-place sequence works in this mode
    gen = make()
    x3 = img[:1].repeat(3, 1, 1, 1).contiguous()
    z3 = z[:1].repeat(3, 1).contiguous()
    big = gen(x3, z3)
    assert torch.equal(big[2:3], wino[:1]) and torch.equal(big[0], big[1])
    if golden == "dec_nf8_bair":
        seq = gen.decode_sequence(img, z, 32)
        assert torch.equal(seq[:, :16], wino) and torch.equal(seq[:, 16:], gen(wino[:, -1].contiguous(), z))


@pytest.mark.parametrize("env", ["I2V_DEC_WINO", "I2V_DEC_WINO4", "I2V_DEC_PW16", "I2V_DEC_IMG16", "I2V_DEC_SPW"])
def test_decoder_alternative_kernel_paths(env, monkeypatch):
    """The kernels the split-fp16 mode picks by default each have a tested fallback behind an env switch read when the
    handle is created (direct instead of Winograd 3x3x3 convs; Winograd F(2,3) instead of F(4,3); exact-fp32 MFMA shortcut GEMM; vector-ALU conv_img; SPADE's gamma | beta
    conv on the direct instead of the 1x3x3 Winograd kernel): the
    full-width BAIR decoder must reproduce the golden frames either way."""
    g, meta = load_golden("dec_nf64_bair")
    ref = _gen(meta)(cu(g["img"]), cu(g["z"]))
    monkeypatch.setenv(env, "0")
    alt = _gen(meta)(cu(g["img"]), cu(g["z"]))
    assert rel_l2(alt[..., ::2, ::2].cpu(), g["out_s2"]) < TOL
    assert rel_l2(alt.cpu(), ref.cpu()) < 1e-5 and not torch.equal(alt, ref)   # a different kernel really ran


@pytest.mark.parametrize("golden", ["dec_nf64_bair", "dec_nf32_128"])
def test_f43_structure_switches_keep_the_bits(golden, monkeypatch, tmp_path):
    """The F(4,3) kernel's measurement switches change WHERE and WHEN a brick is computed, never the arithmetic of an output:
    the brick -> XCD orders, 32-channel workgroups, the 512- / 256-thread geometries and conv_img's frames per workgroup must reproduce the default kernel's frames bit for bit, on
    the 64-channel (BAIR nf = 64) and the 32-channel (128x128 nf = 32) instantiations.  Since round 6 those switches exist only in the
    MEASUREMENT build of the library (-DI2V_MEASURE, lib/libi2v_hip_measure.so): the production library reads no environment variable
    on a launch path.  So the frames of the production library (this process) are handed to tests/measure_worker.py, which runs in
    a process of its own with I2V_LIB_PATH on the measurement build.  The decoder's own switches (read when a handle is created:
    sub-batching of the last two levels, in-call overlap) are flipped in this process."""
    import json
    import subprocess
    import sys
    import i2v_native
    g, meta = load_golden(golden)
    x0, z, _ = synth.bench_inputs(3, g["img"].shape[-1], 64)     # 3 samples: grids that are not a multiple of the CU count
    x0[1], z[1] = torch.from_numpy(g["img"][0]), torch.from_numpy(g["z"][0])
    x0, z = x0.cuda(), z.cuda()
    ref = _gen(meta)(x0, z)
    assert rel_l2(ref[1:2, ..., ::2, ::2].cpu(), g["out_s2"]) < TOL
    for env, val in (("I2V_DEC_SUB", "1"), ("I2V_DEC_SUB", "2"), ("I2V_DEC_OVERLAP", "0"), ("I2V_DEC_OVERLAP", "2")):
        monkeypatch.setenv(env, val)
        alt = _gen(meta)(x0, z)
        monkeypatch.delenv(env)
        assert torch.equal(alt, ref), (env, val, float((alt - ref).abs().max()))
    # the production library ignores the measurement switches altogether (no getenv on a launch path)
    monkeypatch.setenv("I2V_W4_BN", "32")
    monkeypatch.setenv("I2V_W4_NTH", "256")
    assert torch.equal(_gen(meta)(x0, z), ref)
    monkeypatch.delenv("I2V_W4_BN")
    monkeypatch.delenv("I2V_W4_NTH")
    if not os.path.exists(i2v_native.MEASURE_LIB_PATH):
        i2v_native.build_measure()                               # (hipcc is on the GPU box; normally built by __graft_entry__.build())
    blob = tmp_path / "case.npz"
    np.savez(blob, x0=x0.cpu().numpy(), z=z.cpu().numpy(), ref=ref.cpu().numpy(), meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
    env = dict(os.environ, I2V_LIB_PATH=os.path.join("image2video-synthesis-using-cinns_amd", "lib", "libi2v_hip_measure.so"))   # relative to the repo root
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "measure_worker.py"), str(blob)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["checked"] == 9 and res["bad"] == [], res   # the defaults + the eight switch settings of measure_worker.py


def test_generated_operand_kernel_keeps_the_bits(monkeypatch):
    """Round 6: the thin F(4,3) layers of the 128x128 configs (g_4: 64 -> 32 behind SPADE and a x2 spatial up-sampling, 32 -> 32 behind
    ADAIN) can generate their operand in the conv kernel itself -- 8 MFMA waves + 4 producer waves that form lrelu(norm(x)), B^T d
    and the fp16 hi / lo split from the conv's fp32 input (csrc/i2v_conv16w4g.hip, I2V_DEC_GEN; opt-in: measured -6 % on layer + writer,
    profiles/r06_d_thin_fused_no_go.md) -- instead of reading the V tensor modulate_wino4_kernel wrote.  Same expressions in the same
    order: the frames must be the same BITS as the writer path's at the golden's batch and on a 5-sample batch (bricks at every border of
    the tensor, several samples), the range guard must see the same things (in range: nothing; the underflow slot of g_4.conv_1 when
    its ADAIN is scaled to 2^-20), and the golden holds."""
    from stage1_VAE.modules.decoder import Generator
    g, meta = load_golden("dec_nf32_128")
    img, z = cu(g["img"]), cu(g["z"])
    x5, z5, _ = synth.bench_inputs(5, 128, 64)
    x5, z5 = x5.cuda(), z5.cuda()
    monkeypatch.setenv("I2V_DEC_GEN", "0")
    ref_gen = _gen(meta)
    ref, ref5 = ref_gen(img, z), ref_gen(x5, z5)
    monkeypatch.setenv("I2V_DEC_GEN", "1")
    gen = _gen(meta)
    gen.native().set_profile(True)
    out, out5 = gen(img, z), gen(x5, z5)
    torch.cuda.synchronize()
    kernels = {L["layer"]: L["kernel"] for L in gen.native().get_layer_profile()}
    gen.native().set_profile(False)
    assert kernels["g_4.conv_0"] == kernels["g_4.conv_1"] == "conv_wino4g_f16x3" and kernels["g_3.conv_1"] == "conv_wino4_f16x3", kernels
    assert rel_l2(out[..., ::2, ::2].cpu(), g["out_s2"]) < TOL
    d1, d5 = float((out - ref).abs().max()), float((out5 - ref5).abs().max())
    e1, e5 = rel_l2(out.cpu(), ref.cpu()), rel_l2(out5.cpu(), ref5.cpu())
    print(f"generated operand vs writer path: max |diff| {d1:.3e} / rel-L2 {e1:.2e} (golden batch), {d5:.3e} / {e5:.2e} (5 samples)")
    # Same expressions, same bits -- as long as the producer keeps the writer's TWO roundings of the hi part (fp32, then fp16): left
    # alone, hipcc fuses the transform's last fma with the conversion into one v_fma_mixlo_f16 (a single rounding) and ~0.5 % of the
    # conv outputs move by one ulp (found with tools/conv16w_check's I2V_CHECK_GEN stages; i2v_conv16w4g.hip keeps the value opaque).
    assert torch.equal(out, ref) and torch.equal(out5, ref5), (d1, d5, e1, e5)
    assert torch.equal(gen(x5[1:3].contiguous(), z5[1:3].contiguous()), out5[1:3])      # rows of a batch == the shard's own run
    assert gen.native().status() == 0
    # the producer waves publish the same range information as the writer: an operand tensor below the format's floor raises bit 1
    sd = T(synth.decoder_state_dict(**meta["synth"]))
    for key in ("g_4.norm_1.linear.weight", "g_4.norm_1.linear.bias"):
        sd[key] = sd[key] * 2.0 ** -20
    outs = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("I2V_DEC_GEN", flag)
        gu = Generator({"channel_factor": meta["synth"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"],
                        "upsample_t": meta["upsample_t"], "spectral_norm": True, "mma": 1})
        gu.load_state_dict(sd)
        gu = gu.cuda().eval()
        outs[flag] = gu(img, z)
        assert gu.native().status(reset=True) == 2, flag
    assert torch.equal(outs["0"], outs["1"])


@pytest.mark.parametrize("mma", [1, 3])
def test_f43_tile_width_switch_across_batches(mma):
    """The F(4,3) launcher narrows its workgroups to 32 channels when 64-channel ones would leave CUs idle -- a decision that
    depends on batch x bricks (round-4 advisor finding: only tested through I2V_W4_BN at one batch).  nf = 8 BAIR: g_1's convs have 4
    workgroups per sample, so B = 1 / 8 run 32-channel workgroups and B = 64 / 96 run 64-channel ones: rows must equal shards.
    Both operand forms (mma = 1 split-fp16, mma = 3 one-term fp16) take the decision from the one launch plan (wino4_plan)."""
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta, mma=mma)
    x0, z, _ = synth.bench_inputs(96, g["img"].shape[-1], 64)
    x0, z = x0.cuda(), z.cuda()
    big = gen(x0, z)
    for lo, hi in ((0, 1), (40, 48), (95, 96), (0, 64)):
        assert torch.equal(gen(x0[lo:hi].contiguous(), z[lo:hi].contiguous()), big[lo:hi]), (lo, hi)


@pytest.mark.parametrize("golden", ["dec_nf8_bair", "dec_nf32_128"])
def test_decoder_in_call_spade_overlap_keeps_the_bits(golden, monkeypatch):
    """Round 5: a forward that finds no prepared maps runs the SPADE branches of all six blocks on the handle's own side stream
    underneath its first levels (I2V_DEC_OVERLAP=0: inline, round 4).  Same kernels: the frames must be the same bits -- also when
    forwards with DIFFERENT start frames follow each other back to back on one handle and workspace (the next call's branches may not
    overwrite maps the previous call still reads), on a non-default stream, and mixed with explicitly prepared calls."""
    g, meta = load_golden(golden)
    monkeypatch.setenv("I2V_DEC_OVERLAP", "0")
    inline = _gen(meta)
    monkeypatch.delenv("I2V_DEC_OVERLAP")
    gen = _gen(meta)
    img, z = cu(g["img"]), cu(g["z"])
    imgs = [img, (img * 0.5 - 0.2).contiguous(), img.flip(-1).contiguous()]
    refs = [inline(x, z) for x in imgs]
    outs = [gen(imgs[i % 3], z) for i in range(12)]              # enqueued back to back, no host synchronisation in between
    for i, o in enumerate(outs):
        assert torch.equal(o, refs[i % 3]), i
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o2 = [gen(imgs[i % 3], z) for i in range(4)]
    torch.cuda.current_stream().wait_stream(side)
    gen.prepare(imgs[1])
    o3 = gen(imgs[1], z)
    o4 = gen(imgs[2], z)
    assert all(torch.equal(o2[i], refs[i % 3]) for i in range(4)) and torch.equal(o3, refs[1]) and torch.equal(o4, refs[2])
    # two streams use ONE handle (one workspace) without ordering each other: the handle serialises its calls (event behind every call)
    s2 = torch.cuda.Stream()
    for s in (side, s2):
        s.wait_stream(torch.cuda.current_stream())
    res = []
    for i in range(6):
        with torch.cuda.stream(side if i % 2 == 0 else s2):
            res.append(gen(imgs[i % 3], z))
    for s in (side, s2):
        torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(res[i], refs[i % 3]) for i in range(6))


def test_decoder_shared_side_stream_keeps_the_bits():
    """Round 6: the decoder handle can run its side work (SPADE branches, learned shortcuts, prepare) on a stream the CALLER owns --
    the cINN prefetch stream (i2v_dec_set_side_stream / Generator.share_side_stream): one side stream per job, the configuration
    bench.py runs at every N.  Same kernels, same events: the pipelined loop in the shared order (decoder of batch k first, the pass
    of batch k+1 behind it on the same stream) must give the frames of the serial loop bit for bit, single calls with a prepare
    too, and handing the stream back (None) must work while work is still queued."""
    import i2v_pipeline
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(T(synth.flow_state_dict(seed=7, embedding_dim=64)))
    flow = flow.cuda().eval()
    xs, rs, es = [], [], []
    for k in range(4):
        x0, r, e = synth.bench_inputs(3, 64, 64)
        xs.append((x0 * (1.0 - 0.2 * k)).cuda().contiguous()); rs.append((r + 0.1 * k).cuda().contiguous()); es.append(e.cuda().contiguous())
    refs = [gen(xs[k], flow(rs[k], es[k], reverse=True).view(3, -1)) for k in range(4)]
    torch.cuda.synchronize()
    pf = i2v_pipeline.LatentPrefetcher(lambda r, e: flow(r, e, reverse=True))
    gen.share_side_stream(pf.stream)
    for rep in range(3):
        outs = []
        tk = pf.submit(rs[0], es[0])
        for k in range(4):
            z = pf.get(tk)
            ev = pf.mark()
            outs.append(gen(xs[k], z.view(3, -1)))
            if k + 1 < 4:
                tk = pf.submit(rs[k + 1], es[k + 1], _ready=ev)
        for k in range(4):
            assert torch.equal(outs[k], refs[k]), (rep, k)
    outs, tk = [], pf.submit(rs[0], es[0])       # the usual order on the shared stream: the pass of batch k + 1 in FRONT of decoder k's side work
    for k in range(4):
        z = pf.get(tk)
        if k + 1 < 4:
            tk = pf.submit(rs[k + 1], es[k + 1])
        outs.append(gen(xs[k], z.view(3, -1)))
    for k in range(4):
        assert torch.equal(outs[k], refs[k]), k
    # single calls: pass on the side stream, prepare behind it on the same stream, then the decoder
    for k in (2, 0):
        tk = pf.submit(rs[k], es[k])
        gen.prepare(xs[k])
        assert torch.equal(gen(xs[k], pf.get(tk).view(3, -1)), refs[k])
    gen.prepare(xs[1])                       # a prepare is pending on the shared stream when the handle gets its own stream back
    gen.share_side_stream(None)
    assert torch.equal(gen(xs[1], flow(rs[1], es[1], reverse=True).view(3, -1)), refs[1])
    assert gen.native().status() == 0


def test_collation_on_the_prefetch_stream_keeps_the_bits():
    """Round 6: a rank of an N > 1 job issues every step's all-gather on the stream its cINN prefetch runs on
    (OverlappedCollator(stream = LatentPrefetcher.stream): three streams at every N).  One GPU, the gather emulated by a device
    copy: on that stream the pass of step k + 1, the gather of step k and the pass of step k + 2 follow each other; every collated
    step must equal the serial call bit for bit, also when result() is only taken every other step (double buffers)."""
    import i2v_dist
    import i2v_pipeline
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(T(synth.flow_state_dict(seed=7, embedding_dim=64)))
    flow = flow.cuda().eval()
    xs, rs, es = [], [], []
    for k in range(5):
        x0, r, e = synth.bench_inputs(3, 64, 64)
        xs.append((x0 * (1.0 - 0.15 * k)).cuda().contiguous()); rs.append((r - 0.1 * k).cuda().contiguous()); es.append(e.cuda().contiguous())
    refs = [gen(xs[k], flow(rs[k], es[k], reverse=True).view(3, -1)).clone() for k in range(5)]
    torch.cuda.synchronize()
    pf = i2v_pipeline.LatentPrefetcher(lambda r, e: flow(r, e, reverse=True))
    col = i2v_dist.OverlappedCollator(3, emulate="copy", stream=pf.stream)
    for every in (1, 2):
        got = {}
        tk = pf.submit(rs[0], es[0])
        for k in range(5):
            z = pf.get(tk)
            if k + 1 < 5:
                tk = pf.submit(rs[k + 1], es[k + 1])
            col.submit(gen(xs[k], z.view(3, -1)))
            if k % every == every - 1 or k == 4:
                got[k] = col.result().clone()
        torch.cuda.synchronize()
        assert col.stream is pf.stream
        for k, v in got.items():
            assert torch.equal(v, refs[k]), (every, k)
    assert gen.native().status() == 0


def test_decoder_prepare_equals_plain_forward():
    """i2v_dec_prepare (Generator.prepare): the SPADE branches of all blocks computed ahead of the forward -- the next forward
    with the same start-frame tensor must give the same bits as a plain one; a forward with ANOTHER tensor in between must
    ignore (and drop) the prepared maps; sub-batching and a prepare issued on a side stream work too."""
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    img, z = cu(g["img"]), cu(g["z"])
    ref = gen(img, z)
    gen.prepare(img)
    assert torch.equal(gen(img, z), ref)
    other = (img * 0.5).contiguous()
    ref_other = gen(other, z)
    gen.prepare(img)
    assert torch.equal(gen(other, z), ref_other)          # different tensor: computed normally
    assert torch.equal(gen(img, z), ref)                  # and the stale prepare was dropped, not reused later
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gen.prepare(img)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(gen(img, z), ref)
    assert rel_l2(ref.cpu(), g["out"]) < TOL


def test_decoder_prepare_never_outlives_its_start_frames():
    """A prepare must not leak into a later call whose start frames sit at the SAME address (round-4 advisor finding): (1) the
    buffer is refilled in place between prepare and forward -- the binding sees the tensor's version counter and cancels;
    (2) a forward that FAILS in between (workspace too small, straight through the C ABI) consumes the prepare, so that a later
    forward on the same pointer -- refilled behind the version counter's back -- recomputes its SPADE maps."""
    import ctypes
    import i2v_native
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    img, z = cu(g["img"]), cu(g["z"])
    other = (img * 0.5 - 0.1).contiguous()
    ref, ref_other = gen(img, z), gen(other, z)
    assert not torch.equal(ref, ref_other)
    buf = img.clone()
    gen.prepare(buf)
    buf.copy_(other)                                      # in-place refill: same address, new version
    assert torch.equal(gen(buf, z), ref_other)
    # (2) same address, contents changed WITHOUT a version bump; the failing call in between must have dropped the prepare
    buf.copy_(img)
    gen.prepare(buf)
    nat = gen.native()
    out = torch.empty_like(ref)
    rc = i2v_native.lib().i2v_dec_forward(nat._h, buf.data_ptr(), buf.shape[2], buf.shape[3], z.data_ptr(), out.data_ptr(),
                                          buf.data_ptr(), 16, buf.shape[0], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0                                        # I2V_E_WORKSPACE
    buf.data.copy_(other)
    torch.cuda.synchronize()
    assert torch.equal(gen(buf, z), ref_other)
    # and the explicit cancel
    buf.data.copy_(img)
    gen.prepare(buf)
    assert i2v_native.lib().i2v_dec_prepare_cancel(nat._h) == 0
    buf.data.copy_(other)
    assert torch.equal(gen(buf, z), ref_other)


def test_decoder_and_embedder_under_graph_capture():
    """Round-5 advisor finding: the usual torch.cuda.graph recipe warms up on stream A and captures on stream B; the handle's
    cross-stream ordering events (recorded behind the warm-up) and a prepare forked before the capture must not leak into the
    capture ("dependency created on uncaptured work in another stream").  Captured Generator.forward / ResnetEncoder.encode:
    everything inline, replays with refilled static inputs equal the eager results bit for bit, and eager calls on other streams
    after the capture still work."""
    from stage2_cINN.AE.modules.AE import ResnetEncoder
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    img, z = cu(g["img"]), cu(g["z"])
    img2, z2 = (img * 0.5 - 0.2).contiguous(), (z * 0.7).contiguous()
    s_warm = torch.cuda.Stream()
    s_warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_warm):                      # warm-up on stream A (allocates the workspace, records the ordering event)
        ref, ref2 = gen(img, z), gen(img2, z2)
        gen.prepare(img)                                  # ... and leaves a FORKED prepare pending on the handle's side stream
    torch.cuda.current_stream().wait_stream(s_warm)
    torch.cuda.synchronize()
    x_s, z_s = img.clone(), z.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # capture on torch's capture stream B
        y_s = gen(x_s, z_s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_s, ref)
    x_s.copy_(img2); z_s.copy_(z2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_s, ref2)
    with torch.cuda.stream(s_warm):                       # eager again, on another stream than the capture: nothing waits on a captured event
        again = gen(img, z)
    torch.cuda.synchronize()
    assert torch.equal(again, ref) and gen.native().status() == 0
    # the embedder's handle orders its calls the same way
    sd = T(synth.embedder_state_dict(seed=3, z_dim=64, norm="in"))
    enc = ResnetEncoder({"z_dim": 64, "deterministic": False, "in_size": 64, "encoder_type": "resnet50", "norm": "in"})
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    with torch.cuda.stream(s_warm):
        e_ref = enc.encode(img).mode()
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        e_s = enc.encode(x_s).mode()
    x_s.copy_(img)
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(e_s, e_ref)


def test_decoder_side_stream_lifetime_and_inference_mode():
    """Round-5 advisor findings: (1) a forked prepare that is never consumed must not outlive its workspace: a forward at a LARGER
    batch replaces the binding's workspace -- the binding joins the handle's side stream first (i2v_dec_join) -- and destroying the
    handle synchronises the side stream; (2) i2v_dec_join through the C ABI; (3) under torch.inference_mode tensors carry no version
    counter: prepare() is a no-op there and Model.synthesize-style use keeps working with the same bits."""
    import ctypes
    import i2v_native
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    img, z = cu(g["img"]), cu(g["z"])
    ref = gen(img, z)
    big_img, big_z = img.repeat(3, 1, 1, 1).contiguous(), z.repeat(3, 1).contiguous()
    for _ in range(3):
        gen2 = _gen(meta)
        gen2.prepare(img)                                 # forked on gen2's side stream, writes gen2's (small) workspace
        big = gen2(big_img, big_z)                        # needs a larger workspace: join, then replace
        assert torch.equal(big[:2], ref) and torch.equal(big[4:], ref)
        gen2.prepare(img)
        del gen2                                          # destroyed with a prepare in flight: the destructor synchronises the side stream
    nat = gen.native()
    gen.prepare(img)
    assert i2v_native.lib().i2v_dec_join(nat._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert torch.equal(gen(img, z), ref)
    with torch.inference_mode():
        xi, zi = img.clone(), z.clone()                   # inference tensors: no version counter
        gen.prepare(xi)
        assert getattr(nat, "_prep", None) is None
        assert torch.equal(gen(xi, zi), ref)
    with pytest.raises(i2v_native.I2VError):
        nat.prepare(img[:, :, ::2])                       # not contiguous: raises BEFORE any state changes
    assert torch.equal(gen(img, z), ref)


def test_decoder_strided_in_place_sequence():
    """i2v_dec_forward_strided / Generator.decode_sequence: the autoregressive loop of get_model.py:68-73 decoded in place into ONE
    [B, 32, 3, H, W] buffer (pass 2 reads its start frames from the strided view seq[:, 15] and writes frames 16..31) must give
    the bits of the reference-shaped loop (torch.cat of dense tensors); prepared SPADE maps work with it."""
    g, meta = load_golden("dec_nf8_bair")
    gen = _gen(meta)
    img, z = synth.bench_inputs(3, g["img"].shape[-1], 64)[:2]
    img, z = img.cuda(), z.cuda()
    seq = gen(img, z)
    ref = torch.cat((seq, gen(seq[:, -1].contiguous(), z)), dim=1)
    ref = torch.cat((ref, gen(ref[:, -1].contiguous(), z)), dim=1)
    got = gen.decode_sequence(img, z, 48)
    assert got.shape == ref.shape == (3, 48, 3, 64, 64) and got.is_contiguous()
    assert torch.equal(got, ref)
    gen.prepare(img)
    assert torch.equal(gen.decode_sequence(img, z, 40), ref)      # 40 -> three passes as well (get_model.py:71: while T < vid_length)
    assert torch.equal(gen.decode_sequence(img, z, 16), seq)
    # a sample-strided start-frame view and an output view in the middle of a larger buffer
    big = torch.full((3, 5, 16, 3, 64, 64), 7.0, device="cuda")
    out = gen(ref[:, 15], z, out=big[:, 2])
    assert out.data_ptr() == big[:, 2].data_ptr() and torch.equal(big[:, 2], ref[:, 16:32])
    assert bool((big[:, 1] == 7.0).all()) and bool((big[:, 3] == 7.0).all())
    with pytest.raises(Exception):
        gen(img, z, out=big[:, :, 0])                              # sample blocks not contiguous


def _write_checkpoints(tmp_path, meta, with_embedder=False, with_encoder=False):
    """Checkpoint tree as get_model.Model expects it (get_model.py:15-43): <stage2>/config_stage2.yaml + cINN.pth,
    <stage1>/config_stage1.yaml + best_PFVD_GEN.pth."""
    import yaml
    s1 = tmp_path / "stage1" / "run"
    s2 = tmp_path / "stage2"
    s1.mkdir(parents=True)
    s2.mkdir()
    (s1 / "config_stage1.yaml").write_text(yaml.safe_dump({"Decoder": {
        "channel_factor": 8, "z_dim": 64, "upsample_s": meta["upsample_s"], "upsample_t": meta["upsample_t"], "spectral_norm": True},
        "Encoder": {"res_type_encoder": "resnet18", "deterministic": False, "use_max_pool": False, "z_dim": 64,
                    "channels": [64, 128, 256, 512, 512], "stride_t": [1, 2, 2, 2], "stride_s": [1, 2, 2, 2]}}))
    torch.save({"state_dict": T(synth.decoder_state_dict(**meta["synth_dec"]))}, s1 / "best_PFVD_GEN.pth")
    (s2 / "config_stage2.yaml").write_text(yaml.safe_dump({
        "Flow": {"n_flows": 20, "flow_hidden_depth": 2, "flow_mid_channels_factor": 8},
        "Conditioning_Model": {"z_dim": 64, "checkpoint_name": "Encoder_stage2", "model_name": "ae/", "model_path": str(tmp_path) + "/"},
        "First_stage_model": {"checkpoint_decoder": "best_PFVD_GEN", "checkpoint_encoder": "best_PFVD_ENC",
                              "model_name": "run", "model_path": str(tmp_path / "stage1") + "/"},
        "Training": {"bs": 50}, "Data": {"img_size": 64}}))
    torch.save({"state_dict": T(synth.flow_state_dict(**meta["synth_flow"]))}, s2 / "cINN.pth")
    if with_encoder:    # First_stage_model.checkpoint_encoder + '.pth.tar' (get_model.py:29)
        torch.save({"state_dict": T(synth.encoder3d_state_dict(seed=9))}, s1 / "best_PFVD_ENC.pth.tar")
    if with_embedder:   # Conditioning_Model.model_path + model_name = <tmp>/ae/ (INN.py:37)
        ae = tmp_path / "ae"
        ae.mkdir()
        (ae / "config_stage2_AE.yaml").write_text(yaml.safe_dump({"AE": {
            "deterministic": False, "in_size": 64, "norm": "in", "encoder_type": "resnet50", "z_dim": 64}}))
        torch.save({"state_dict": T(synth.embedder_state_dict(seed=3, z_dim=64, norm="in"))}, ae / "Encoder_stage2.pth")
    return str(s2) + "/"


def test_model_forward_semantics_vs_golden(tmp_path):
    """get_model.Model from YAML + checkpoints on disk: T = 32 autoregressive, quirk Q3 batch slice."""
    from get_model import Model
    g, meta = load_golden("model_nf8")
    model = Model(_write_checkpoints(tmp_path, meta), 32)
    y32 = model(cu(g["x1"]), residual=cu(g["r1"]), embed=cu(g["e1"]))
    assert y32.shape == (1, 32, 3, 64, 64) and rel_l2(y32.cpu(), g["y32"]) < TOL
    model.vid_length = 2
    yq3 = model(cu(g["x3"]), residual=cu(g["r3"]), embed=cu(g["e3"]))
    assert list(yq3.shape) == list(g["yq3_shape"])  # B=3 > vid_length=2: two SAMPLES come back (Q3)
    assert rel_l2(yq3[:, ::4].cpu(), g["yq3_t4"]) < TOL
    model.vid_length = 20
    assert list(model(cu(g["x1"]), residual=cu(g["r1"]), embed=cu(g["e1"])).shape) == list(g["y20_shape"])
    assert model.synthesize(cu(g["x3"]), residual=cu(g["r3"]), embed=cu(g["e3"])).shape[0] == 3
    # one call overlaps its cINN pass (side stream) with the decoder's SPADE branches: same bits as the strictly serial order
    a = model.synthesize(cu(g["x3"]), residual=cu(g["r3"]), embed=cu(g["e3"]))
    model.overlap = False
    b = model.synthesize(cu(g["x3"]), residual=cu(g["r3"]), embed=cu(g["e3"]))
    assert torch.equal(a, b)


def test_model_from_pixels_with_embedder(tmp_path):
    """Model.forward(x_0) end to end from pixels: ResNet-50 embedder -> cINN inverse -> decoder, vs the CPU oracle chain."""
    from get_model import Model
    from oracle import embedder_ref, model_ref, decoder_ref
    _, meta = load_golden("model_nf8")
    model = Model(_write_checkpoints(tmp_path, meta, with_embedder=True), 16)
    assert model.flow.embedder is not None
    x0, residual, _ = synth.bench_inputs(2, 64, 64)
    out = model(x0.cuda(), residual=residual.cuda())
    esd = T(synth.embedder_state_dict(seed=3, z_dim=64, norm="in"))
    esd64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in esd.items()}
    fsd = T(synth.flow_state_dict(**meta["synth_flow"]))
    dsd = decoder_ref.fold_spectral_norm(T(synth.decoder_state_dict(**meta["synth_dec"])))

    def chain(embed):
        return model_ref.model_forward(fsd, dsd, x0, residual, embed.float().reshape(2, -1), 16, upsample_s=meta["upsample_s"],
                                       upsample_t=meta["upsample_t"], faithful=False)

    ref32 = chain(embedder_ref.encode_mode(esd, x0, "in"))
    ref64 = chain(embedder_ref.encode_mode(esd64, x0.double(), "in"))
    # The 64x64 InstanceNorm embedder is ill-conditioned (test_embedder_vs_oracle): the fp32 oracle embedding sits ~3e-4 from its
    # fp64 evaluation, and the cINN + decoder carry that to the frames.  Same rule as there: 1e-4, or 3x the oracle's OWN
    # fp32-vs-fp64 noise measured on the frames -- not a flat bound.
    noise = rel_l2(ref32, ref64)
    err = rel_l2(out.cpu(), ref64)
    print(f"from pixels: HIP vs oracle(fp64 embedder) {err:.2e}; oracle fp32-vs-fp64 embedder noise on the frames {noise:.2e}")
    assert out.shape == (2, 16, 3, 64, 64) and err < max(TOL, 3 * noise), (err, noise)


def test_generate_samples_cli(tmp_path, monkeypatch):
    """The sampling CLI end to end: PNG start frames -> results.gif (B = 5 images, -bs 2 -> short last batch), and the
    frames it writes against convert_seq2gif(oracle chain) for the same latent / embedding draws (row M3)."""
    from PIL import Image
    import generate_samples
    from oracle import decoder_ref, model_ref
    from utils import auxiliaries as aux
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta)
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(5):
        Image.fromarray(rng.integers(0, 255, (48, 72, 3), dtype=np.uint8)).save(img_dir / f"f{i}.png")
    out_dir = tmp_path / "out"
    generate_samples.main(["-gpu", os.environ.get("HIP_VISIBLE_DEVICES", "0"), "-dataset", "bair", "-ckpt_path", ckpt,
                           "-bs", "2", "-embed_seed", "1", "-img_path", str(img_dir) + "/", "-out_path", str(out_dir) + "/",
                           "-raw_npy", str(out_dir / "frames.npy"), "-seed", "123"])
    gif = Image.open(out_dir / "results.gif")
    assert gif.n_frames == 16 and gif.size == (5 * 64, 64)
    # the same computation through the CPU oracle
    names = sorted(str(p) for p in img_dir.glob("*.png"))
    imgs = generate_samples.load_images(names, 64)
    embeds = torch.randn(5, 64, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(123)
    fsd = T(synth.flow_state_dict(**meta["synth_flow"]))
    dsd = decoder_ref.fold_spectral_norm(T(synth.decoder_state_dict(**meta["synth_dec"])))
    vids = []
    for i in range(3):
        x = imgs[2 * i:2 * i + 2]
        r = torch.randn(x.size(0), 64)
        vids.append(model_ref.model_forward(fsd, dsd, x, r, embeds[2 * i:2 * i + 2], 16, upsample_s=meta["upsample_s"],
                                            upsample_t=meta["upsample_t"], faithful=False))
    ref = aux.convert_seq2gif(torch.cat(vids)).astype(np.uint8)
    raw = np.load(out_dir / "frames.npy")
    assert raw.shape == ref.shape == (16, 64, 5 * 64, 3) and raw.dtype == np.uint8
    diff = np.abs(raw.astype(np.int16) - ref.astype(np.int16))
    assert int(diff.max()) <= 1 and float((diff > 0).mean()) < 0.01, (int(diff.max()), float((diff > 0).mean()))
    # the GIF itself carries the same strip up to palette quantisation
    gif.seek(3)
    g3 = np.asarray(gif.convert("RGB"), dtype=np.int16)
    assert float(np.abs(g3 - ref[3].astype(np.int16)).mean()) < 12.0


def test_sample_prior_loop_vs_oracle():
    """Row N4: the prior-sampling loop of the reference's evaluate_FVD_prior (utils/auxiliaries.py:87-101) -- second caller
    of cINN^-1 + decoder -- over a small loader, vs the oracle chain on the same latent draws."""
    from oracle import decoder_ref, flow_ref
    from stage2_cINN.modules.INN import SupervisedTransformer
    from utils import auxiliaries as aux
    _, meta = load_golden("model_nf8")
    gen = _gen(dict(synth=meta["synth_dec"], upsample_s=meta["upsample_s"], upsample_t=meta["upsample_t"]))

    class PooledEmbedder:   # test scaffolding: a deterministic stand-in for the conditioning embedder (encode(x).mode())
        def encode(self, x):
            e = torch.nn.functional.adaptive_avg_pool2d(x, (4, 4)).reshape(x.size(0), -1)[:, :32]
            e = torch.cat((e, -e), dim=1)[:, :, None, None]
            return type("D", (), {"mode": lambda self_, e=e: e})()

    st = SupervisedTransformer(flow_in_channels=64, flow_mid_channels=512, flow_hidden_depth=2, n_flows=20,
                               flow_conditioning_option="None", flow_embedding_channels=64, control=False, dic=None,
                               embedder=PooledEmbedder())
    fsd = T(synth.flow_state_dict(**meta["synth_flow"]))
    st.flow.load_state_dict(fsd)
    st = st.cuda().eval()
    g = torch.Generator().manual_seed(17)
    loader = [{"seq": 2 * torch.rand(b, 17, 3, 64, 64, generator=g) - 1} for b in (2, 1)]
    seq_gen, seq_orig = aux.sample_prior(loader, st, gen, 64, generator=torch.Generator().manual_seed(5))
    assert seq_gen.shape == (3, 16, 3, 64, 64) and seq_orig.shape == (3, 16, 3, 64, 64) and not seq_gen.is_cuda
    assert torch.equal(seq_orig, torch.cat([f["seq"][:, 1:] for f in loader]))
    dsd = decoder_ref.fold_spectral_norm(T(synth.decoder_state_dict(**meta["synth_dec"])))
    gr = torch.Generator().manual_seed(5)
    refs = []
    for f in loader:
        x0 = f["seq"][:, 0]
        res = torch.randn(x0.size(0), 64, generator=gr)
        emb = PooledEmbedder().encode(x0).mode().reshape(x0.size(0), -1)
        z = flow_ref.flow_reverse(fsd, res, emb).view(x0.size(0), -1)
        refs.append(decoder_ref.generator(dsd, x0, z, meta["upsample_s"], meta["upsample_t"], faithful=False))
    assert rel_l2(seq_gen, torch.cat(refs)) < TOL


@pytest.mark.parametrize("norm,size", [("in", 64), ("bn", 128), ("in", 128)])
def test_embedder_vs_oracle(norm, size):
    """Row N1: ResnetEncoder.encode(x).mode() on the HIP path vs the (unpinned, see oracle/embedder_ref.py) CPU restatement."""
    from oracle import embedder_ref
    from stage2_cINN.AE.modules.AE import ResnetEncoder
    sd = T(synth.embedder_state_dict(seed=3, z_dim=64, norm=norm))
    enc = ResnetEncoder({"z_dim": 64, "deterministic": False, "in_size": size, "encoder_type": "resnet50", "norm": norm})
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    x = 2 * torch.rand(3, 3, size, size, generator=torch.Generator().manual_seed(9)) - 1
    ref32 = embedder_ref.encode_mode(sd, x, norm)
    sd64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}
    ref64 = embedder_ref.encode_mode(sd64, x.double(), norm)
    out = enc.encode(x.cuda()).mode()
    assert out.shape == (3, 64, 1, 1)
    # InstanceNorm over the 2x2 / 4x4 maps of the last stages (64x64 inputs) is ill-conditioned: the fp32 CPU oracle itself
    # sits 2.9e-4 (64^2) / 1.4e-5 (128^2) from its fp64 evaluation.  Gate: 1e-4, or 3x the oracle's own fp32 noise.
    noise = rel_l2(ref32, ref64)
    assert rel_l2(out.cpu(), ref64) < max(TOL, 3 * noise), (rel_l2(out.cpu(), ref64), noise)


@pytest.mark.parametrize("name", ["enc3d_bair", "enc3d_land"])
def test_motion_encoder_vs_golden(name):
    """Row N3: Encoder.forward (3D ResNet-18) on the HIP path vs the reference module's outputs."""
    from stage1_VAE.modules.resnet3D import Encoder
    from test_oracle_golden import golden_clip
    g, meta = load_golden(name)
    a = meta["synth"]
    enc = Encoder({"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": 64, "channels": a["channels"],
                   "stride_s": a["stride_s"], "stride_t": meta["stride_t"]})
    enc.load_state_dict(T(synth.encoder3d_state_dict(**a)))
    enc = enc.cuda().eval()
    x = golden_clip(meta, g).cuda()
    sample, mu, logvar = enc(x)
    assert rel_l2(mu.cpu(), g["mu"]) < TOL and rel_l2(logvar.cpu(), g["logvar"]) < TOL
    assert sample.shape == mu.shape and bool(torch.isfinite(sample).all())
    _, mu2, _ = enc(x.transpose(1, 2).contiguous())   # [B,T,3,H,W] is transposed like the reference does (resnet3D.py:206-207)
    assert torch.equal(mu2, mu)


def test_model_transfer_vs_oracle(tmp_path):
    """Model.transfer (get_model.py:77-103): encoder -> cINN forward -> cINN inverse on new start frames -> decoder."""
    from get_model import Model
    from oracle import decoder_ref, encoder_ref, flow_ref
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta, with_encoder=True)
    model = Model(ckpt, 16, transfer=True)
    gsd = torch.Generator().manual_seed(5)
    query = 2 * torch.rand(1, 17, 3, 64, 64, generator=gsd) - 1
    x0 = 2 * torch.rand(2, 3, 64, 64, generator=gsd) - 1
    eq, e0 = torch.randn(1, 64, generator=gsd), torch.randn(2, 64, generator=gsd)
    out = model.transfer(query.cuda(), x0.cuda(), embed_query=eq.cuda(), embed=e0.cuda())
    esd = T(synth.encoder3d_state_dict(seed=9))
    fsd = T(synth.flow_state_dict(**meta["synth_flow"]))
    dsd = decoder_ref.fold_spectral_norm(T(synth.decoder_state_dict(**meta["synth_dec"])))
    mu, _ = encoder_ref.encoder(esd, query[:, 1:].transpose(1, 2))
    res, _ = flow_ref.flow_forward(fsd, mu, eq)
    z_ref = flow_ref.flow_reverse(fsd, res.view(1, -1).repeat(2, 1), e0).view(2, -1)
    ref = decoder_ref.generator(dsd, x0, z_ref, meta["upsample_s"], meta["upsample_t"], faithful=False)
    assert out.shape == (2, 16, 3, 64, 64) and rel_l2(out.cpu(), ref) < TOL


def test_model_control_variant_vs_oracle(tmp_path):
    """Row N2: endpoint-controlled sampling (Training.control = True): E = 64 + 30, blocks fl % 4 != 0 in mode 'cond',
    embed_pos one-hots (INN.py:49-57, flow_blocks.py:24) -- Model.forward(x_0, cond=pos) vs the oracle chain."""
    import yaml
    from get_model import Model
    from oracle import decoder_ref, flow_ref
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta)
    cfg = yaml.safe_load(open(ckpt + "config_stage2.yaml"))
    cfg["Training"]["control"] = True
    open(ckpt + "config_stage2.yaml", "w").write(yaml.safe_dump(cfg))
    fargs = dict(seed=7, n_flows=20, embedding_dim=94, control=True)
    torch.save({"state_dict": T(synth.flow_state_dict(**fargs))}, ckpt + "cINN.pth")
    model = Model(ckpt, 16)
    x0, residual, embed = synth.bench_inputs(3, 64, 64)
    pos = torch.tensor([[0.05, 0.5, 1.0], [0.31, 0.999, 0.1001], [0.7, 0.2, 0.45]])
    out = model(x0.cuda(), cond=pos, residual=residual.cuda(), embed=embed.cuda())
    full = torch.cat((embed, flow_ref.embed_pos(pos)), dim=1)
    z = flow_ref.flow_reverse(T(synth.flow_state_dict(**fargs)), residual, full, control=True).view(3, -1)
    ref = decoder_ref.generator(decoder_ref.fold_spectral_norm(T(synth.decoder_state_dict(**meta["synth_dec"]))), x0, z,
                                meta["upsample_s"], meta["upsample_t"], faithful=False)
    assert out.shape == (3, 16, 3, 64, 64) and rel_l2(out.cpu(), ref) < TOL


def test_generate_transfer_cli(tmp_path):
    from PIL import Image
    import generate_transfer
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta, with_embedder=True, with_encoder=True)
    rng = np.random.default_rng(1)
    for v in range(2):
        d = tmp_path / "clips" / f"v{v}"
        d.mkdir(parents=True)
        for i in range(17):
            Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(d / f"{i:03d}.png")
    out_dir = tmp_path / "out"
    generate_transfer.main(["-gpu", os.environ.get("HIP_VISIBLE_DEVICES", "0"), "-dataset", "bair", "-ckpt_path", ckpt, "-seq_length", "17",
                            "-img_path", str(tmp_path / "clips") + "/", "-out_path", str(out_dir) + "/"])
    gif = Image.open(out_dir / "transfer_1.gif")
    assert gif.n_frames == 17 and gif.size == (3 * 64, 64)


def test_full_size_bair_b8_every_row_vs_oracle():
    """BASELINE geometry (nf = 64, 64x64x16) at the per-GPU batch of the 8-GPU job (B = 8): EVERY row of the HIP decoder
    output against the CPU oracle on the same seeded inputs (a few seconds of CPU work on the GPU box's host cores), plus
    the shard property (rows of the full batch == shard runs, bit for bit)."""
    from oracle import decoder_ref
    from stage1_VAE.modules.decoder import Generator
    sd = T(synth.decoder_state_dict(seed=7, channel_factor=64))
    gen = Generator({"channel_factor": 64, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True})
    gen.load_state_dict(sd)
    gen = gen.cuda().eval()
    x0, residual, _ = synth.bench_inputs(8, 64, 64)
    out = gen(x0.cuda(), residual.cuda())
    assert out.shape == (8, 16, 3, 64, 64) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref = decoder_ref.generator(decoder_ref.fold_spectral_norm(sd), x0, residual, faithful=False)
    for b in range(8):
        assert rel_l2(out[b].cpu(), ref[b]) < TOL, b
    lo = gen(x0[:3].cuda().contiguous(), residual[:3].cuda().contiguous())
    hi = gen(x0[3:].cuda().contiguous(), residual[3:].cuda().contiguous())
    assert torch.equal(torch.cat((lo, hi)), out)
    assert gen.native().status() == 0


def test_cfg1_exact_inputs_vs_oracle():
    """BASELINE configs[0] -- the CPU reference's own case, BAIR 64x64, seq_len 16, batch 4 -- on its exact bench inputs
    (x_0 seed 1234, residual seed 4321, embedding seed 2468, weights seed 7): cINN inverse + decoder on the HIP path against
    the oracle chain that bench.py times as `cpu_baseline` (oracle/model_ref.synthesize, faithful variant)."""
    from oracle import model_ref
    from stage1_VAE.modules.decoder import Generator
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    fsd = T(synth.flow_state_dict(seed=7, embedding_dim=64))
    dsd = T(synth.decoder_state_dict(seed=7, channel_factor=64))
    flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(fsd)
    gen = Generator({"channel_factor": 64, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True})
    gen.load_state_dict(dsd)
    flow, gen = flow.cuda().eval(), gen.cuda().eval()
    x0, residual, embed = synth.bench_inputs(4, 64, 64)
    z = flow(residual.cuda(), embed.cuda(), reverse=True).view(4, -1)
    seq = gen(x0.cuda(), z)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref = model_ref.synthesize(fsd, dsd, x0, residual, embed, 16, (2, 1), (2, 1), faithful=True)
    assert seq.shape == tuple(ref.shape) == (4, 16, 3, 64, 64)
    for b in range(4):
        assert rel_l2(seq[b].cpu(), ref[b]) < TOL, b
    assert gen.native().status() == 0


def _range_sweep(exps):
    """One GeneratorBlock (128 -> 128, identity shortcut, [1,128,4,16,16]: both 3x3x3 convs run the Winograd split-fp16
    kernel) whose conv_1 OPERANDS are scaled by s = 2**k exactly: ADAIN's Linear (weight and bias -> gamma, beta) is
    multiplied by s, so lrelu(gamma * norm + beta) -- the tensor that is split into fp16 hi / lo parts and Winograd-
    transformed -- and with it the conv output scale by s; the input x of the identity shortcut is scaled by s too, so the
    whole block output is s times the unscaled one (conv_1's bias is set to zero) and rel-L2 stays meaningful.  (SPADE's (1 + gamma) pins conv_0's
    operands at O(1); conv_0 and conv_1 run the same kernel.)  Returns [(k, rel-L2 vs the oracle, range flag)]."""
    from oracle import decoder_ref
    from stage1_VAE.modules import decoder as dec
    base = T(synth.decoder_state_dict(seed=11, channel_factor=8))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 128, 4, 16, 16, generator=g)
    img = 2 * torch.rand(1, 3, 16, 16, generator=g) - 1
    z = torch.randn(1, 64, generator=g)
    rows = []
    for k in exps:
        s = float(2.0 ** k)
        sd = dict(base)
        for key in ("g_0.norm_1.linear.weight", "g_0.norm_1.linear.bias"):
            sd[key] = base[key] * s
        sd["g_0.conv_1.bias"] = torch.zeros_like(base["g_0.conv_1.bias"])   # (an unscaled bias would swamp the conv term at small s)
        blk = dec.GeneratorBlock(128, 128, True, 64)
        blk.load_state_dict(sub(sd, "g_0."))
        blk = blk.cuda().eval()
        ref = decoder_ref.generator_block(sd, "g_0", x * s, z, img)
        out = blk(x.cuda() * s, z.cuda(), img.cuda())
        flag = blk.native().status(reset=True)
        rows.append((k, rel_l2(out.cpu(), ref), flag))
    return rows


def test_split_fp16_dynamic_range():
    """Where the split-fp16 operand format (hi = fp16(x), lo = fp16(x - hi)) holds the 1e-4 gate: at the top it ends at the
    fp16 range (65 504; the sticky range flag must then be raised instead of returning garbage silently), at the bottom the
    lo part becomes an fp16 subnormal for |x| < 2^-3 and the 2^-22 relative precision degrades towards 2^-11 at 2^-14.
    The measured table is in INTEGRATION.md; the gate is asserted over operand scales 2^-12 .. 2^10 around the synthetic O(1)
    regime."""
    rows = _range_sweep([-12, -8, -4, 0, 4, 8, 10])
    for k, err, flag in rows:
        assert err < TOL and flag & 1 == 0, rows          # in range: exact enough and no overflow flag
        assert k < -8 or flag == 0, rows                  # and no underflow warning anywhere near the O(1) regime
    top = _range_sweep([16])[0]
    assert top[2] & 1 or top[1] < TOL, top     # past the fp16 range: flagged (or still exact), never silently wrong
    # the bottom: below ~2^-13 the 2^-25 absolute floor of the format breaks the gate -- the underflow bit (status bit 1) says so
    low = _range_sweep([-14, -16, -20])
    for k, err, flag in low:
        assert flag & 2 or err < TOL, low                 # never silently imprecise
        assert flag & 1 == 0, low
    assert low[-1][2] & 2, low                            # a tensor 2^-20 below the O(1) regime is always reported


def test_model_128_t32_vs_golden():
    """BASELINE cfg5 geometry (128x128, nf = 32, E = 128, vid_length = 32 -> two dependent decoder passes, B = 2) against
    the reference-generated fixture (get_model.py:65-75 sequence driven with the reference flow + decoder)."""
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    g, meta = load_golden("model_nf32_128_t32")
    flow = ConditionalFlow(64, 128, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(T(synth.flow_state_dict(**meta["synth_flow"])))
    flow = flow.cuda().eval()
    gen = _gen(dict(synth=meta["synth_dec"], upsample_s=meta["upsample_s"], upsample_t=meta["upsample_t"]))
    z = flow(cu(g["r"]), cu(g["e"]), reverse=True).view(2, -1)
    assert rel_l2(z.cpu(), g["z"]) < TOL
    x0 = cu(g["x0"])
    seq = gen(x0, z)
    while seq.shape[1] < 32:
        seq = torch.cat((seq, gen(seq[:, -1].contiguous(), z)), dim=1)
    assert torch.equal(gen.decode_sequence(x0, z, 32), seq)       # the in-place form Model.decode uses: same bits
    assert seq.shape == (2, 32, 3, 128, 128) and bool(torch.isfinite(seq).all())
    assert rel_l2(seq[:, :16, :, ::4, ::4].cpu(), g["out_s4"][:, :16]) < TOL
    assert rel_l2(seq[:, 16:, :, ::4, ::4].cpu(), g["out_s4"][:, 16:]) < TOL   # second (autoregressive) pass


@pytest.mark.parametrize("golden,batch,rows", [("dec_nf64_bair", 64, ((0, 8), (24, 32), (56, 64))),
                                                ("dec_nf32_128", 32, ((0, 8), (24, 32))),
                                                ("dec_nf32_128", 256, ((0, 8), (120, 128), (248, 256)))])  # cfg4, strong, N = 1
def test_baseline_batch_rows_equal_shards_and_golden(golden, batch, rows):
    """BASELINE cfg2 (BAIR nf = 64, B = 64) / cfg3 (128x128 nf = 32, B = 32): the full-batch decoder output is what
    bench.py times.  Its rows must equal the B = 8 shard runs bit for bit (tile selection depends on the batch: samples per
    brick, channel-tile narrowing, bricks with b0 > 0), and the row that carries the committed golden sample must match
    the reference-generated frames."""
    g, meta = load_golden(golden)
    gen = _gen(meta)
    size = g["img"].shape[-1]
    x0, residual, _ = synth.bench_inputs(batch, size, 64)
    x0[5], residual[5] = torch.from_numpy(g["img"][0]), torch.from_numpy(g["z"][0])
    x0, z = x0.cuda(), residual.cuda()
    out = gen(x0, z)
    assert out.shape == (batch, 16, 3, size, size) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    assert rel_l2(out[5:6, ..., ::2, ::2].cpu(), g["out_s2"]) < TOL
    for lo, hi in rows:
        shard = gen(x0[lo:hi].contiguous(), z[lo:hi].contiguous())
        assert torch.equal(shard, out[lo:hi]), (lo, hi, float((shard - out[lo:hi]).abs().max()))
    assert gen.native().status() == 0


def test_cfg5_share_b16_t32_rows_equal_shards_and_golden():
    """BASELINE cfg5's per-GPU share (128x128 geometry, nf = 32, E = 128, B = 16, vid_length 32 = two dependent decoder
    passes, the second one started from the first one's last frame): every row must equal the B = 8 shard runs bit for bit
    over all 32 frames, and the rows carrying the committed fixture's two samples must match the reference frames."""
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    g, meta = load_golden("model_nf32_128_t32")
    flow = ConditionalFlow(64, 128, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(T(synth.flow_state_dict(**meta["synth_flow"])))
    flow = flow.cuda().eval()
    gen = _gen(dict(synth=meta["synth_dec"], upsample_s=meta["upsample_s"], upsample_t=meta["upsample_t"]))
    x0, residual, embed = synth.bench_inputs(16, 128, 128)
    for row, k in ((3, 0), (12, 1)):
        x0[row], residual[row], embed[row] = torch.from_numpy(g["x0"][k]), torch.from_numpy(g["r"][k]), torch.from_numpy(g["e"][k])
    x0, residual, embed = x0.cuda(), residual.cuda(), embed.cuda()

    def run(lo, hi):
        z = flow(residual[lo:hi].contiguous(), embed[lo:hi].contiguous(), reverse=True).view(hi - lo, -1)
        seq = gen(x0[lo:hi].contiguous(), z)
        while seq.shape[1] < 32:
            seq = torch.cat((seq, gen(seq[:, -1].contiguous(), z)), dim=1)
        return z, seq

    z, seq = run(0, 16)
    assert seq.shape == (16, 32, 3, 128, 128) and bool(torch.isfinite(seq).all()) and float(seq.abs().max()) <= 1.0
    for row, k in ((3, 0), (12, 1)):
        assert rel_l2(z[row:row + 1].cpu(), g["z"][k:k + 1]) < TOL
        assert rel_l2(seq[row:row + 1, :, :, ::4, ::4].cpu(), g["out_s4"][k:k + 1]) < TOL
    for lo, hi in ((0, 8), (8, 16)):
        zs, ss = run(lo, hi)
        assert torch.equal(zs, z[lo:hi]) and torch.equal(ss, seq[lo:hi]), (lo, hi)
    assert gen.native().status() == 0


@pytest.mark.parametrize("case", ["bair_nf64", "land_nf32", "bair_nf64_f23"])
def test_determinism_soak(case, monkeypatch):
    """Intermittent-fault coverage: round 3 found two one-in-hundreds races (an under-waited loop entry of the Winograd kernel,
    an in-place state in the cINN tail) that single-shot parity tests passed.  300 decoder forwards per case -- together every
    instantiation of the F(4,3) kernel (<9,64>, <6,64>, <3,64> in the BAIR nf = 64 decoder, <9,32> / <6,32> in the 128x128 nf = 32
    one) and of the F(2,3) kernel (g_1; everything with I2V_DEC_WINO4=0) -- every output compared with the first ON THE DEVICE
    (no sync inside the loop, so launches run back to back), every second forward with the cINN chain running on a side
    stream underneath (irregular workgroup dispatch: the situation in which both round-3 races showed)."""
    from stage1_VAE.modules.decoder import Generator
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    if case == "bair_nf64_f23":
        monkeypatch.setenv("I2V_DEC_WINO4", "0")
    nf, size, ups, B, n = (32, 128, [2, 2], 1, 300) if case == "land_nf32" else (64, 64, [2, 1], 2, 300 if case == "bair_nf64" else 150)
    gen = Generator({"channel_factor": nf, "z_dim": 64, "upsample_s": ups, "upsample_t": [2, 1], "spectral_norm": True})
    gen.load_state_dict(T(synth.decoder_state_dict(seed=7, channel_factor=nf)))
    gen = gen.cuda().eval()
    flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(T(synth.flow_state_dict(seed=7, embedding_dim=64)))
    flow = flow.cuda().eval()
    x0, residual, embed = synth.bench_inputs(B, size, 64)
    x0, residual, embed = x0.cuda(), residual.cuda(), embed.cuda()
    z = flow(residual, embed, reverse=True).view(B, -1).clone()
    first = gen(x0, z).clone()
    ndiff = torch.zeros((), dtype=torch.int64, device="cuda")
    zdiff = torch.zeros((), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream(priority=-1)
    for it in range(n):
        if it & 1:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                zi = flow(residual, embed, reverse=True).view(B, -1)
                zdiff += (zi != z).sum()
        out = gen(x0, z)
        ndiff += (out != first).sum()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(ndiff) == 0 and int(zdiff) == 0, (case, int(ndiff), int(zdiff))
    assert gen.native().status() == 0


@pytest.mark.parametrize("emb", [64, 128])
def test_flow_fp16_operand_mode(emb):
    """BASELINE configs[4] names an "fp16 MFMA conditioning GEMM" variant of the cINN: ``ConditionalFlow.linear_f16 = 1`` runs
    every Linear of the s- / t-nets on v_mfma_f32_16x16x16_f16 (weights rounded to fp16 at load, activations per layer, fp32
    accumulation).  It is pinned twice: TIGHTLY against the oracle with the same operand rounding emulated (only the fp32
    summation order differs), and LOOSELY against the fp32 reference path -- its tolerance is reported separately from the
    1e-4 fp32 gate, as SURVEY §8d allows (the measured values are printed and recorded in INTEGRATION.md)."""
    from oracle import flow_ref
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    sd = T(synth.flow_state_dict(seed=7, embedding_dim=emb))
    _, residual, embed = synth.bench_inputs(24, 64, emb)
    flows = []
    for f16 in (0, 1):
        flow = ConditionalFlow(64, emb, 512, 2, 20, conditioning_option="None")
        flow.load_state_dict(sd)
        flow.linear_f16 = f16
        flows.append(flow.cuda().eval())
    assert flows[1].native().param_bytes < 0.52 * flows[0].native().param_bytes     # half the streamed weight bytes
    z32 = flows[0](residual.cuda(), embed.cuda(), reverse=True).view(24, -1).cpu()
    z16 = flows[1](residual.cuda(), embed.cuda(), reverse=True).view(24, -1).cpu()
    with flow_ref.linear_f16_emulation():
        zr16 = flow_ref.flow_reverse(sd, residual, embed).reshape(24, -1)
        ztr16, ldr16 = flow_ref.flow_forward(sd, residual, embed)
    zr32 = flow_ref.flow_reverse(sd, residual, embed).reshape(24, -1)
    assert rel_l2(z32, zr32) < TOL
    e_emul, e_fp32 = rel_l2(z16, zr16), rel_l2(z16, zr32)
    print(f"fp16-operand cINN (E = {emb}): z rel-L2 vs emulated oracle {e_emul:.2e}, vs fp32 oracle {e_fp32:.2e}")
    # measured on MI355X (round 5): E = 64: 3.3e-4 / 4.2e-4, E = 128: 2.2e-4 / 3.1e-4; bounds = ~2x the larger (a rounding flip of one
    # activation costs 2^-11 on that element)
    assert e_emul < 6e-4 and e_fp32 < 9e-4, (e_emul, e_fp32)
    assert not torch.equal(z16, z32)                      # the mode really changes the arithmetic
    zt16, ld16 = flows[1](residual.cuda(), embed.cuda())
    e_zt = rel_l2(zt16.view(24, -1).cpu(), ztr16.reshape(24, -1))
    e_ld = float(np.max(np.abs(ld16.cpu().numpy().reshape(-1) - np.asarray(ldr16).reshape(-1)) / (1.0 + np.abs(np.asarray(ldr16).reshape(-1)))))
    print(f"fp16-operand cINN forward: z~ rel-L2 vs emulated oracle {e_zt:.2e}, log-det max |err| / (1 + |ld|) {e_ld:.2e}")
    assert e_zt < 6e-4 and e_ld < 4e-4, (e_zt, e_ld)   # measured 3.2e-4 / 1.3e-4
    # shards equal the full batch bit for bit in this mode too
    zs = flows[1](residual[8:16].cuda().contiguous(), embed[8:16].cuda().contiguous(), reverse=True).view(8, -1).cpu()
    assert torch.equal(zs, z16[8:16])


def test_flow_large_batches_vs_oracle():
    """cINN at per-GPU batches above 64 (cfg4 / cfg5 on fewer than 8 GPUs): B = 128 and 256 -- the Bp/64 > 1 grids."""
    from oracle import flow_ref
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    sd = T(synth.flow_state_dict(seed=7, embedding_dim=128))
    flow = ConditionalFlow(64, 128, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(sd)
    flow = flow.cuda().eval()
    _, residual, embed = synth.bench_inputs(256, 64, 128)
    ref = flow_ref.flow_reverse(sd, residual, embed).reshape(256, 64)
    for B in (256, 128, 200):
        z = flow(residual[:B].cuda().contiguous(), embed[:B].cuda().contiguous(), reverse=True).reshape(B, 64)
        assert rel_l2(z.cpu(), ref[:B]) < TOL, B
    zt, ld = flow(residual[:128].cuda().contiguous(), embed[:128].cuda().contiguous())
    ztr, ldr = flow_ref.flow_forward(sd, residual[:128], embed[:128])
    assert rel_l2(zt.reshape(128, 64).cpu(), ztr.reshape(128, 64)) < TOL and np.allclose(ld.cpu(), ldr, rtol=1e-4, atol=1e-4)
    # the reference's last_outs / last_logdets side effect (flow_blocks.py:34-35,49-50) is opt-in
    flow.record_intermediates = True
    zt2, ld2 = flow(residual[:4].cuda().contiguous(), embed[:4].cuda().contiguous())
    assert len(flow.last_outs) == 20 and len(flow.last_logdets) == 20
    assert rel_l2(zt2.reshape(4, 64).cpu(), ztr.reshape(128, 64)[:4]) < TOL and np.allclose(ld2.cpu(), ldr[:4], rtol=1e-4, atol=1e-4)
    # as in the reference (checked by running it): 2-D block outputs, CUMULATIVE log-dets
    assert all(t.shape == (4, 64) for t in flow.last_outs) and all(t.shape == (4,) for t in flow.last_logdets)
    assert np.allclose(flow.last_logdets[-1].cpu(), ldr[:4], rtol=1e-4, atol=1e-4)
    assert float(flow.last_logdets[0].abs().max()) > 0 and not torch.equal(flow.last_logdets[0], flow.last_logdets[-1])


def test_generic_flow_chain_and_other_geometries(monkeypatch):
    """The two implementations of the cINN launch chain: the matrix-core tile chain (csrc/i2v_flow_tile.hip, the default
    for the shipped geometry) and the generic vector-ALU chain (I2V_FLOW_TILE=0; also what hidden_dim % 128 != 0 or
    depth 0 fall back to).  Same goldens, same gates; hidden widths 128 / 256 / 384 (1, 2, 3 k-blocks per wave of the
    tile kernels), depth 1 and 3, a width only the generic chain covers (192), and every sample-tile grouping NS."""
    from oracle import flow_ref
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    monkeypatch.setenv("I2V_FLOW_TILE", "0")
    for name in ("flow_full_e64", "flow_full_ctrl"):
        g, meta = load_golden(name)
        a = meta["synth"]
        flow = ConditionalFlow(64, a["embedding_dim"], 512, 2, 20, conditioning_option="None", control=a["control"])
        flow.load_state_dict(T(synth.flow_state_dict(**a)))
        flow = flow.cuda().eval()
        x, e = cu(g["x"]), cu(g["e"])
        zt, ld = flow(x, e)
        assert rel_l2(zt.reshape(8, 64).cpu(), g["fwd"]) < TOL and np.allclose(ld.cpu(), g["logdet"], rtol=1e-4, atol=1e-4)
        z = flow(x, e, reverse=True)
        assert rel_l2(z.reshape(8, 64).cpu(), g["rev"]) < TOL
    monkeypatch.delenv("I2V_FLOW_TILE")
    _, residual, embed = synth.bench_inputs(70, 64, 64)
    for hidden, depth, nfl in ((128, 2, 3), (256, 1, 3), (384, 3, 2), (192, 2, 2)):
        sd = T(synth.flow_state_dict(seed=3, embedding_dim=64, n_flows=nfl, hidden_dim=hidden, hidden_depth=depth))
        flow = ConditionalFlow(64, 64, hidden, depth, nfl, conditioning_option="None")
        flow.load_state_dict(sd)
        flow = flow.cuda().eval()
        for B in (70, 16, 3):
            ref = flow_ref.flow_reverse(sd, residual[:B], embed[:B], n_flows=nfl, depth=depth).reshape(B, 64)
            z = flow(residual[:B].cuda().contiguous(), embed[:B].cuda().contiguous(), reverse=True).reshape(B, 64)
            assert rel_l2(z.cpu(), ref) < TOL, (hidden, depth, B)
        ztr, ldr = flow_ref.flow_forward(sd, residual[:21], embed[:21], n_flows=nfl, depth=depth)
        zt, ld = flow(residual[:21].cuda().contiguous(), embed[:21].cuda().contiguous())
        assert rel_l2(zt.reshape(21, 64).cpu(), ztr.reshape(21, 64)) < TOL and np.allclose(ld.cpu(), ldr, rtol=1e-4, atol=1e-4)
    # sample-tile grouping of the hidden-layer workgroups: any NS gives the same bits
    sd = T(synth.flow_state_dict(seed=7, embedding_dim=64))
    outs = []
    for ns in ("1", "2", "4"):
        monkeypatch.setenv("I2V_FLOW_NS", ns)
        flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
        flow.load_state_dict(sd)
        flow = flow.cuda().eval()
        outs.append(flow(residual.cuda(), embed.cuda(), reverse=True))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_flow_fold_keeps_the_bits(monkeypatch):
    """Round 5: the tail of every half-step is folded into the first hidden layer's launch (flow_first_tile_kernel: 82 launches per
    pass instead of 122; I2V_FLOW_FOLD=0 restores round 4's chain).  Same operations in the same order: both directions, the log-det,
    the control geometry ('cond' blocks: first Linear without state channels), fp16-operand mode, ragged batches over every sample-
    tile grouping, and depth 1 (the folded layer is also the last hidden one: partial-product buffers alternate) give the same bits."""
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    _, residual, embed = synth.bench_inputs(150, 64, 128)
    cases = [dict(emb=64, hidden=512, depth=2, nfl=20, control=False, f16=0, Bs=(64, 8, 3, 150)),
             dict(emb=128, hidden=512, depth=2, nfl=20, control=False, f16=1, Bs=(24, 130)),
             dict(emb=94, hidden=512, depth=2, nfl=20, control=True, f16=0, Bs=(21,)),
             dict(emb=64, hidden=256, depth=1, nfl=3, control=False, f16=0, Bs=(70, 5)),
             dict(emb=64, hidden=384, depth=3, nfl=2, control=False, f16=0, Bs=(33,))]
    for cse in cases:
        sd = T(synth.flow_state_dict(seed=11, embedding_dim=cse["emb"], n_flows=cse["nfl"], hidden_dim=cse["hidden"],
                                     hidden_depth=cse["depth"], control=cse["control"]))
        outs = {}
        for fold in ("0", "1"):
            monkeypatch.setenv("I2V_FLOW_FOLD", fold)
            flow = ConditionalFlow(64, cse["emb"], cse["hidden"], cse["depth"], cse["nfl"], conditioning_option="None", control=cse["control"])
            flow.load_state_dict(sd)
            flow.linear_f16 = cse["f16"]
            flow = flow.cuda().eval()
            res = []
            for B in cse["Bs"]:
                r, e = residual[:B].cuda().contiguous(), embed[:B, :cse["emb"]].cuda().contiguous()
                z = flow(r, e, reverse=True)
                zt, ld = flow(r, e)
                res += [z, zt, ld, flow(r, e, reverse=True)]      # (the last one replays the captured graph)
            outs[fold] = res
        monkeypatch.delenv("I2V_FLOW_FOLD")
        for k, (a, b) in enumerate(zip(outs["0"], outs["1"])):
            assert torch.equal(a, b), (cse, k, float((a - b).abs().max()))


def test_pipelined_sampling_equals_serial():
    """i2v_pipeline.LatentPrefetcher: the cINN pass of batch k+1 on a high-priority side stream underneath the decoder of
    batch k.  The chain's workgroups are then dispatched irregularly between the decoder's -- the situation in which a
    missing inter-workgroup ordering inside a launch shows (round 3 found one: the row-group workgroups of a tail launch read
    the state a sibling was already overwriting).  Every latent and every frame must equal the serial loop bit for bit."""
    import i2v_pipeline
    from stage1_VAE.modules.decoder import Generator
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(T(synth.flow_state_dict(seed=7, embedding_dim=64)))
    # full-width decoder: its conv workgroups fill every CU (136 KB LDS each), so the chain's workgroups trickle in one by one
    gen = Generator({"channel_factor": 64, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True})
    gen.load_state_dict(T(synth.decoder_state_dict(seed=7, channel_factor=64)))
    flow, gen = flow.cuda().eval(), gen.cuda().eval()
    nb, B = 8, 8
    x0, residual, embed = synth.bench_inputs(nb * B, 64, 64)
    x0, residual, embed = x0.cuda(), residual.cuda(), embed.cuda()
    sl = lambda k: slice(k * B, (k + 1) * B)
    zs = [flow(residual[sl(k)].contiguous(), embed[sl(k)].contiguous(), reverse=True).view(B, -1).clone() for k in range(nb)]
    seqs = [gen(x0[sl(k)].contiguous(), zs[k]).clone() for k in range(nb)]
    torch.cuda.synchronize()
    for trial in range(3):
        pf = i2v_pipeline.LatentPrefetcher(lambda r, e: flow(r, e, reverse=True))
        ticket = pf.submit(residual[sl(0)].contiguous(), embed[sl(0)].contiguous())
        for k in range(nb):
            z = pf.get(ticket).view(B, -1)
            if k + 1 < nb:
                ticket = pf.submit(residual[sl(k + 1)].contiguous(), embed[sl(k + 1)].contiguous())
            seq = gen(x0[sl(k)].contiguous(), z)
            assert torch.equal(z, zs[k]), (trial, k, float((z - zs[k]).abs().max()))
            assert torch.equal(seq, seqs[k]), (trial, k)


def test_hl16_range_guard():
    """A checkpoint whose SPADE (1 + gamma) drives activations past the fp16 range: the split-fp16 path must say so
    (sticky flag -> I2VError at the next call), the exact-fp32 mode must keep working."""
    import i2v_native
    from oracle import decoder_ref
    from stage1_VAE.modules.decoder import Generator
    sd = T(synth.decoder_state_dict(seed=5, channel_factor=8))
    sd["g_2.norm_0.conv_gamma.bias"] = sd["g_2.norm_0.conv_gamma.bias"] * 0 + 3.0e6
    cfg = {"channel_factor": 8, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True}
    x0, z, _ = synth.bench_inputs(2, 64, 64)
    gen = Generator(dict(cfg, mma=1))
    gen.load_state_dict(sd)
    gen = gen.cuda().eval()
    gen(x0.cuda(), z.cuda())                      # enqueues; the flag travels back asynchronously
    assert gen.native().status() & 1              # on-demand check (synchronises)
    with pytest.raises(i2v_native.I2VError, match="fp16 range"):
        gen(x0.cuda(), z.cuda())
    assert gen.native().status(reset=True) & 1 and gen.native().status() == 0
    gen0 = Generator(dict(cfg, mma=0))
    gen0.load_state_dict(sd)
    out0 = gen0.cuda().eval()(x0.cuda(), z.cuda())
    ref = decoder_ref.generator(sd, x0, z)
    assert bool(torch.isfinite(out0).all()) and rel_l2(out0.cpu(), ref) < 1e-3   # (huge activations: looser gate)
    # and an in-range checkpoint never raises the flag
    ok = Generator(dict(cfg, mma=1))
    ok.load_state_dict(T(synth.decoder_state_dict(seed=5, channel_factor=8)))
    ok = ok.cuda().eval()
    ok(x0.cuda(), z.cuda())
    assert ok.native().status() == 0
    # conv_img's fused matrix-core kernel converts g_4's output to fp16 hi / lo in registers: the last producer of split-fp16
    # operands, with its own guard.  A huge conv_1 bias of g_4 reaches no other operand writer (that tensor only feeds conv_img).
    sd2 = T(synth.decoder_state_dict(seed=5, channel_factor=16))
    sd2["g_4.conv_1.bias"] = sd2["g_4.conv_1.bias"] * 0 + 1.0e6
    gi = Generator(dict(cfg, channel_factor=16, mma=1))
    gi.load_state_dict(sd2)
    gi = gi.cuda().eval()
    gi(x0.cuda(), z.cuda())
    assert gi.native().status(reset=True) & 1
    # underflow side (status bit 1, a warning: the next call still runs): ADAIN's gamma / beta of one block scaled by 2^-20 put
    # the whole operand tensor of its conv_1 below the format's absolute error floor
    sd3 = T(synth.decoder_state_dict(seed=5, channel_factor=8))
    for key in ("g_3.norm_1.linear.weight", "g_3.norm_1.linear.bias"):
        sd3[key] = sd3[key] * 2.0 ** -20
    gu = Generator(dict(cfg, mma=1))
    gu.load_state_dict(sd3)
    gu = gu.cuda().eval()
    out_u = gu(x0.cuda(), z.cuda())
    assert gu.native().status() == 2 and bool(torch.isfinite(out_u).all())
    gu(x0.cuda(), z.cuda())                        # not fatal
    assert gu.native().status(reset=True) == 2 and gu.native().status() == 0


def test_mma_auto_falls_back_per_layer_behind_the_range_guard():
    """Round 6 (review item: "nothing automatic stands behind the range guard"): mma = "auto" packs both weight sets; every forward
    synchronises, reads the operand maxima the writers published, switches the 3x3x3 convs whose operand left the window of the
    split-fp16 format to the exact-fp32 kernels (for the life of the handle) and runs the call again.  The checkpoints of
    test_hl16_range_guard must return VALID frames without an exception -- the 3e6 SPADE bias (overflow in g_2.conv_0's operand:
    1e-3 vs the oracle, huge activations), the 2^-20 ADAIN (underflow in g_3.conv_1's operand: 1e-4), the 1e6 bias that only
    conv_img's guard sees (whole-handle fallback) -- and an in-range checkpoint must run exactly the mma = 1 launches (same bits,
    nothing switched).  get_model.Model runs the decoder in this mode by default."""
    from oracle import decoder_ref
    from stage1_VAE.modules.decoder import Generator
    cfg = {"channel_factor": 8, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True}
    x0, z, _ = synth.bench_inputs(2, 64, 64)
    xc, zc = x0.cuda(), z.cuda()

    def make(sd, mma, **kw):
        g = Generator(dict(cfg, mma=mma, **kw))
        g.load_state_dict(sd)
        return g.cuda().eval()

    base = T(synth.decoder_state_dict(seed=5, channel_factor=8))
    ref1 = make(base, 1)(xc, zc)
    ga = make(base, "auto")
    assert ga.mma == 2 and torch.equal(ga(xc, zc), ref1)
    assert ga.native().fallback_layers() == {"layers": [], "whole_handle": False, "reruns": 0} and ga.native().status() == 0
    # overflow in ONE operand tensor
    sd = dict(base)
    sd["g_2.norm_0.conv_gamma.bias"] = sd["g_2.norm_0.conv_gamma.bias"] * 0 + 3.0e6
    g1 = make(sd, "auto")
    out = g1(xc, zc)
    fb = g1.native().fallback_layers()
    ref = decoder_ref.generator(sd, x0, z)
    err = rel_l2(out.cpu(), ref)
    print(f"mma auto, 3e6 SPADE bias: switched {fb}, rel-L2 vs oracle {err:.2e}")
    assert bool(torch.isfinite(out).all()) and err < 1e-3 and "g_2.conv_0" in fb["layers"] and not fb["whole_handle"] and fb["reruns"] >= 1
    assert g1.native().status() == 0
    again = g1(xc, zc)                                   # the decision sticks: no further re-run, same frames
    assert torch.equal(again, out) and g1.native().fallback_layers()["reruns"] == fb["reruns"]
    out0 = make(sd, 0)(xc, zc)
    assert rel_l2(out.cpu(), out0.cpu()) < 1e-3
    # underflow in one operand tensor
    sd3 = dict(base)
    for key in ("g_3.norm_1.linear.weight", "g_3.norm_1.linear.bias"):
        sd3[key] = sd3[key] * 2.0 ** -20
    g3 = make(sd3, "auto")
    out_u = g3(xc, zc)
    fb3 = g3.native().fallback_layers()
    err_u = rel_l2(out_u.cpu(), decoder_ref.generator(sd3, x0, z))
    print(f"mma auto, 2^-20 ADAIN: switched {fb3}, rel-L2 vs oracle {err_u:.2e}")
    assert err_u < TOL and fb3["layers"] == ["g_3.conv_1"] and g3.native().status() == 0
    # an overflow no operand slot explains (only conv_img's guard sees g_4.conv_1's huge bias): the whole handle falls back
    sd2 = T(synth.decoder_state_dict(seed=5, channel_factor=16))
    sd2["g_4.conv_1.bias"] = sd2["g_4.conv_1.bias"] * 0 + 1.0e6
    g2 = make(sd2, "auto", channel_factor=16)
    out2 = g2(xc, zc)
    fb2 = g2.native().fallback_layers()
    assert fb2["whole_handle"] and bool(torch.isfinite(out2).all()) and g2.native().status() == 0
    assert rel_l2(out2.cpu(), make(sd2, 0, channel_factor=16)(xc, zc).cpu()) < 1e-5


def test_handles_are_bound_to_their_device():
    """A native handle serves the GPU its module lives on: a tensor from another device is rejected; with one GPU
    visible the check is exercised through the C ABI's own device test."""
    import i2v_native
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    flow = ConditionalFlow(64, 64, 512, 2, 2, conditioning_option="None")
    flow.load_state_dict(T(synth.flow_state_dict(seed=1, n_flows=2, embedding_dim=64)))
    flow = flow.cuda().eval()
    x, e = torch.randn(3, 64).cuda(), torch.randn(3, 64).cuda()
    z = flow(x, e, reverse=True)
    assert flow.native().device == x.device
    if torch.cuda.device_count() > 1:
        with pytest.raises(i2v_native.I2VError):
            flow(x.to("cuda:1"), e.to("cuda:1"), reverse=True)
        flow1 = flow.to("cuda:1")       # moving the module rebuilds the handle on the new device
        with torch.cuda.device(0):      # current device differs from the tensors': the binding switches for the call
            z1 = flow1(x.to("cuda:1"), e.to("cuda:1"), reverse=True)
        assert z1.device.index == 1 and torch.equal(z1.cpu(), z.cpu())


def test_two_process_rccl_collation(tmp_path):
    """Two ranks over RCCL ("nccl"), one per GPU: sharded synthesis + overlapped all-gather must reproduce the
    one-process result bit for bit.  Needs >= 2 GPUs (the driver's multi-GPU box); skipped on a 1-GPU box."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "tests", "rccl_worker.py")
    port = str(29600 + os.getpid() % 2000)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", str(tmp_path)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def test_bench_multi_gpu_code_paths_on_one_gpu():
    """Round 6: the lines of bench.py that only an N > 1 job reaches -- RCCL group start-up, the collectives around the timing, the rank
    lists, every step's all-gather on the cINN prefetch stream, the N > 1 keys of the line -- on ONE GPU over a one-rank RCCL group
    (I2V_BENCH_FORCE_MULTI=1).  stdout must carry exactly the one JSON line (RCCL's start-up banner goes to stderr); the timed steps are
    checked against a serial reference call by the bench itself."""
    import json
    import subprocess
    import sys
    from conftest import REPO
    port = str(29500 + (os.getpid() * 7) % 2000)
    env = dict(os.environ, I2V_BENCH_FORCE_MULTI="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--batch", "4", "--steps", "3", "--warmup", "1", "--full", "--lean"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:6]
    line = json.loads(lines[0])
    assert line["ranks_seen"] == 1 and line["rccl_version"] and len(line["rank_ms_per_step"]) == 1
    assert line["streams"]["collation_stream"] == "the cINN prefetch stream" and line["steps_check"]["all_bit_identical_to_serial_reference"]


def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """A plain `bench.py` run (no --full): one JSON line with the contract keys and nothing the --full line adds, `steps` timed steps,
    and with --dump-outputs the last timed step's frames, which must be what a serial cINN inverse + decoder call computes on the
    bench's seeded inputs and weights."""
    import json
    import subprocess
    import sys
    from conftest import REPO
    from stage1_VAE.modules.decoder import Generator
    from stage2_cINN.modules.flow_blocks import ConditionalFlow
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--batch", "4", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:6]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    frames = line["config"]["frames_per_step"]
    assert frames == 4 * 16 and abs(line["value"] * line["ms_per_step"] * 1e-3 - frames) < 1e-6 * frames
    assert not {"roofline", "steps_check", "single_call", "cpu_baseline", "sustained"} & set(line)
    seq = np.load(tmp_path / "frames.npy")
    assert seq.dtype == np.float32 and seq.shape == (4, 16, 3, 64, 64)
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    fsd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.flow_state_dict(seed=7, embedding_dim=64).items()}
    dsd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.decoder_state_dict(seed=7, channel_factor=64).items()}
    flow = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
    flow.load_state_dict(fsd)
    gen = Generator({"channel_factor": 64, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True})
    gen.load_state_dict(dsd)
    flow, gen = flow.to(dev).eval(), gen.to(dev).eval()
    x0, residual, embed = synth.bench_inputs(4, 64, 64)
    z = flow(residual.to(dev), embed.to(dev), reverse=True).view(4, -1)
    ref = gen.decode_sequence(x0.to(dev), z, 16).cpu().numpy()
    err = rel_l2(seq, ref)
    assert err < 1e-6, f"dumped frames vs a serial call: rel-L2 {err:.3e}"


def test_smoke_entry():
    import __graft_entry__ as ge
    ge.smoke()
