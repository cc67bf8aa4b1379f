"""Several realizations per start frame (i2v_dec_forward_realizations, Generator.forward(..., realizations=K), Model.sample): sample
f*K + k decodes frame f with latent row f*K + k, and the frames must be the bits of the repeated path -- the start frames
repeat_interleave'd K times through i2v_dec_forward_strided -- in every matrix-core mode and under every structure switch, while
the SPADE branches run once per frame (batch F) and every SPADE-consuming operand writer reads map row sample / K."""
import os

import numpy as np
import pytest
import torch

import i2v_synth as synth
from conftest import load_golden

pytestmark = pytest.mark.gpu

MODES = [0, 1, "fp16", "auto"]


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import i2v_native
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()
    torch.set_grad_enabled(False)


def _gen(meta, mma, sd=None):
    from stage1_VAE.modules.decoder import Generator
    gen = Generator({"channel_factor": meta["synth"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"],
                     "upsample_t": meta["upsample_t"], "spectral_norm": True, "mma": mma})
    gen.load_state_dict(sd if sd is not None else T(synth.decoder_state_dict(**meta["synth"])))
    return gen.cuda().eval()


def _inputs(F, K, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(F, 3, size, size, generator=g) * 2 - 1).cuda()
    z = torch.randn(F * K, 64, generator=g).cuda()
    return img, z


def _img_size(name):
    return 64 if name == "dec_nf64_bair" else 128


# ------------------------------------------------------------------------------------------------ Generator.forward
@pytest.mark.parametrize("name", ["dec_nf64_bair", "dec_nf32_128", "dec_nf8_128"])
@pytest.mark.parametrize("mma", MODES)
def test_forward_realizations_equal_repeated_frames(name, mma):
    _, meta = load_golden(name)
    gen = _gen(meta, mma)
    size = _img_size(name)
    for F, K in ((2, 1), (2, 2), (3, 3), (1, 4)):
        img, z = _inputs(F, K, size, seed=F * 10 + K)
        ref = gen(img.repeat_interleave(K, 0), z).clone()
        out = gen(img, z, realizations=K)
        assert out.shape == ref.shape and torch.equal(out, ref), (name, mma, F, K)
        # with a matching prepare (forked onto the side stream, consumed per level)
        gen.prepare(img, realizations=K)
        assert torch.equal(gen(img, z, realizations=K), ref), (name, mma, F, K, "prepared")
    if mma == "auto":
        assert gen.native().fallback_layers()["reruns"] == 0   # in range: the mma = 1 launches


@pytest.mark.parametrize("env,val,name", [("I2V_DEC_OVERLAP", "0", "dec_nf64_bair"), ("I2V_DEC_OVERLAP", "2", "dec_nf32_128"),
                                          ("I2V_DEC_SUB", "2", "dec_nf32_128"), ("I2V_DEC_SUB", "5", "dec_nf8_128"),
                                          ("I2V_DEC_GEN", "1", "dec_nf32_128")])
@pytest.mark.parametrize("mma", [1, "fp16"])
def test_forward_realizations_under_structure_switches(env, val, name, mma, monkeypatch):
    """Sub-batches that are not a multiple of K (the launch's first sample sits inside a frame's realizations), the in-call overlap
    off / half on, and the operand-generating F(4,3) kernel (I2V_DEC_GEN=1: its SPADE form reads the shared maps in-kernel)."""
    monkeypatch.setenv(env, val)
    _, meta = load_golden(name)
    gen = _gen(meta, mma)
    size = _img_size(name)
    if env == "I2V_DEC_GEN" and mma == 1:
        h = gen.native()
        h.set_profile(True)
        img, z = _inputs(2, 3, size)
        gen(img, z, realizations=3)
        torch.cuda.synchronize()
        kernels = {r["layer"]: r["kernel"] for r in h.get_layer_profile()}
        h.set_profile(False)
        assert kernels["g_4.conv_0"] == "conv_wino4g_f16x3", kernels
    for F, K in ((3, 3), (2, 4), (5, 2)):
        img, z = _inputs(F, K, size, seed=F + K)
        ref = gen(img.repeat_interleave(K, 0), z).clone()
        assert torch.equal(gen(img, z, realizations=K), ref), (env, val, name, mma, F, K)
        gen.prepare(img, realizations=K)
        assert torch.equal(gen(img, z, realizations=K), ref), (env, val, name, mma, F, K, "prepared")


def test_prepare_matches_only_the_same_realizations():
    """A prepare for (F, K) is dropped by a forward with another K (or the plain forward): the maps are recomputed inline."""
    _, meta = load_golden("dec_nf64_bair")
    gen = _gen(meta, 1)
    img, z4 = _inputs(2, 4, 64)
    ref4 = gen(img.repeat_interleave(4, 0), z4).clone()
    ref1 = gen(img, z4[:2]).clone()
    gen.prepare(img, realizations=2)
    assert torch.equal(gen(img, z4, realizations=4), ref4)
    gen.prepare(img, realizations=4)
    assert torch.equal(gen(img, z4[:2]), ref1)
    gen.prepare(img)
    assert torch.equal(gen(img, z4, realizations=4), ref4)


def test_decode_sequence_realizations():
    _, meta = load_golden("dec_nf64_bair")
    gen = _gen(meta, 1)
    img, z = _inputs(2, 3, 64)
    ref = gen.decode_sequence(img.repeat_interleave(3, 0), z, 40)
    out = gen.decode_sequence(img, z, 40, realizations=3)
    assert out.shape == (6, 48, 3, 64, 64) and torch.equal(out, ref)


def test_auto_out_of_range_falls_back_on_the_shared_path():
    """mma = auto with a checkpoint outside the split window (the 3e6 SPADE bias of the range-guard tests): the re-run after the
    per-layer switch goes through the shared path again and still equals the repeated path."""
    cfg = {"channel_factor": 8, "z_dim": 64, "upsample_s": [2, 1], "upsample_t": [2, 1], "spectral_norm": True}
    sd = T(synth.decoder_state_dict(seed=5, channel_factor=8))
    sd["g_2.norm_0.conv_gamma.bias"] = sd["g_2.norm_0.conv_gamma.bias"] * 0 + 3.0e6
    from stage1_VAE.modules.decoder import Generator

    def make():
        g = Generator(dict(cfg, mma="auto"))
        g.load_state_dict(sd)
        return g.cuda().eval()
    img, z = _inputs(2, 3, 64)
    g_rep, g_sh = make(), make()
    ref = g_rep(img.repeat_interleave(3, 0), z)
    out = g_sh(img, z, realizations=3)
    fb_rep, fb_sh = g_rep.native().fallback_layers(), g_sh.native().fallback_layers()
    assert "g_2.conv_0" in fb_sh["layers"] and fb_sh["reruns"] >= 1
    assert fb_sh["layers"] == fb_rep["layers"] and fb_sh["whole_handle"] == fb_rep["whole_handle"]
    assert bool(torch.isfinite(out).all()) and torch.equal(out, ref)
    assert g_sh.native().status() == g_rep.native().status() == 0


@pytest.mark.parametrize("mma", [1, "fp16"])
def test_graph_capture_replays_realizations(mma):
    _, meta = load_golden("dec_nf64_bair")
    gen = _gen(meta, mma)
    img, z = _inputs(3, 2, 64)
    eager = gen(img, z, realizations=2).clone()
    gen.native()   # (built before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = gen(img, z, realizations=2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


@pytest.mark.parametrize("mma", [0, 1])
def test_workspace_is_smaller_and_sufficient(mma):
    import i2v_native
    _, meta = load_golden("dec_nf32_128")
    gen = _gen(meta, mma)
    h = gen.native()
    F, K = 2, 3
    lib = i2v_native.lib()
    shared, repeated = h.workspace_bytes(F, 128, 128, K), int(lib.i2v_dec_workspace_bytes(h._h, F * K, 128, 128))
    assert h.workspace_bytes(F, 128, 128, 1) == int(lib.i2v_dec_workspace_bytes(h._h, F, 128, 128))
    for k in (2, 4, 8):
        assert h.workspace_bytes(F, 128, 128, k) < int(lib.i2v_dec_workspace_bytes(h._h, F * k, 128, 128))
    print(f"workspace F = {F}, K = {K}: shared {shared / 2**20:.1f} MiB, repeated {repeated / 2**20:.1f} MiB")
    img, z = _inputs(F, K, 128)
    ref = gen(img.repeat_interleave(K, 0), z).clone()
    ws = torch.full((shared // 4,), float("nan"), dtype=torch.float32, device="cuda")
    T_, H, W = h.out_shape
    out = torch.empty(F * K, T_, 3, H, W, device="cuda")
    i2v_native._check(lib.i2v_dec_forward_realizations(h._h, img.data_ptr(), 128, 128, 0, F, K, z.data_ptr(), out.data_ptr(), 0,
                                                       ws.data_ptr(), shared, torch.cuda.current_stream().cuda_stream), "forward")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and torch.equal(out, ref)
    rc = lib.i2v_dec_forward_realizations(h._h, img.data_ptr(), 128, 128, 0, F, K, z.data_ptr(), out.data_ptr(), 0, ws.data_ptr(),
                                          shared - 4, torch.cuda.current_stream().cuda_stream)
    assert rc != 0   # one byte short: I2V_E_WORKSPACE


def test_debug_tap0_returns_the_frame_maps():
    _, meta = load_golden("dec_nf64_bair")
    gen = _gen(meta, 1)
    h = gen.native()
    F, K = 3, 2
    img, z = _inputs(F, K, 64)
    nf = gen.channel_factor
    for block in (4, 5):
        C = {4: 4, 5: 2}[block] * nf
        size = F * K * 64 * 64 * 2 * C   # at least the block's maps (its level is at most 64 x 64)
        rep = torch.full((size,), float("nan"), device="cuda")
        h.debug_tap(block, 0, rep)
        gen(img.repeat_interleave(K, 0), z)
        sh = torch.full((size,), float("nan"), device="cuda")
        h.debug_tap(block, 0, sh)
        gen(img, z, realizations=K)
        h.debug_tap(0, 0, None)
        torch.cuda.synchronize()
        n_rep = int(torch.isfinite(rep).sum())
        per = n_rep // (F * K)
        assert n_rep == F * K * per and bool(torch.isfinite(rep[:n_rep]).all())
        assert int(torch.isfinite(sh).sum()) == F * per   # F maps, nothing behind them
        assert torch.equal(sh[:F * per].view(F, per), rep[:n_rep].view(F, K, per)[:, 0])


# ------------------------------------------------------------------------------------------------ Model.sample
def _model(tmp_path, vid_length, control=False, with_embedder=False, mma=None):
    import yaml
    from get_model import Model
    from test_gpu_parity import _write_checkpoints
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta, with_embedder=with_embedder)
    if control:
        cfg = yaml.safe_load(open(ckpt + "config_stage2.yaml"))
        cfg["Training"]["control"] = True
        open(ckpt + "config_stage2.yaml", "w").write(yaml.safe_dump(cfg))
        torch.save({"state_dict": T(synth.flow_state_dict(seed=7, n_flows=20, embedding_dim=94, control=True))}, ckpt + "cINN.pth")
    return Model(ckpt, vid_length, mma=mma)


@pytest.mark.parametrize("vid_length", [16, 32])
def test_model_sample_equals_repeated_synthesize(tmp_path, vid_length):
    model = _model(tmp_path, vid_length)
    F, n = 3, 3
    x0, _, embed = synth.bench_inputs(F, 64, 64)
    residual = torch.randn(F * n, 64, generator=torch.Generator().manual_seed(4))
    ref = model.synthesize(x0.cuda().repeat_interleave(n, 0), residual=residual.cuda(), embed=embed.cuda().repeat_interleave(n, 0))
    out = model.sample(x0.cuda(), n, residual=residual.cuda(), embed=embed.cuda())
    assert out.shape == (F, n, vid_length, 3, 64, 64)
    assert torch.equal(out.reshape(F * n, *out.shape[2:]), ref)
    assert torch.equal(model.sample(x0.cuda(), n, residual=residual.view(F, n, 64).cuda(), embed=embed.cuda()), out)
    model.overlap = False
    assert torch.equal(model.sample(x0.cuda(), n, residual=residual.cuda(), embed=embed.cuda()), out)
    model.check()


def test_model_sample_n1_is_synthesize(tmp_path):
    model = _model(tmp_path, 16)
    x0, _, embed = synth.bench_inputs(2, 64, 64)
    torch.manual_seed(11)
    a = model.sample(x0.cuda(), 1, embed=embed.cuda())
    torch.manual_seed(11)
    b = model.synthesize(x0.cuda(), embed=embed.cuda())
    assert torch.equal(a, b.unsqueeze(1))


def test_model_sample_control(tmp_path):
    model = _model(tmp_path, 16, control=True)
    F, n = 2, 4
    x0, _, embed = synth.bench_inputs(F, 64, 64)
    pos = torch.tensor([[0.05, 0.5, 1.0], [0.31, 0.999, 0.1001]])
    residual = torch.randn(F * n, 64, generator=torch.Generator().manual_seed(2)).cuda()
    ref = model.synthesize(x0.cuda().repeat_interleave(n, 0), cond=pos.repeat_interleave(n, 0), residual=residual,
                           embed=embed.cuda().repeat_interleave(n, 0))
    out = model.sample(x0.cuda(), n, cond=pos, residual=residual, embed=embed.cuda())
    assert torch.equal(out.reshape(F * n, *out.shape[2:]), ref)


def test_model_sample_from_pixels_embeds_once_per_frame(tmp_path):
    model = _model(tmp_path, 16, with_embedder=True)
    emb = model.flow.embedder
    seen = []
    orig = emb.encode

    def encode(x):
        seen.append(x.shape[0])
        return orig(x)
    emb.encode = encode
    F, n = 2, 3
    x0, _, _ = synth.bench_inputs(F, 64, 64)
    residual = torch.randn(F * n, 64, generator=torch.Generator().manual_seed(5)).cuda()
    out = model.sample(x0.cuda(), n, residual=residual)
    assert seen == [F]
    e = orig(x0.cuda()).mode().reshape(F, -1)
    ref = model.synthesize(x0.cuda().repeat_interleave(n, 0), residual=residual, embed=e.repeat_interleave(n, 0))
    assert torch.equal(out.reshape(F * n, *out.shape[2:]), ref)


# ------------------------------------------------------------------------------------------------ CLIs
def _images(d, n, size=64, seed=1):
    from PIL import Image
    d.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (size, size, 3), dtype=np.uint8)).save(d / f"{i:02d}.png")


def test_generate_samples_n_realiz(tmp_path):
    import generate_samples
    from test_gpu_parity import _write_checkpoints
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta)
    _images(tmp_path / "imgs", 3)
    gpu = os.environ.get("HIP_VISIBLE_DEVICES", "0")
    base = ["-gpu", gpu, "-dataset", "bair", "-ckpt_path", ckpt, "-seq_length", "16", "-bs", "2", "-embed_seed", "3", "-seed", "9",
            "-img_path", str(tmp_path / "imgs") + "/"]
    os.environ["HIP_VISIBLE_DEVICES"] = gpu
    generate_samples.main(base + ["-out_path", str(tmp_path / "a") + "/", "-raw_npy", str(tmp_path / "a.npy")])
    generate_samples.main(base + ["-out_path", str(tmp_path / "b") + "/", "-raw_npy", str(tmp_path / "b.npy"), "-n_realiz", "1"])
    assert (tmp_path / "a" / "results.gif").read_bytes() == (tmp_path / "b" / "results.gif").read_bytes()
    assert np.array_equal(np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy"))
    generate_samples.main(base + ["-out_path", str(tmp_path / "c") + "/", "-raw_npy", str(tmp_path / "c.npy"), "-n_realiz", "2"])
    grid = np.load(tmp_path / "c.npy")
    assert grid.shape == (16, 2 * 64, 3 * 64, 3)
    # the rows against the repeated path: the same residual draws (realization fastest) through synthesize
    from get_model import Model
    from utils import auxiliaries as aux
    import generate_samples as gs
    model = Model(ckpt, 16)
    imgs = gs.load_images(sorted(str(p) for p in (tmp_path / "imgs").glob("*.png")), 64)
    E = 64
    embeds = torch.randn(3, E, generator=torch.Generator().manual_seed(3))
    torch.manual_seed(9)
    vids = []
    for i in range(0, 3, 2):
        b = imgs[i:i + 2]
        res = torch.randn(b.size(0) * 2, 64).cuda()
        vids.append(model.synthesize(b.cuda().repeat_interleave(2, 0), residual=res,
                                     embed=embeds[i:i + 2].cuda().repeat_interleave(2, 0)).view(b.size(0), 2, 16, 3, 64, 64).cpu())
    v = torch.cat(vids)
    assert np.array_equal(grid, aux.convert_grid2gif(v).astype(np.uint8))


def test_visualize_endpoint_cli(tmp_path):
    import yaml
    from PIL import Image
    import visualize_endpoint
    from test_gpu_parity import _write_checkpoints
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta)
    cfg = yaml.safe_load(open(ckpt + "config_stage2.yaml"))
    cfg["Training"]["control"] = True
    open(ckpt + "config_stage2.yaml", "w").write(yaml.safe_dump(cfg))
    torch.save({"state_dict": T(synth.flow_state_dict(seed=7, n_flows=20, embedding_dim=94, control=True))}, ckpt + "cINN.pth")
    _images(tmp_path / "imgs", 4)
    np.save(tmp_path / "cond.npy", np.random.default_rng(0).uniform(0.01, 0.99, (4, 3)).astype(np.float32))
    out = tmp_path / "out"
    visualize_endpoint.main(["-gpu", os.environ.get("HIP_VISIBLE_DEVICES", "0"), "-ckpt_path", ckpt, "-img_path", str(tmp_path / "imgs") + "/",
                             "-cond_npy", str(tmp_path / "cond.npy"), "-n_samples", "3", "-n_realiz", "3", "-bs", "2", "-seq_length", "16",
                             "-embed_seed", "1", "-seed", "4", "-out_path", str(out) + "/"])
    for i in range(3):
        gif = Image.open(out / f"endpoint_{i}.gif")
        assert gif.n_frames == 16 and gif.size == (3 * 64, 64)
        png = Image.open(out / f"endpoint_{i}.png")
        assert png.size == (3 * 64 + 4 * 2, 64 + 2 * 2)   # one row of 3 tiles, padding 2 (save_image's grid)
    assert not (out / "endpoint_3.gif").exists()
