"""FVD on the GPU: the native I3D vs goldens made from the reference's own module, the input stage vs torch's bilinear resize,
determinism, the end-to-end metric vs the reference's value, the evaluation hook, graph capture."""
import ctypes

import numpy as np
import pytest
import torch

import fvd_common as fc
import i2v_native
import i2v_synth as synth
from conftest import load_golden, rel_l2
from metrics.PyTorch_FVD import FVD_logging as fvd
from metrics.PyTorch_FVD.I3D import I3D

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's parity gate (relative L2 vs the reference goldens)


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


_MODELS = {}


def _model(seed, num_classes):
    if (seed, num_classes) not in _MODELS:
        m = I3D(num_classes)
        m.load_state_dict(T(fc.i3d_state_dict(seed, num_classes)))
        _MODELS[(seed, num_classes)] = m.cuda().eval()
    return _MODELS[(seed, num_classes)]


def _fixture(name):
    arr, meta = fc.load_fixture(name)
    c = meta["clips"]
    clips = fc.clips(c["seed"], c["n"], c["t"], c["h"], c["w"], signed=c["signed"])
    if "clips" in arr:
        assert np.allclose(arr["clips"], clips, rtol=0, atol=1e-6)   # the generator is the one the fixture was made with (libm may differ by an ulp)
    return arr, meta, torch.from_numpy(clips).cuda()


@pytest.mark.parametrize("name", ["fvd_i3d_t16", "fvd_i3d_t9", "fvd_i3d_128"])
def test_i3d_logits_vs_reference_golden(name):
    arr, meta, clips = _fixture(name)
    model = _model(meta["weights"]["seed"], meta["weights"]["num_classes"])
    # the product path: frames in the decoder's layout and range, resize + denorm in the input stage
    got = model.forward_frames(clips, True)
    e1 = rel_l2(got.cpu().numpy(), arr["logits"])
    # the reference's signature: [B, 3, T, H, W], values as they are (de-normalised by the caller)
    soft, logits = model(((clips + 1.0) / 2.0).permute(0, 2, 1, 3, 4))
    e2 = rel_l2(logits.cpu().numpy(), arr["logits"])
    print(f"{name}: rel-L2 forward_frames {e1:.3e}, forward {e2:.3e}")
    assert got.shape == arr["logits"].shape
    assert e1 <= TOL and e2 <= TOL
    assert torch.allclose(soft.sum(1), torch.ones_like(soft[:, 0]), atol=1e-5)


@pytest.mark.parametrize("name", ["fvd_i3d_t16", "fvd_i3d_t9", "fvd_i3d_128"])
def test_i3d_logits_raw_c_abi(name):
    arr, meta, clips = _fixture(name)
    nc = meta["weights"]["num_classes"]
    lib = i2v_native.lib()
    h = ctypes.c_void_p()
    assert lib.i2v_i3d_create(nc, 3, ctypes.byref(h)) == 0
    try:
        tensors, keep = i2v_native._pack_state_dict(fc.i3d_state_dict(meta["weights"]["seed"], nc))
        assert lib.i2v_i3d_load(h, tensors, len(tensors)) == 0, lib.i2v_last_error()
        B, Tn, _, H, W = clips.shape
        nbytes = lib.i2v_i3d_workspace_bytes(h, B, Tn, H, W)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(B, nc, dtype=torch.float32, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.i2v_i3d_forward(h, clips.data_ptr(), B, Tn, H, W, 1, out.data_ptr(), ws.data_ptr(), nbytes - 1, st) != 0   # short workspace
        assert lib.i2v_i3d_forward(h, clips.data_ptr(), B, Tn, H, W, 1, out.data_ptr(), ws.data_ptr(), nbytes, st) == 0, lib.i2v_last_error()
        torch.cuda.synchronize()
        e = rel_l2(out.cpu().numpy(), arr["logits"])
        print(f"{name} (C ABI): rel-L2 {e:.3e}")
        assert e <= TOL
        assert lib.i2v_i3d_workspace_bytes(h, B, 8, H, W) == 0   # 8 frames leave one time step in front of AvgPool3d((2, 7, 7))
    finally:
        lib.i2v_i3d_destroy(h)


@pytest.mark.parametrize("size,denorm", [((32, 32), True), ((64, 48), False), ((224, 224), True), ((300, 256), False)])
def test_input_stage_vs_torch_interpolate(size, denorm):
    """Bound: both sides evaluate h0 (w0 a + w1 b) + h1 (w0 c + w1 d) in fp32 with the same weights; they differ in fused vs separate
    multiply-adds -- at most 6 roundings of values <= 1 in magnitude, 6 * 2^-24 = 3.6e-7, (then halved by the denorm); gate 1e-6 absolute."""
    g = torch.Generator().manual_seed(size[0])
    x = 2 * torch.rand(5, 3, *size, generator=g) - 1
    ref = torch.nn.functional.interpolate(x, mode="bilinear", size=(224, 224), align_corners=True)
    if denorm:
        ref = (ref + 1.0) / 2.0
    got = i2v_native.i3d_input_stage(x.cuda(), denorm).cpu()
    err = float((got[..., :3].permute(0, 3, 1, 2) - ref).abs().max())
    print(f"input stage {size} denorm={denorm}: max-abs {err:.3e}")
    assert err <= 1e-6 and float(got[..., 3].abs().max()) == 0.0
    if size == (224, 224):
        assert err <= 6e-8   # identity resize: only the denorm's rounding can differ


def test_batch_rows_equal_single_sample_runs_bitwise():
    arr, meta, clips = _fixture("fvd_i3d_t16")
    model = _model(meta["weights"]["seed"], meta["weights"]["num_classes"])
    both = model.forward_frames(clips, True).clone()
    for b in range(clips.shape[0]):
        assert torch.equal(model.forward_frames(clips[b:b + 1].contiguous(), True)[0], both[b]), b


def test_two_runs_are_bit_identical_statistics_included():
    _, meta = fc.load_fixture("fvd_end2end")
    model = _model(meta["weights"]["seed"], 16)
    clips = torch.from_numpy(fc.clips(31, 7, 16, 32, 32)).cuda()
    runs = []
    for _ in range(2):
        acc = fvd.FVDAccumulator(model)
        f1 = acc.update(clips[:4].contiguous(), "gen").clone()
        f2 = acc.update(clips[4:].contiguous(), "gen").clone()
        st = acc.state("gen")["gen"]
        runs.append((f1.cpu(), f2.cpu(), st["sum"], st["gram"]))
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # and the statistics are the float64 sums of the features
    f = torch.cat(runs[0][:2]).double().numpy()
    assert np.allclose(runs[0][2], f.sum(0), rtol=1e-13, atol=1e-13) and np.allclose(runs[0][3], f.T @ f, rtol=1e-13, atol=1e-12)


def _end2end():
    arr, meta = fc.load_fixture("fvd_end2end")
    model = _model(meta["weights"]["seed"], 16)
    sets = [torch.from_numpy(fc.clips(m["seed"], m["n"], m["t"], m["h"], m["w"], signed=m["signed"])).cuda() for m in (meta["gen"], meta["orig"])]
    return arr, meta, model, sets


def test_end2end_calculate_fvd_vs_reference():
    """Gate (set by the issue): relative deviation from the reference's fp32 value <= 10 x the deviation the reference shows between its own
    fp32 and fp64 runs on the same clips (fixture meta ref_fp32_vs_fp64_rel)."""
    arr, meta, model, (gen, orig) = _end2end()
    act_g = fvd.get_activations(gen, model, meta["batch_size"], cuda=True)
    act_o = fvd.get_activations(orig, model, meta["batch_size"], cuda=True)
    print(f"end2end activations: rel-L2 gen {rel_l2(act_g, arr['act_gen']):.3e}, orig {rel_l2(act_o, arr['act_orig']):.3e}")
    got = fvd.calculate_FVD(model, gen, orig, meta["batch_size"], cuda=True)
    dev = abs(got - meta["fvd_fp32"]) / abs(meta["fvd_fp32"])
    print(f"end2end FVD: got {got!r}, reference fp32 {meta['fvd_fp32']!r}, fp64 {meta['fvd_fp64']!r}, relative deviation {dev:.3e}, "
          f"allowed {10 * meta['ref_fp32_vs_fp64_rel']:.3e}")
    assert rel_l2(act_g, arr["act_gen"]) <= TOL and rel_l2(act_o, arr["act_orig"]) <= TOL
    assert dev <= 10 * meta["ref_fp32_vs_fp64_rel"]


def test_end2end_accumulator_in_uneven_chunks():
    """The streaming form on the same clips, fed in chunks of 5, 16, 1, 26: every clip counts, so with 48 = 3 x 16 clips per set it must give
    calculate_FVD's value; same gate as above vs the reference, and 1e-9 relative vs calculate_FVD (float64 gram route vs np.cov)."""
    arr, meta, model, (gen, orig) = _end2end()
    acc = fvd.FVDAccumulator(model)
    for data, which, signed in ((gen, "gen", True), (orig, "orig", False)):
        i = 0
        for n in (5, 16, 1, 26):
            acc.update(data[i:i + n].contiguous(), which, denorm_input=signed)
            i += n
        assert i == data.shape[0]
    got = acc.compute()
    direct = fvd.calculate_FVD(model, gen, orig, meta["batch_size"], cuda=True)
    dev = abs(got - meta["fvd_fp32"]) / abs(meta["fvd_fp32"])
    print(f"end2end accumulator: got {got!r}, calculate_FVD {direct!r}, relative deviation vs reference {dev:.3e}")
    assert abs(got - direct) <= 1e-9 * abs(direct)
    assert dev <= 10 * meta["ref_fp32_vs_fp64_rel"]
    # the real set's statistics carried over to a fresh accumulator
    acc2 = fvd.FVDAccumulator(model)
    acc2.load_state(acc.state("orig"))
    acc2.update(gen, "gen")
    assert abs(acc2.compute() - got) <= 1e-12 * abs(got)


def test_ragged_last_batch_is_dropped_by_get_activations_only():
    _, meta, model, (gen, _) = _end2end()
    a = fvd.get_activations(gen[:11], model, 4, cuda=True)
    assert a.shape == (8, 16)
    acc = fvd.FVDAccumulator(model)
    acc.update(gen[:11].contiguous(), "gen")
    assert acc.state()["gen"]["n"] == 11


def test_evaluate_fvd_prior_vs_sample_prior_by_hand():
    from stage2_cINN.modules.INN import SupervisedTransformer
    from stage1_VAE.modules.decoder import Generator
    from utils import auxiliaries as aux
    _, meta = load_golden("model_nf8")
    gen = Generator({"channel_factor": meta["synth_dec"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"],
                     "upsample_t": meta["upsample_t"], "spectral_norm": True})
    gen.load_state_dict(T(synth.decoder_state_dict(**meta["synth_dec"])))
    gen = gen.cuda().eval()

    class PooledEmbedder:   # test scaffolding: a deterministic stand-in for the conditioning embedder (encode(x).mode())
        def encode(self, x):
            e = torch.nn.functional.adaptive_avg_pool2d(x, (4, 4)).reshape(x.size(0), -1)[:, :32]
            e = torch.cat((e, -e), dim=1)[:, :, None, None]
            return type("D", (), {"mode": lambda self_, e=e: e})()

    st = SupervisedTransformer(flow_in_channels=64, flow_mid_channels=512, flow_hidden_depth=2, n_flows=20, flow_conditioning_option="None",
                               flow_embedding_channels=64, control=False, dic=None, embedder=PooledEmbedder())
    st.flow.load_state_dict(T(synth.flow_state_dict(**meta["synth_flow"])))
    st = st.cuda().eval()
    model = _model(41, 4)   # 4 features: the 9 clips of the loader give full-rank covariances
    g = torch.Generator().manual_seed(17)
    loader = [{"seq": 2 * torch.rand(b, 17, 3, 64, 64, generator=g) - 1} for b in (4, 3, 2)]
    torch.manual_seed(5)
    value = aux.evaluate_FVD_prior(loader, st, gen, model, 64, None, 0, "FVD", False)
    torch.manual_seed(5)
    seq_gen, seq_orig = aux.sample_prior(loader, st, gen, 64)
    by_hand = fvd.calculate_FVD(model, seq_gen.cuda(), seq_orig.cuda(), 9, cuda=True)
    print(f"evaluate_FVD_prior {value!r}, by hand {by_hand!r}")
    # the same features (batch rows do not depend on the batch); float64 gram route vs np.cov
    assert np.isfinite(value) and value >= 0 and abs(value - by_hand) <= 1e-9 * abs(by_hand)
    with pytest.raises(NotImplementedError, match="DTFVD"):
        aux.evaluate_FVD_prior(loader, st, gen, model, 64, None, 0, "DTFVD", False)


def test_graph_capture_replays_to_the_same_bits():
    arr, meta, clips = _fixture("fvd_i3d_t9")
    model = _model(meta["weights"]["seed"], meta["weights"]["num_classes"])
    eager = model.forward_frames(clips, True).clone()
    static_in = clips.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.forward_frames(static_in, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = model.forward_frames(static_in, True)
    for _ in range(2):
        static_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager)
    static_in.copy_(-clips)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, model.forward_frames((-clips).contiguous(), True))
