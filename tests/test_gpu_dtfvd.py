"""DTFVD and the DT-I3D diversity on the GPU: the dynamic-texture variant of the native I3D vs goldens made from the reference's own
``metrics.DTFVD`` modules, the time rule of the input stage, determinism, the metric end to end, the pair-diversity kernel, the
evaluation hook.

Gates: features and embeddings at the project's 1e-4 relative L2 vs the reference's fp32 result; DTFVD and diversity VALUES at the
relative deviation stored in the fixture (``gate.gate_rel`` = 10 x the reference's own fp32-vs-fp64 deviation of that value, measured
when the fixture was made: 2.33e-6 for dtfvd_end2end, 4.80e-6 for dtfvd_diversity; neither is floored)."""
import ctypes

import numpy as np
import pytest
import torch

import dtfvd_common as dc
import i2v_native
import i2v_synth as synth
from conftest import load_golden, rel_l2
from metrics.Diversity import I3D as diversity
from metrics.DTFVD import DTFVD_Score as score
from metrics.DTFVD import ID3, ID3_32

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's parity gate (relative L2 vs the reference goldens)
NC = 18


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


_MODELS = {}


def _model(seed, length=16):
    if (seed, length) not in _MODELS:
        m = (ID3_32 if length == 32 else ID3).InceptionI3D(NC, 1)
        m.load_state_dict(T(dc.dti3d_state_dict(seed, NC)), strict=True)
        _MODELS[(seed, length)] = m.cuda().eval()
    return _MODELS[(seed, length)]


def _clips(c):
    return dc.clips(c["seed"], c["n"] * c.get("r", 1), c["t"], c["h"], c["w"], signed=c["signed"])


def _fixture(name):
    arr, meta = dc.load_fixture(name)
    clips = _clips(meta["clips"])
    if "clips" in arr:
        assert np.allclose(arr["clips"], clips, rtol=0, atol=1e-6)   # the generator is the one the fixture was made with
    return arr, meta, torch.from_numpy(clips).cuda()


I3D_FIXTURES = ["dtfvd_i3d16_t16", "dtfvd_i3d16_t9", "dtfvd_i3d16_t24", "dtfvd_i3d32_t32", "dtfvd_i3d32_t40"]


@pytest.mark.parametrize("name", I3D_FIXTURES)
def test_representation_vs_reference_golden(name):
    arr, meta, clips = _fixture(name)
    model = _model(meta["weights"]["seed"], meta["length"])
    want = arr["features"]
    # the product path: frames as the decoder leaves them, resized by the input stage, values as they are
    got = model.features(clips)
    e1 = rel_l2(got.cpu().numpy(), want)
    # the reference's signature: [B, 3, T, 224, 224]
    x = torch.nn.functional.interpolate(clips.reshape(-1, *clips.shape[2:]), mode="bilinear", size=(224, 224), align_corners=True)
    x = x.reshape(*clips.shape[:2], 3, 224, 224).permute(0, 2, 1, 3, 4)
    rep = model.get_representation(x)
    e2 = rel_l2(rep.cpu().numpy(), want)
    print(f"{name}: rel-L2 features {e1:.3e}, get_representation {e2:.3e}, shape {tuple(got.shape)}")
    assert tuple(got.shape) == want.shape == tuple(meta["endpoints"]["AvgPool_5"]["shape"][:3]) and tuple(rep.shape) == want.shape
    assert e1 <= TOL and e2 <= TOL
    if want.shape[2] == 1:
        assert torch.equal(model.forward_frames(clips), got[:, :, 0])
    else:
        with pytest.raises(ValueError):
            model.forward_frames(clips)
    with pytest.raises(ValueError):
        model.get_representation(x[..., :112, :112])


def test_representation_raw_c_abi():
    arr, meta, clips = _fixture("dtfvd_i3d32_t40")
    lib = i2v_native.lib()
    h = ctypes.c_void_p()
    assert lib.i2v_dti3d_create(NC, 24, ctypes.byref(h)) != 0 and "16 and 32" in i2v_native.lib().i2v_last_error().decode()
    assert lib.i2v_dti3d_create(NC, 32, ctypes.byref(h)) == 0
    try:
        sd = dc.dti3d_state_dict(meta["weights"]["seed"], NC)
        short = {k: v for k, v in sd.items() if k != "Mixed_4d.b2a.bn.running_var"}
        tensors, keep = i2v_native._pack_state_dict(short)
        assert lib.i2v_i3d_load(h, tensors, len(tensors)) == -2, "a missing key is I2V_E_MISSING"
        tensors, keep = i2v_native._pack_state_dict(sd)
        assert lib.i2v_i3d_load(h, tensors, len(tensors)) == 0, lib.i2v_last_error()
        B, Tn, _, H, W = clips.shape
        steps = lib.i2v_i3d_feature_steps(h, Tn)
        nbytes = lib.i2v_i3d_features_workspace_bytes(h, B, Tn, H, W)
        assert steps == 2 and nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(B, 1024, steps, dtype=torch.float32, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.i2v_i3d_features(h, clips.data_ptr(), B, Tn, Tn, H, W, 0, out.data_ptr(), ws.data_ptr(), nbytes - 1, st) != 0   # short workspace
        assert lib.i2v_i3d_features(h, clips.data_ptr(), B, Tn, Tn, H, W, 0, out.data_ptr(), ws.data_ptr(), nbytes, st) == 0, lib.i2v_last_error()
        torch.cuda.synchronize()
        e = rel_l2(out.cpu().numpy(), arr["features"])
        print(f"dtfvd_i3d32_t40 (C ABI): rel-L2 {e:.3e}")
        assert e <= TOL
        # 24 frames leave 3 time steps in front of AvgPool3d((4, 7, 7)): refused, with the message in the style of the Kinetics one
        assert lib.i2v_i3d_feature_steps(h, 24) == 0 and lib.i2v_i3d_features_workspace_bytes(h, B, 24, H, W) == 0
        assert "AvgPool3d((4, 7, 7)); at least 25 frames" in lib.i2v_last_error().decode()
        assert lib.i2v_i3d_feature_steps(h, 25) == 1
    finally:
        lib.i2v_i3d_destroy(h)


def test_time_wrap_and_truncation_vs_reference():
    arr, meta = dc.load_fixture("dtfvd_repeat")
    model = _model(meta["weights"]["seed"], 16)
    for c in meta["cases"]:
        clips = torch.from_numpy(_clips(c)).cuda()
        want = arr[f"rows_t{c['t']}"]
        got = score.get_activations(clips, model, c["n"], cuda=True, t_out=16)
        # the same frames laid out by torch: repeat(1, 3, 1, 1, 1)[:, :16] on the un-resized clip, then the plain path -- bit for bit
        tiled = clips.repeat(1, 3, 1, 1, 1)[:, :16].contiguous()
        assert np.array_equal(got, model.forward_frames(tiled).cpu().numpy().astype(np.float64))
        e = rel_l2(got, want)
        print(f"dtfvd_repeat T_in = {c['t']}: rel-L2 {e:.3e}")
        assert got.shape == want.shape and e <= TOL
        if c["t"] >= 16:
            assert np.array_equal(score.embedding_I3D(model, clips, c["n"], cuda=True), got)
    # no de-normalisation: the denorm switch of the input stage moves the features far beyond the gate
    assert rel_l2(model.forward_frames(clips, True, 16).cpu().numpy(), want) > 100 * TOL


def test_batch_rows_equal_single_sample_runs_bitwise():
    arr, meta, clips = _fixture("dtfvd_i3d16_t16")
    model = _model(meta["weights"]["seed"], 16)
    both = model.features(clips).clone()
    for b in range(clips.shape[0]):
        assert torch.equal(model.features(clips[b:b + 1].contiguous())[0], both[b]), b


def test_two_runs_are_bit_identical_statistics_and_diversity_included():
    _, meta = dc.load_fixture("dtfvd_end2end")
    model = _model(meta["weights"]["seed"], 16)
    clips = torch.from_numpy(dc.clips(31, 8, 16, 32, 32)).cuda()
    runs = []
    for _ in range(2):
        acc = score.DTFVDAccumulator(model)
        f1 = acc.update(clips[:3].contiguous(), "gen").clone()
        f2 = acc.update(clips[3:].contiguous(), "gen").clone()
        st = acc.state("gen")["gen"]
        div = diversity.DiversityAccumulator(model, batch_size=5)
        div.update(clips.reshape(2, 4, *clips.shape[1:]))
        runs.append((f1.cpu(), f2.cpu(), st["sum"], st["gram"], div.state()))
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    f = torch.cat(runs[0][:2]).double().numpy()
    assert f.shape == (8, 1024)
    assert np.allclose(runs[0][2], f.sum(0), rtol=1e-13, atol=1e-13) and np.allclose(runs[0][3], f.T @ f, rtol=1e-13, atol=1e-12)
    s, n = runs[0][4]
    assert n == 2 * 4 * 3 and abs(s / n - dc.pair_diversity(f.reshape(2, 4, 1024))) <= 1e-13 * abs(s / n)


def _end2end():
    arr, meta = dc.load_fixture("dtfvd_end2end")
    model = _model(meta["weights"]["seed"], 16)
    sets = [torch.from_numpy(_clips(m)).cuda() for m in (meta["gen"], meta["orig"])]
    return arr, meta, model, sets


def _route_bound(act_g, act_o):
    """How far two float64 evaluations of the SAME rank-deficient Frechet distance may lie apart (np.cov vs the (n, sum, gram) route):
    with N < D clips every null direction of S1^(1/2) S2 S1^(1/2) carries an eigenvalue error ~ eps * lmax(S1) * lmax(S2), whose square
    root -- sqrt(eps * lmax1 * lmax2), not eps -- enters -2 tr sqrt(.): at most 2 D sqrt(eps * lmax1 * lmax2) in all (the argument of
    tests/test_host_fvd.py::test_frechet_rank_deficient_and_identical_sets)."""
    l1 = np.linalg.eigvalsh(np.cov(act_g, rowvar=False)).max()
    l2 = np.linalg.eigvalsh(np.cov(act_o, rowvar=False)).max()
    return 2 * act_g.shape[1] * np.sqrt(np.finfo(np.float64).eps * l1 * l2)


def _check_value(what, got, meta):
    gate = meta["gate"]["gate_rel"]
    for key in ("fvd_fp32_eigh", "fvd_fp32_sqrtm"):
        dev = abs(got - meta[key]) / abs(meta[key])
        print(f"{what}: got {got!r}, reference {key} {meta[key]!r} (fp64 {meta['fvd_fp64_eigh']!r}), relative deviation {dev:.3e}, allowed {gate:.3e}")
    for key in ("fvd_fp32_eigh", "fvd_fp32_sqrtm"):
        assert abs(got - meta[key]) <= gate * abs(meta[key]), key


def test_end2end_calculate_fvd_vs_reference():
    """Gate (set by the issue): relative deviation from the reference's fp32 value <= 10 x the deviation the reference shows between its own
    fp32 and fp64 runs on the same clips (fixture meta gate.gate_rel = 2.33e-6), against the value of the reference's own sqrtm formulation
    and against the eigh formulation on the reference's fp32 activations."""
    arr, meta, model, (gen, orig) = _end2end()
    act_g = score.get_activations(gen, model, meta["batch_size"], cuda=True, t_out=16)
    act_o = score.get_activations(orig, model, meta["batch_size"], cuda=True, t_out=16)
    eg, eo = rel_l2(act_g, arr["act_gen"]), rel_l2(act_o, arr["act_orig"])
    print(f"end2end activations: rel-L2 gen {eg:.3e}, orig {eo:.3e}")
    got = score.calculate_FVD(model, gen, orig, meta["batch_size"], cuda=True)
    _check_value("end2end DTFVD", got, meta)
    assert eg <= TOL and eo <= TOL


def test_end2end_accumulator_in_uneven_chunks():
    """The streaming form on the same clips in chunks of 5, 8, 1, 10: every clip counts, so with 24 = 3 x 8 clips per set it must give
    calculate_FVD's value up to ``_route_bound`` (float64 gram route vs np.cov), and the same gate as above vs the reference."""
    arr, meta, model, (gen, orig) = _end2end()
    acc = score.DTFVDAccumulator(model)
    for data, which in ((gen, "gen"), (orig, "orig")):
        i = 0
        for n in (5, 8, 1, 10):
            acc.update(data[i:i + n].contiguous(), which)
            i += n
        assert i == data.shape[0]
    got = acc.compute()
    direct = score.calculate_FVD(model, gen, orig, meta["batch_size"], cuda=True)
    bound = _route_bound(arr["act_gen64"], arr["act_orig64"])
    print(f"end2end accumulator: got {got!r}, calculate_FVD {direct!r}, difference {abs(got - direct):.3e}, bound {bound:.3e}")
    _check_value("end2end accumulator", got, meta)
    assert abs(got - direct) <= bound
    acc2 = score.DTFVDAccumulator(model)
    acc2.load_state(acc.state("orig"))
    acc2.update(gen, "gen")
    assert abs(acc2.compute() - got) <= 1e-12 * abs(got)
    # the ragged-batch drop is get_activations' alone
    assert score.get_activations(gen[:11], model, 4, cuda=True, t_out=16).shape == (8, 1024) and acc2.state()["gen"]["n"] == 24


def test_diversity_vs_reference(capsys):
    """compute_DTI3D_diversity and the accumulator in two chunks on [N = 3, R = 4] videos; gate: fixture meta gate.gate_rel = 4.80e-6
    (10 x the reference's fp32-vs-fp64 deviation of the value), embeddings at 1e-4 relative L2."""
    arr, meta = dc.load_fixture("dtfvd_diversity")
    c = meta["clips"]
    model = _model(meta["weights"]["seed"], 16)
    seq1 = torch.from_numpy(_clips(c)).cuda().reshape(c["n"], c["r"], c["t"], 3, c["h"], c["w"])
    want, gate = meta["diversity_fp32"], meta["gate"]["gate_rel"]
    acc = diversity.DiversityAccumulator(model, batch_size=5)
    emb = torch.cat([acc.update(seq1[:1]), acc.update(seq1[1:])])
    e = rel_l2(emb.cpu().numpy(), arr["embed"])
    chunked = acc.compute()
    value = diversity.compute_DTI3D_diversity(seq1, model)
    line = capsys.readouterr().out
    with capsys.disabled():
        print(f"diversity: embeddings rel-L2 {e:.3e}; got {value!r} (two chunks {chunked!r}), reference fp32 {want!r}, fp64 {meta['diversity_fp64']!r}, "
              f"relative deviation {abs(value - want) / want:.3e}, allowed {gate:.3e}")
    assert e <= TOL and emb.shape == arr["embed"].shape
    assert abs(value - want) <= gate * want and abs(chunked - want) <= gate * want
    assert abs(chunked - value) <= 1e-13 * value and acc.state()[1] == c["n"] * c["r"] * (c["r"] - 1)
    assert line.strip() == f"Diversity score of {value * 1000} using I3D backbone pretrained on dynamic textures"
    # the kernel alone on the reference's embeddings: float64 sums of fp32 inputs, 1e-13
    ref_emb = torch.from_numpy(arr["embed"]).cuda()
    a = torch.zeros(2, dtype=torch.float64, device="cuda")
    i2v_native.diversity_update(ref_emb, a)
    assert abs(float(a[0] / a[1]) - want) <= 1e-13 * want
    # the [N, R] ordering: swapping the two axes is another number
    i2v_native.diversity_update(ref_emb.transpose(0, 1).contiguous(), a.zero_())
    assert abs(float(a[0] / a[1]) - want) > 100 * gate * want


def test_evaluate_fvd_prior_dtfvd_vs_sample_prior_by_hand():
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
    model = _model(41, 16)
    g = torch.Generator().manual_seed(17)
    loader = [{"seq": 2 * torch.rand(b, 17, 3, 64, 64, generator=g) - 1} for b in (4, 3, 2)]
    torch.manual_seed(5)
    value = aux.evaluate_FVD_prior(loader, st, gen, model, 64, None, 0, "DTFVD", False)
    torch.manual_seed(5)
    seq_gen, seq_orig = aux.sample_prior(loader, st, gen, 64)
    by_hand = score.calculate_FVD(model, seq_gen.cuda(), seq_orig.cuda(), 9, cuda=True)
    bound = _route_bound(score.get_activations(seq_gen, model, 9, cuda=True, t_out=16), score.get_activations(seq_orig, model, 9, cuda=True, t_out=16))
    print(f"evaluate_FVD_prior (DTFVD) {value!r}, by hand {by_hand!r}, difference {abs(value - by_hand):.3e}, bound {bound:.3e}")
    # the same features (batch rows do not depend on the batch); float64 gram route vs np.cov on rank-8 covariances of 1024 features
    assert np.isfinite(value) and value >= 0 and abs(value - by_hand) <= bound and bound < 1e-3 * abs(by_hand)
    with pytest.raises(NotImplementedError, match="DTFVD"):
        aux.evaluate_FVD_prior(loader, st, gen, model, 64, None, 0, "FVD+", False)
