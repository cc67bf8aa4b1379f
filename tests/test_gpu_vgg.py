"""GPU checks of the native VGG-16 trunk (csrc/i2v_vgg.hip) and the reductions on its taps (csrc/i2v_lpips.hip): one convolution against the float64 oracle at the element-wise dot-product
bound over ragged tiles, batches and chunk counts; the max pool bit for bit; the input stage; the five taps, LPIPS and the diversity
score against the fixtures written from the reference's own modules (tests/golden/make_golden_vgg.py); repeatability and graph capture."""
import numpy as np
import pytest
import torch

import i2v_native
import vgg_common as vc
from metrics.Diversity.VGG import compute_vgg_diversity
from stage2_cINN.AE.modules.LPIPS import LPIPS, lpips_score
from stage2_cINN.AE.modules.vgg16 import vgg16

pytestmark = pytest.mark.gpu
DEV = "cuda"


def holder(seed, lin_seed=None):
    """vgg16 / LPIPS filled from the synthesiser (no file involved)."""
    own = {k: torch.from_numpy(v) for k, v in zip(vc.holder_keys(), vc.vgg_state_dict(seed).values())}
    if lin_seed is None:
        m = vgg16(pretrained=False)
        m.load_state_dict(own, strict=True)
    else:
        m = LPIPS()
        sd = {"net." + k: v for k, v in own.items()}
        sd.update({k: torch.from_numpy(v) for k, v in vc.lin_state_dict(lin_seed).items()})
        m.load_state_dict(sd, strict=False)
    return m.to(DEV).eval()


_MODELS = {}


def model(kind, seed, lin_seed=None):
    key = (kind, seed, lin_seed)
    if key not in _MODELS:
        _MODELS[key] = holder(seed, lin_seed)
    return _MODELS[key]


# ---------------------------------------------------------------------------------------------------------------- units

@pytest.mark.parametrize("case", vc.conv_cases(), ids=lambda c: c["id"])
def test_conv_unit_vs_float64_at_the_dot_product_bound(case):
    x, (w, b) = vc.conv_input(case), vc.conv_params(case)
    ref, S, n = vc.conv_oracle(x, w, b)
    got = i2v_native.vgg_conv_unit(vc.to_cl(x, pad4=case["cin"] == 3).to(DEV), w, b).cpu().permute(0, 3, 1, 2)
    ok, ratio, l2 = vc.gate(got, ref, S, n)
    print(f"{case['id']}: worst |err| / bound {ratio:.3f}, worst rel-L2 {l2:.2e} (n = {n})")
    assert ok, (ratio, l2)


@pytest.mark.parametrize("cin,cout,hw", [(3, 64, (17, 33)), (16, 128, (9, 17)), (48, 64, (13, 21)), (64, 128, (17, 33))])
def test_batch_rows_equal_single_image_runs_bit_for_bit(cin, cout, hw):
    case = {"cin": cin, "cout": cout, "hw": hw, "batch": 3, "seed": 7900 + cin}
    x, (w, b) = vc.to_cl(vc.conv_input(case), pad4=cin == 3).to(DEV), vc.conv_params(case)
    full = i2v_native.vgg_conv_unit(x, w, b)
    for i in range(3):
        assert torch.equal(full[i:i + 1], i2v_native.vgg_conv_unit(x[i:i + 1].contiguous(), w, b)), i
    assert torch.equal(full, i2v_native.vgg_conv_unit(x, w, b))


@pytest.mark.parametrize("cin,cout", [(4, 64), (8, 64), (24, 64), (16, 32), (16, 96), (3, 16)])
def test_bad_channel_counts_are_refused(cin, cout):
    x = torch.zeros(1, 5, 5, 4 if cin == 3 else cin, device=DEV)
    with pytest.raises(i2v_native.I2VError, match="channels"):
        i2v_native.vgg_conv_unit(x, torch.zeros(cout, cin, 3, 3), torch.zeros(cout))


@pytest.mark.parametrize("shape", [(2, 8, 6, 10), (1, 64, 7, 9), (3, 128, 5, 4), (1, 512, 2, 3), (2, 4, 17, 33)])
@pytest.mark.parametrize("negative", [False, True])
def test_maxpool_bit_for_bit(shape, negative):
    x = vc.randn(8000 + shape[1] + shape[2], shape, negative)
    got = i2v_native.vgg_maxpool2(vc.to_cl(x).to(DEV)).cpu().permute(0, 3, 1, 2)
    assert torch.equal(got, vc.maxpool_oracle(x))


@pytest.mark.parametrize("hw", [(16, 16), (20, 24), (35, 29)])
def test_input_stage_lpips_mode_is_exact(hw):
    x = torch.from_numpy(vc.clips(8100 + hw[0], 2, 1, *hw))[:, 0].contiguous()
    got = i2v_native.vgg_input_stage(x.to(DEV), i2v_native.VGG_INPUT_LPIPS).cpu()
    shift, scale = torch.Tensor(vc.LPIPS_SHIFT)[None, :, None, None], torch.Tensor(vc.LPIPS_SCALE)[None, :, None, None]
    assert torch.equal(got[..., :3].permute(0, 3, 1, 2), (x - shift) / scale)          # ScalingLayer.forward in fp32
    assert torch.count_nonzero(got[..., 3]) == 0
    assert vc.rel_l2(got[..., :3].permute(0, 3, 1, 2), vc.input_oracle(x, "lpips")) <= 1e-6
    with pytest.raises(i2v_native.I2VError, match="resize"):
        i2v_native.vgg_input_stage(x.to(DEV), i2v_native.VGG_INPUT_LPIPS, (224, 224))


@pytest.mark.parametrize("hw,size", [((16, 16), (224, 224)), ((20, 24), (224, 224)), ((64, 64), (224, 224)), ((30, 40), (17, 23)), ((16, 16), (16, 16))])
@pytest.mark.parametrize("align_corners", [False, True])
def test_input_stage_diversity_mode(hw, size, align_corners):
    x = torch.from_numpy(vc.clips(8200 + hw[0], 2, 1, *hw))[:, 0].contiguous()
    got = i2v_native.vgg_input_stage(x.to(DEV), i2v_native.VGG_INPUT_DIVERSITY, size, align_corners).cpu()
    ref = vc.input_oracle(x, "diversity", size, align_corners)
    err = vc.rel_l2(got[..., :3].permute(0, 3, 1, 2), ref)
    print(f"{hw} -> {size} align_corners={align_corners}: rel-L2 {err:.2e}")
    assert tuple(got.shape) == (2, *size, 4) and err <= 1e-6 and torch.count_nonzero(got[..., 3]) == 0
    if hw != size:     # the other align_corners value is another function: the gate tells them apart
        assert vc.rel_l2(got[..., :3].permute(0, 3, 1, 2), vc.input_oracle(x, "diversity", size, not align_corners)) > 1e-4


def test_lpips_layer_and_pairdiff_units_vs_float64():
    for k, c in enumerate(vc.CHNS):
        f0, f1 = torch.relu(vc.randn(8300 + k, (3, c, 5, 7))), torch.relu(vc.randn(8310 + k, (3, c, 5, 7)))
        f0[0, :, 0, 0] = 0                                   # an all-zero feature vector: 0 / (0 + 1e-10), not 0 / 0
        lin = torch.from_numpy(vc.lin_state_dict(9)[f"lin{k}.model.1.weight"]).flatten()
        out = torch.zeros(3, dtype=torch.float64, device=DEV)
        i2v_native.lpips_layer(vc.to_cl(f0).to(DEV), vc.to_cl(f1).to(DEV), lin.to(DEV), out)
        i2v_native.lpips_layer(vc.to_cl(f0).to(DEV), vc.to_cl(f1).to(DEV), lin.to(DEV), out)     # accumulates
        ref = 2 * vc.lpips_layer_oracle(f0, f1, lin)
        assert torch.isfinite(out).all() and float(((out.cpu() - ref).abs() / ref).max()) <= 1e-12, (k, out, ref)
    for r, d in ((2, 1000), (5, 64 * 9 * 11), (16, 300001)):
        f = vc.randn(8400 + r, (r, d))
        acc = torch.zeros(2, dtype=torch.float64, device=DEV)
        i2v_native.vgg_pairdiff_update(f.to(DEV), acc)
        i2v_native.vgg_pairdiff_update(f.to(DEV), acc)
        ref = 2 * sum(float(((f[i].double() - f[j].double()) ** 2).mean()) for i in range(r) for j in range(r) if i != j)
        s, cnt = acc.cpu().tolist()
        assert cnt == 2 * r * (r - 1) and abs(s - ref) <= 1e-12 * ref, (r, d, s, ref)
    with pytest.raises(i2v_native.I2VError, match="maps"):
        i2v_native.vgg_pairdiff_update(torch.zeros(17, 8, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- trunk vs the reference

@pytest.mark.parametrize("fixture", ["vgg_taps_16", "vgg_taps_odd"])
def test_five_taps_vs_reference(fixture):
    arr, meta = vc.load_fixture(fixture)
    x = vc.randn(meta["input"]["seed"], tuple(meta["input"]["shape"]))
    out = model("vgg", meta["weights"]["seed"])(x.to(DEV))
    assert out._fields == vc.TAPS
    for name, got in zip(vc.TAPS, out):
        err = vc.rel_l2(got.cpu(), arr[name])
        print(f"{fixture} {name} {tuple(got.shape)}: rel-L2 {err:.2e}")
        assert list(got.shape) == meta["taps"][name]["shape"] and err <= vc.TOL_L2, (name, err)


@pytest.mark.parametrize("ac", [0, 1])
def test_taps_at_224_behind_the_diversity_input_stage(ac):
    arr, meta = vc.load_fixture("vgg_224")
    f = meta["frame"]
    frame = torch.from_numpy(vc.clips(f["seed"], 1, 1, f["h"], f["w"]))[0].contiguous()
    x = i2v_native.vgg_input_stage(frame.to(DEV), i2v_native.VGG_INPUT_DIVERSITY, (224, 224), bool(ac))
    taps = model("vgg", meta["weights"]["seed"]).taps(x)
    for name, t in zip(vc.TAPS, taps):
        st = meta["taps"][f"ac{ac}"][name]
        t = t.permute(0, 3, 1, 2).double()
        assert list(t.shape) == st["shape"]
        assert abs(float(t.norm()) - st["l2"]) <= vc.TOL_L2 * st["l2"] and abs(float(t.mean()) - st["mean"]) <= vc.TOL_L2 * st["l2"] / t.numel() ** 0.5, name
    err = vc.rel_l2(taps[4].permute(0, 3, 1, 2).cpu(), arr[f"relu5_3_ac{ac}"])
    print(f"vgg_224 align_corners={ac} relu5_3: rel-L2 {err:.2e}")
    assert err <= vc.TOL_L2
    assert vc.rel_l2(taps[4].permute(0, 3, 1, 2).cpu(), arr[f"relu5_3_ac{1 - ac}"]) > vc.TOL_L2     # the two definitions differ


@pytest.mark.parametrize("tag", ["32x32", "24x40"])
def test_lpips_forward_and_score_vs_reference(tag):
    arr, meta = vc.load_fixture("vgg_lpips")
    sz, n = meta["sizes"][tag], meta["n"]
    seed = meta["first_seed"] + (0 if tag == "32x32" else 2)
    a = torch.from_numpy(vc.clips(seed, n, 1, sz["h"], sz["w"]))[:, 0]
    b = (0.7 * a + 0.3 * torch.from_numpy(vc.clips(seed + 1, n, 1, sz["h"], sz["w"]))[:, 0]).contiguous()
    m = model("lpips", meta["weights"]["seed"], meta["weights"]["lin_seed"])
    got = m(a.contiguous().to(DEV), b.to(DEV))
    assert tuple(got.shape) == (n, 1, 1, 1) and got.is_cuda
    ref = arr[f"lpips32_{tag}"].astype(np.float64)
    rel = float(np.max(np.abs(got.flatten().cpu().double().numpy() - ref) / np.abs(ref)))
    score = lpips_score(m, a.contiguous().to(DEV), b.to(DEV))
    srel = abs(score - sz["score_fp32"]) / abs(sz["score_fp32"])
    print(f"lpips {tag}: per image rel {rel:.2e} (gate {sz['per_image_gate']['gate_rel']:.2e}), score {score!r} rel {srel:.2e} "
          f"(gate {sz['gate']['gate_rel']:.2e})")
    assert rel <= sz["per_image_gate"]["gate_rel"] and srel <= sz["gate"]["gate_rel"]
    assert torch.equal(got, m(a.contiguous().to(DEV), b.to(DEV)))                     # two runs, the same bits


def test_vgg_diversity_vs_reference(capsys):
    _, meta = vc.load_fixture("vgg_diversity")
    c = meta["clips"]
    videos = torch.from_numpy(vc.clips(c["seed"], c["n"] * c["r"], c["t"], c["h"], c["w"])).reshape(c["n"], c["r"], c["t"], 3, c["h"], c["w"])
    m = model("vgg", meta["weights"]["seed"])
    got = compute_vgg_diversity(videos.to(DEV), m)
    out = capsys.readouterr().out
    rel = abs(got - meta["diversity_fp32"]) / abs(meta["diversity_fp32"])
    print(f"vgg diversity {got!r} vs reference fp32 {meta['diversity_fp32']!r}: rel {rel:.2e} (gate {meta['gate']['gate_rel']:.2e})")
    assert rel <= meta["gate"]["gate_rel"]
    assert "Evaluate Diversity score based on VGG trained on ImageNet" in out and f"Diversity score of {got} using VGG backbone" in out
    assert compute_vgg_diversity(videos.to(DEV), m) == got                            # two runs, the same bits
    assert abs(compute_vgg_diversity(videos.to(DEV), m, align_corners=True) - got) > meta["gate"]["gate_rel"] * got
    with pytest.raises(AssertionError):
        compute_vgg_diversity((videos.to(DEV) + 1) / 2, m)                             # [0, 1] input: the reference's range check


def test_two_runs_and_graph_replay_give_the_same_bits():
    m = model("vgg", 41)
    native = m.native()
    x = vc.to_cl(vc.randn(8500, (2, 3, 35, 29)), pad4=True).to(DEV)
    x2 = vc.to_cl(vc.randn(8501, (2, 3, 35, 29)), pad4=True).to(DEV)
    ref, ref2 = [t.clone() for t in native.features(x)], [t.clone() for t in native.features(x2)]
    for a, b in zip(ref, native.features(x)):
        assert torch.equal(a, b)
    x_s = x.clone()
    out = [torch.empty_like(t) for t in ref]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        native.features(x_s, out)
    for src, want in ((x, ref), (x2, ref2)):
        x_s.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(want, out):
            assert torch.equal(a, b)
