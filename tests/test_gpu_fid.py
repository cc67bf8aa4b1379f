"""GPU checks of the native FID Inception-v3 trunk (csrc/i2v_inception.hip): one BasicConv2d of every window shape against the float64 oracle
at the element-wise dot-product bound over ragged tiles, channel slices and batches; the four pools; every Mixed block kind per branch; the
whole trunk at the smallest and at a non-square input; the fixtures written from the reference's own modules
(tests/golden/make_golden_fid.py); the input stage; repeatability and graph capture."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_common as fc
import i2v_native
from metrics.FID import FID_Score
from metrics.FID.inception import InceptionV3

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0

_MODELS = {}


def model(seed, blocks=(3,), resize=True, normalize=False):
    """InceptionV3 filled from the synthesiser (no file involved)."""
    key = (seed, tuple(blocks), resize, normalize)
    if key not in _MODELS:
        m = InceptionV3(output_blocks=list(blocks), resize_input=resize, normalize_input=normalize)
        m.load_state_dict(fc.torch_state_dict(seed))
        _MODELS[key] = m.to(DEV).eval()
    return _MODELS[key]


def nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- conv unit

def run_conv(case, x_nchw=None):
    """-> (got [N, cout, H', W'] on the host, the full output tensor, its channel offset)."""
    x = fc.conv_input(case) if x_nchw is None else x_nchw
    w, bn = fc.conv_params(case)
    xc = fc.to_cl(x, pad4=case["cin"] == 3)
    in_off, out, out_off = 0, None, 0
    if case["slices"]:                       # the input is a channel slice of a wider tensor, the output a slice of a sentinel-filled one
        in_off, out_off = 8, 12
        wide = torch.full((*xc.shape[:3], xc.shape[3] + 20), 1e30)
        wide[..., in_off:in_off + xc.shape[3]] = xc
        xc = wide
        (kh, kw), s, (ph, pw), (h, wd) = case["kernel"], case["stride"], case["padding"], case["hw"]
        out = torch.full((x.shape[0], (h + 2 * ph - kh) // s + 1, (wd + 2 * pw - kw) // s + 1, case["cout"] + 16), SENTINEL, device=DEV)
    full = i2v_native.inception_conv_unit(xc.to(DEV), w, bn, case["stride"], case["padding"], in_off=in_off, out=out, out_off=out_off)
    return nchw(full[..., out_off:out_off + case["cout"]]), full, out_off


_WORST = []


@pytest.mark.parametrize("case", fc.conv_cases(), ids=lambda c: c["id"])
def test_conv_unit_vs_float64_at_the_dot_product_bound(case):
    x = fc.conv_input(case)
    w, bn = fc.conv_params(case)
    ref, S, n = fc.conv_oracle(x, w, bn, case["stride"], case["padding"])
    got, full, off = run_conv(case)
    ok, ratio, l2 = fc.gate(got, ref, S, n)
    _WORST.append((ratio, l2, case["id"]))
    print(f"{case['id']}: worst |err| / bound {ratio:.3f}, worst rel-L2 {l2:.2e} (n = {n}); so far {max(_WORST)[0]:.3f} / {max(w[1] for w in _WORST):.2e}")
    assert n == fc.padded_k(case["cin"], *case["kernel"]) + 1 and ok, (ratio, l2)
    if case["slices"]:
        rest = torch.cat([full[..., :off], full[..., off + case["cout"]:]], -1)
        assert torch.all(rest == SENTINEL)                                  # the other channels of the output stay untouched


@pytest.mark.parametrize("i", [0, 5, 9, 12, 17, 21, 24, 26])      # 24, 26: the 128-column tile
def test_batch_rows_equal_single_image_runs_bit_for_bit(i):
    case = dict(fc.conv_cases()[i], batch=3, slices=False)
    x = fc.conv_input(case)
    full = run_conv(case, x)[0]
    for b in range(3):
        assert torch.equal(full[b:b + 1], run_conv(case, x[b:b + 1].contiguous())[0]), b
    assert torch.equal(full, run_conv(case, x)[0])


@pytest.mark.parametrize("cin,cout,kernel,stride,padding", [(8, 32, (3, 3), 1, (0, 0)), (24, 32, (1, 1), 1, (0, 0)), (16, 32, (9, 1), 1, (0, 0)),
                                                            (16, 32, (3, 3), 3, (0, 0)), (16, 32, (3, 3), 1, (3, 0))])
def test_unserved_conv_shapes_are_refused(cin, cout, kernel, stride, padding):
    x = torch.zeros(1, 12, 12, cin, device=DEV)
    bn = tuple(np.ones(cout, dtype=np.float32) for _ in range(4))
    with pytest.raises(i2v_native.I2VError, match="channels"):
        i2v_native.inception_conv_unit(x, torch.zeros(cout, cin, *kernel), bn, stride, padding)


# ---------------------------------------------------------------------------------------------------------------- pools

@pytest.mark.parametrize("hw", fc.MAXPOOL_MAPS)
@pytest.mark.parametrize("kind", [fc.POOL_MAX_S2, fc.POOL_MAX_S1])
@pytest.mark.parametrize("negative", [False, True])
def test_max_pools_bit_for_bit(hw, kind, negative):
    x = fc.randn(12000 + 10 * hw[0] + kind, (2, 8, *hw), negative)
    got = nchw(i2v_native.inception_pool(fc.to_cl(x).to(DEV), kind))
    assert torch.equal(got, fc.pool_oracle(x, kind)[0])
    if negative and kind == fc.POOL_MAX_S1:                                     # zero padding would win over an all-negative map
        assert not torch.equal(got, fc.pool_oracle(x, kind, "zero_pad_max")[0])
    if kind == fc.POOL_MAX_S2 and hw[0] % 2 == 0:                               # an even extent: ceil mode has one more row
        assert tuple(got.shape) != tuple(fc.pool_oracle(x, kind, "ceil_mode")[0].shape)


def test_max_pool_writes_its_channel_slice():
    x = fc.randn(12100, (2, 8, 7, 9))
    out = torch.full((2, 3, 4, 20), SENTINEL, device=DEV)
    i2v_native.inception_pool(fc.to_cl(x).to(DEV), fc.POOL_MAX_S2, out=out, out_off=8)
    assert torch.equal(nchw(out[..., 8:16]), F.max_pool2d(x, 3, 2)) and torch.all(out[..., :8] == SENTINEL) and torch.all(out[..., 16:] == SENTINEL)


@pytest.mark.parametrize("hw", fc.AVGPOOL_MAPS)
def test_avg_pool_vs_float64(hw):
    x = fc.randn(12200 + 10 * hw[0] + hw[1], (2, 12, *hw))
    ref, S, n = fc.pool_oracle(x, fc.POOL_AVG)
    got = nchw(i2v_native.inception_pool(fc.to_cl(x).to(DEV), fc.POOL_AVG))
    ok, ratio, l2 = fc.gate(got, ref, S, n)
    print(f"avg pool {hw}: worst |err| / bound {ratio:.3f}, rel-L2 {l2:.2e}")
    assert ok, (ratio, l2)
    if hw != (1, 1):
        bad = fc.pool_oracle(x, fc.POOL_AVG, "count_pad")
        assert not fc.gate(got, bad[0], bad[1], n)[0]                           # the padded divisor is another function
    else:
        assert torch.equal(got, x)                                              # one tap, divisor 1


@pytest.mark.parametrize("shape", [(2, 2048, 1, 1), (3, 64, 1, 2), (2, 768, 5, 7), (1, 8, 35, 35)])
def test_global_average_vs_float64(shape):
    x = fc.randn(12300 + shape[1], shape)
    ref, S, n = fc.global_avg_oracle(x)
    got = i2v_native.inception_global_avg(fc.to_cl(x).to(DEV)).cpu()
    ok, ratio, l2 = fc.gate(got, ref, S, n)
    print(f"global average {shape}: worst |err| / bound {ratio:.3f}, rel-L2 {l2:.2e}")
    assert ok, (ratio, l2)


# ---------------------------------------------------------------------------------------------------------------- Mixed blocks

SEED_MIXED = 91


def gpu_unit(sd, key, x_cl):
    _, _, _, stride, padding = fc.UNITS[key]
    return i2v_native.inception_conv_unit(x_cl, sd[key + ".conv.weight"], tuple(sd[f"{key}.bn.{n}"] for n in ("weight", "bias", "running_mean", "running_var")),
                                          stride, padding)


@pytest.mark.parametrize("block,batch,hw", fc.MIXED_CASES, ids=[c[0] for c in fc.MIXED_CASES])
def test_mixed_block_per_branch(block, batch, hw):
    sd = fc.fid_state_dict(SEED_MIXED)
    name, kind, cin, par = fc.MIXED[fc.BLOCK_NAMES.index(block)]
    bi = fc.BLOCK_NAMES.index(block)
    x = fc.randn(13000 + bi, (batch, cin, *hw))
    xc = fc.to_cl(x).to(DEV)
    native = model(SEED_MIXED).native()
    cin_n, cout, ohw = native.mixed_shape(bi, *hw)
    out = torch.full((batch, *ohw, cout), float("nan"), device=DEV)
    native.mixed(bi, xc, out)
    assert cin_n == cin and torch.isfinite(out).all()
    if kind == "B":
        assert (hw, ohw) == ((7, 9), (3, 4))
    # the GPU's own intermediates in front of every branch's last step: the same kernel on the same packed weights
    first = []
    for pre, _ in fc.block_branches(kind, par):
        h = xc
        for step in pre:
            h = i2v_native.inception_pool(h, step) if isinstance(step, int) else gpu_unit(sd, f"{name}.{step}", h)
        first.append(nchw(h) if pre else None)
    got, off = nchw(out), 0
    for k, (ref, S, n) in enumerate(fc.mixed_oracle(sd, block, x, first=first)):
        c = ref.shape[1]
        piece = got[:, off:off + c]
        if S is None:
            assert torch.equal(piece, ref.float()), (block, k)
        else:
            ok, ratio, l2 = fc.gate(piece, ref, S, n)
            print(f"{block} slice {k} [{off}, +{c}): worst |err| / bound {ratio:.3f}, rel-L2 {l2:.2e}")
            assert ok, (block, k, ratio, l2)
        off += c
    assert off == cout
    whole = fc.mixed_cat(fc.mixed_oracle(sd, block, x))
    assert max(fc.rel_l2_rows(got, whole)) <= fc.TOL_L2
    assert max(fc.rel_l2_rows(got, fc.mixed_cat(fc.mixed_oracle(sd, block, x, mutate="cat_order")))) > fc.TOL_L2


# ---------------------------------------------------------------------------------------------------------------- trunk

@pytest.mark.parametrize("batch,hw", [(2, (75, 75)), (1, (83, 107))])
def test_trunk_without_resize_vs_float64(batch, hw):
    sd = fc.fid_state_dict(SEED_MIXED)
    x = torch.from_numpy(fc.clips(14000 + hw[0], batch, 1, *hw))[:, 0].contiguous()
    outs = model(SEED_MIXED, (0, 1, 2, 3), resize=False)(x.to(DEV))
    refs = fc.trunk_oracle(sd, x)
    if hw == (75, 75):
        assert [tuple(r.shape[2:]) for r in refs] == [(17, 17), (7, 7), (3, 3), (1, 1)]
    else:
        assert tuple(refs[2].shape[2:]) == (3, 5)
    for b, (got, ref) in enumerate(zip(outs, refs)):
        l2 = max(fc.rel_l2_rows(got.cpu(), ref))
        print(f"trunk {hw} block {b} {tuple(got.shape)}: worst rel-L2 {l2:.2e}")
        assert tuple(got.shape) == tuple(ref.shape) and l2 <= fc.TOL_L2, (b, l2)


@pytest.mark.parametrize("hw", [(74, 80), (80, 74)])
def test_inputs_below_75_are_refused(hw):
    m = model(SEED_MIXED, (3,), resize=False)
    with pytest.raises(i2v_native.I2VError, match="75"):
        m(torch.zeros(1, 3, *hw, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- reference fixtures

@pytest.mark.parametrize("tag", ["16x16", "64x48"])
def test_block3_at_299_vs_reference(tag):
    arr, meta = fc.load_fixture("fid_feats_299")
    f = meta["frames"][tag]
    x = torch.from_numpy(fc.clips(f["seed"], f["n"], 1, f["h"], f["w"]))[:, 0].contiguous()
    got = model(meta["weights"]["seed"])(x.to(DEV))[0]
    assert tuple(got.shape) == (f["n"], 2048, 1, 1)
    l2 = max(fc.rel_l2_rows(got.cpu().flatten(1), torch.from_numpy(arr[f"block3_{tag}"])))
    print(f"fid_feats_299 {tag}: worst rel-L2 {l2:.2e}")
    assert l2 <= fc.TOL_L2


def test_blocks_0_to_2_vs_reference():
    _, meta = fc.load_fixture("fid_blocks")
    f = meta["frame"]
    x = torch.from_numpy(fc.clips(f["seed"], f["n"], 1, f["h"], f["w"]))[:, 0].contiguous()
    outs = model(meta["weights"]["seed"], (0, 1, 2))(x.to(DEV))
    for b, t in enumerate(outs):
        st = meta["blocks"][str(b)]
        t = t.double()
        assert list(t.shape) == st["shape"]
        assert abs(float(t.norm()) - st["l2"]) <= fc.TOL_L2 * st["l2"] and abs(float(t.mean()) - st["mean"]) <= fc.TOL_L2 * st["l2"] / t.numel() ** 0.5, b


def score_sets(meta):
    im = meta["images"]
    return [torch.from_numpy(fc.clips(im["seed"] + k, im["n"], 1, im["h"], im["w"]))[:, 0].contiguous() for k in (0, 1)]


def test_calculate_fid_vs_reference():
    _, meta = fc.load_fixture("fid_score")
    gen, orig = score_sets(meta)
    m = model(meta["weights"]["seed"])
    got, num = FID_Score.calculate_FID(m, gen.to(DEV), orig.to(DEV), meta["images"]["batch_size"], 2048)
    rel = abs(got - meta["fid_fp32_eigh"]) / abs(meta["fid_fp32_eigh"])
    print(f"FID {got!r} vs reference fp32 {meta['fid_fp32_eigh']!r}: rel {rel:.2e} (gate {meta['gate']['gate_rel']:.2e})")
    assert num == meta["images"]["n"] and rel <= meta["gate"]["gate_rel"]
    assert FID_Score.calculate_FID(m, gen, orig, meta["images"]["batch_size"], 2048)[0] == got         # host tensors move batch by batch; same bits


def test_accumulator_in_uneven_batches_uses_all_images():
    _, meta = fc.load_fixture("fid_score")
    gen, orig = score_sets(meta)
    acc = FID_Score.FIDAccumulator(model(meta["weights"]["seed"]))
    for lo, hi in ((0, 7), (7, 8), (8, 20)):
        acc.update(gen[lo:hi].to(DEV), "gen")
    for lo, hi in ((0, 11), (11, 20)):
        acc.update(orig[lo:hi].to(DEV), "orig")
    got = acc.compute()
    rel = abs(got - meta["fid_all_fp64_eigh"]) / abs(meta["fid_all_fp64_eigh"])
    print(f"FIDAccumulator {got!r} vs all 20 images {meta['fid_all_fp64_eigh']!r}: rel {rel:.2e}")
    assert acc.state()["gen"]["n"] == 20 and rel <= meta["gate"]["gate_rel"]
    assert abs(got - meta["fid_fp64_eigh"]) / abs(meta["fid_fp64_eigh"]) > meta["gate"]["gate_rel"]    # ... not the value of the 16 the quirk keeps


# ---------------------------------------------------------------------------------------------------------------- input stage, capture

@pytest.mark.parametrize("hw,resize", [((16, 16), True), ((64, 48), True), ((128, 128), True), ((256, 256), True), ((598, 598), True), ((75, 80), False)])
@pytest.mark.parametrize("normalize", [False, True])
def test_input_stage_vs_float64(hw, resize, normalize):
    """The stage is torch's fp32 ``upsample_bilinear2d`` arithmetic, whose source index ``scale * (dst + 0.5) - 0.5`` is rounded at
    2^-24 of its magnitude: against float64 that arithmetic itself reaches 1e-6 at the sizes below (torch's own fp32 result on the CPU:
    1.6e-7 at 16 x 16, 3.4e-7 at 128 x 128, 6.8e-7 at 256 x 256, 3.4e-8 at the exact 2:1 reduction from 598 x 598) and misses it for a
    source just above 299 (300 x 310: 1.30e-6, the same figure from torch's fp32 and from this kernel) -- such sizes are not in the list."""
    x = torch.from_numpy(fc.clips(15000 + hw[0], 2, 1, *hw))[:, 0].contiguous()
    got = i2v_native.inception_input_stage(x.to(DEV), resize, normalize).cpu()
    err = fc.rel_l2(got[..., :3].permute(0, 3, 1, 2), fc.input_oracle(x, resize, normalize))
    print(f"{hw} resize={resize} normalize={normalize}: rel-L2 {err:.2e}")
    assert tuple(got.shape) == (2, *((299, 299) if resize else hw), 4) and err <= 1e-6 and torch.count_nonzero(got[..., 3]) == 0
    if resize:
        assert fc.rel_l2(got[..., :3].permute(0, 3, 1, 2), fc.input_oracle(x, resize, normalize, align_corners=True)) > 1e-6
    elif not normalize:
        assert torch.equal(got[..., :3].permute(0, 3, 1, 2), x)                 # the default path applies no range change


def test_two_runs_and_graph_replay_give_the_same_bits():
    m = model(SEED_MIXED, (0, 1, 2, 3), resize=False)
    native = m.native()
    x = fc.to_cl(torch.from_numpy(fc.clips(16000, 2, 1, 75, 91))[:, 0], pad4=True).to(DEV)
    x2 = fc.to_cl(torch.from_numpy(fc.clips(16001, 2, 1, 75, 91))[:, 0], pad4=True).to(DEV)
    ref, ref2 = [t.clone() for t in native.features(x, (0, 1, 2, 3))], [t.clone() for t in native.features(x2, (0, 1, 2, 3))]
    for a, b in zip(ref, native.features(x, (0, 1, 2, 3))):
        assert torch.equal(a, b)
    assert torch.equal(native.features(x, (3,))[0], ref[3])                     # the buffer plan does not change the bits
    x_s = x.clone()
    out = [torch.empty_like(t) for t in ref]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        native.features(x_s, (0, 1, 2, 3), out)
    for src, want in ((x, ref), (x2, ref2)):
        x_s.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(want, out):
            assert torch.equal(a, b)
