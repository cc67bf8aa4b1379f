"""Device-side output stage on the GPU: the bytes of ``frames_to_u8`` / ``FrameSink`` / ``-dev_out`` EQUAL the bytes of the host path
(``convert_seq2gif`` / ``convert_grid2gif`` + ``astype(uint8)``, the torch expression of ``to_uint8_clips``) -- no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import i2v_synth as synth
from conftest import load_golden

pytestmark = pytest.mark.gpu


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _frames(shape, gain=1.5, seed=0):
    """tanh(gain * randn) with exact -1, exact 0 and a value below -1 planted; from gain 1 on also exact +1 and values above it (the
    strip's peak is then 1 after the clamp; below gain 1 the peak stays inside (0, 1) and the scale is a non-trivial float)."""
    x = torch.tanh(gain * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))
    flat = x.view(-1)
    planted = (-1.0, 0.0, -2.5, -0.99999994) + ((1.0, 1.75, 1.0000001) if gain >= 1 else ())
    for i, v in enumerate(planted):
        flat[(i * 7919) % flat.numel()] = v
    return x


def _host_strip(x):
    from utils import auxiliaries as aux
    return (aux.convert_grid2gif(x) if x.dim() == 6 else aux.convert_seq2gif(x)).astype(np.uint8)


def _unit_expr(x):
    return torch.clamp(x * 0.5 + 0.5, 0.0, 1.0).mul(255).add(0.5).clamp(0, 255).movedim(-3, -1).to(torch.uint8)


# (N, K, T, H, W): BAIR and Landscape frames, grids, a ragged width, one sample
GEOMS = [(6, 1, 16, 64, 64), (4, 1, 16, 128, 128), (6, 3, 16, 64, 64), (3, 3, 4, 128, 128), (5, 1, 3, 9, 7), (6, 3, 2, 5, 6), (1, 1, 16, 64, 64),
         (2, 1, 2, 4, 1)]


@pytest.mark.parametrize("n,k,t,h,w", GEOMS)
@pytest.mark.parametrize("gain", [0.4, 3.0])
def test_strip_and_grid_bytes_equal_the_host_path(n, k, t, h, w, gain):
    from utils import auxiliaries as aux
    x = _frames((n // k, k, t, 3, h, w) if k > 1 else (n, t, 3, h, w), gain, seed=n + k)
    fn = aux.convert_grid2gif_u8 if k > 1 else aux.convert_seq2gif_u8
    out = fn(x.cuda())
    assert out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), _host_strip(x))
    assert torch.equal(aux.to_uint8_clips(x.cuda()).cpu(), _unit_expr(x))


@pytest.mark.parametrize("w", [64, 6])
def test_strided_samples_are_read_in_place(w):
    """A [:, :16] view of a T = 32 buffer (what decode_sequence leaves at vid_length 32), for a strip and for the [F, K] grid view."""
    from utils import auxiliaries as aux
    buf = _frames((6, 32, 3, 64, w), 2.0, seed=3).cuda()
    view = buf[:, :16]
    assert not view.is_contiguous()
    assert np.array_equal(aux.convert_seq2gif_u8(view).cpu().numpy(), _host_strip(view.cpu()))
    grid = buf.view(2, 3, 32, 3, 64, w)[:, :, :16]
    assert np.array_equal(aux.convert_grid2gif_u8(grid).cpu().numpy(), _host_strip(grid.cpu()))
    assert torch.equal(aux.to_uint8_clips(grid).cpu(), _unit_expr(grid.cpu()))
    assert torch.equal(buf.cpu(), _frames((6, 32, 3, 64, w), 2.0, seed=3))      # the input is left untouched


@pytest.mark.parametrize("k", [1, 3])
def test_accumulated_peak_and_column_blocks(k):
    """Three batches, one accumulated peak, each batch into its own column block of ONE strip == the concatenation converted at once."""
    import i2v_native
    t, h, w = 16, 64, 64
    batches = [_frames((f, k, t, 3, h, w) if k > 1 else (f, t, 3, h, w), g, seed=10 + i) for i, (f, g) in enumerate(((2, 0.3), (3, 2.5), (1, 0.8)))]
    whole = torch.cat(batches)
    peak = torch.full((1,), 123.0, device="cuda")       # accumulate=False must overwrite what is there
    for i, b in enumerate(batches):
        i2v_native.frames_peak(b.cuda(), out=peak, accumulate=i > 0)
    assert float(peak) == float(whole.max())
    d_peak = torch.clamp(peak.cpu() * 0.5 + 0.5, 0.0, 1.0)
    assert float(d_peak) == float(torch.clamp(whole * 0.5 + 0.5, 0.0, 1.0).max())
    strip = torch.zeros(t, k * h, 6 * w, 3, dtype=torch.uint8, device="cuda")
    col0 = 0
    for b in batches:
        i2v_native.frames_to_u8(b.cuda(), peak=peak, out=strip, mode="peak", col0=col0)
        col0 += b.shape[0] * w
    assert np.array_equal(strip.cpu().numpy(), _host_strip(whole))
    # a block placed at a row / column offset inside a larger canvas leaves the rest alone
    canvas = torch.full((t, k * h + 5, 6 * w + 3, 3), 7, dtype=torch.uint8, device="cuda")
    i2v_native.frames_to_u8(whole.cuda(), peak=peak, out=canvas, mode="peak", row0=5, col0=3)
    c = canvas.cpu().numpy()
    assert np.array_equal(c[:, 5:, 3:], _host_strip(whole)) and (c[:, :5] == 7).all() and (c[:, :, :3] == 7).all()
    # all-negative frames: the peak is the (negative) maximum, not the initial value
    neg = -0.25 - torch.rand(2, 2, 3, 8, 8)
    assert float(i2v_native.frames_peak(neg.cuda())) == float(neg.max())


def test_c_side_argument_errors_come_before_any_launch():
    import ctypes
    import i2v_native
    lib = i2v_native.lib()
    x = torch.zeros(4, 2, 3, 8, 8, device="cuda")
    dst = torch.zeros(2 * 8 * 32 * 3, dtype=torch.uint8, device="cuda")
    peak = torch.zeros(1, device="cuda")

    def cfg(**kw):
        base = dict(n=4, t=2, h=8, w=8, n_stride=0, k=1, layout=0, dst_row_bytes=96, dst_frame_bytes=768, dst_bytes=dst.numel(), row0=0, col0=0)
        base.update(kw)
        return ctypes.byref(i2v_native.FramesCfg(**base))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = [cfg(n=0), cfg(w=-1), cfg(k=3), cfg(col0=1), cfg(row0=1), cfg(dst_row_bytes=95), cfg(dst_bytes=100), cfg(layout=2), cfg(n_stride=5),
           cfg(layout=1, k=2), cfg(layout=1, dst_bytes=4 * 2 * 8 * 8 * 3 - 1)]
    for c in bad:
        assert lib.i2v_frames_to_u8(x.data_ptr(), c, None, dst.data_ptr(), 1, st) == -1
        assert lib.i2v_last_error()
    assert lib.i2v_frames_to_u8(None, cfg(), None, dst.data_ptr(), 1, st) == -1
    assert lib.i2v_frames_to_u8(x.data_ptr(), cfg(), None, None, 1, st) == -1
    assert lib.i2v_frames_to_u8(x.data_ptr(), cfg(), None, dst.data_ptr(), 0, st) == -1          # PEAK without a peak
    assert lib.i2v_frames_to_u8(x.data_ptr(), cfg(), peak.data_ptr(), dst.data_ptr(), 1, st) == -1   # UNIT with one
    assert lib.i2v_frames_to_u8(x.data_ptr(), cfg(), None, dst.data_ptr(), 7, st) == -1
    assert lib.i2v_frames_peak(x.data_ptr(), cfg(), None, 0, st) == -1
    assert lib.i2v_frames_peak(None, cfg(), peak.data_ptr(), 0, st) == -1
    assert lib.i2v_frames_peak(x.data_ptr(), cfg(t=0), peak.data_ptr(), 0, st) == -1
    torch.cuda.synchronize()
    assert not dst.any() and float(peak) == 0.0            # nothing was launched
    assert lib.i2v_frames_to_u8(x.data_ptr(), cfg(), None, dst.data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    assert bool((dst == 128).all())                        # trunc(0.5 * 255 + 0.5)


def test_side_stream_and_graph_replay():
    import i2v_native
    a, b = _frames((4, 16, 3, 64, 64), 0.5, seed=1), _frames((4, 16, 3, 64, 64), 4.0, seed=2)
    ref_a, ref_b = _host_strip(a), _host_strip(b)
    side = torch.cuda.Stream()
    xa = a.cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        peak = i2v_native.frames_peak(xa)
        out = i2v_native.frames_to_u8(xa, peak=peak, mode="peak")
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref_a)
    # capture the two launches, replay on new data in the same buffers
    x = a.cuda()
    peak = torch.zeros(1, device="cuda")
    out = torch.zeros(16, 64, 4 * 64, 3, dtype=torch.uint8, device="cuda")
    clips = torch.zeros(4, 16, 64, 64, 3, dtype=torch.uint8, device="cuda")
    i2v_native.frames_to_u8(x, out=clips, mode="unit", layout="clips")      # (every kernel of the capture has run once)
    clips.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        i2v_native.frames_peak(x, out=peak)
        i2v_native.frames_to_u8(x, peak=peak, out=out, mode="peak")
        i2v_native.frames_to_u8(x, out=clips, mode="unit", layout="clips")
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref_a) and torch.equal(clips.cpu(), _unit_expr(a))
    x.copy_(b.cuda())
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref_b) and torch.equal(clips.cpu(), _unit_expr(b)) and float(peak) == float(b.max())


@pytest.mark.parametrize("k", [1, 2])
def test_frame_sink_peak(k):
    from i2v_pipeline import FrameSink, FrameSinkBudgetError
    t, h, w = 16, 64, 64
    batches = [_frames((f, k, t, 3, h, w) if k > 1 else (f, t, 3, h, w), g, seed=20 + i) for i, (f, g) in enumerate(((3, 0.3), (2, 2.5), (3, 0.8)))]
    sink = FrameSink("peak")
    for job in range(2):                       # the sink is reusable; the second job sees the batches in another order
        order = batches if job == 0 else batches[::-1]
        for b in order:
            sink.add(b.cuda())
        sink.finish()
        res = sink.result()
        assert isinstance(res, np.ndarray) and res.dtype == np.uint8
        assert np.array_equal(res, _host_strip(torch.cat(order)))
    # budget: room for the first batch only; the refusal leaves the sink as it was and usable
    one = batches[0].numel() * 5
    small = FrameSink("peak", budget_bytes=one + 16)
    small.add(batches[0].cuda())
    with pytest.raises(FrameSinkBudgetError, match="budget"):
        small.add(batches[1].cuda())
    small.finish()
    assert np.array_equal(small.result(), _host_strip(batches[0]))
    small.add(batches[0].cuda())
    kept = small.drain()
    assert len(kept) == 1 and torch.equal(kept[0].cpu(), batches[0])
    small.add(batches[1][:1].cuda())
    small.finish()
    assert np.array_equal(small.result(), _host_strip(batches[1][:1]))
    with pytest.raises(RuntimeError):
        small.result()


def test_frame_sink_unit_double_buffered():
    from i2v_pipeline import FrameSink
    batches = [_frames((f, 16, 3, 64, 64), 1.0 + i, seed=30 + i) for i, f in enumerate((4, 2, 4, 3, 1))]
    sink = FrameSink("unit")
    got = []
    sink.add(batches[0].cuda())
    for b in batches[1:]:
        sink.add(b.cuda())                     # batch i + 1 enqueued while batch i is carried away
        got.append(sink.result().copy())       # (a view is valid until the next add)
    sink.add(batches[0].cuda())                # two in flight: the last batch and this one
    with pytest.raises(RuntimeError, match="in flight"):
        sink.add(batches[1].cuda())
    got.append(sink.result().copy())
    for g, b in zip(got, batches):
        assert g.dtype == np.uint8 and np.array_equal(g, _unit_expr(b).numpy())
    assert np.array_equal(sink.result(), _unit_expr(batches[0]).numpy())
    with pytest.raises(RuntimeError):
        sink.result()
    grid = _frames((2, 3, 16, 3, 64, 64), 2.0, seed=40)
    sink.add(grid.cuda())
    assert np.array_equal(sink.result(), _unit_expr(grid).numpy())


@pytest.mark.parametrize("mma", [1, "fp16"])
def test_model_u8_methods(tmp_path, mma):
    from get_model import Model
    from test_gpu_parity import _write_checkpoints
    from utils import auxiliaries as aux
    _, meta = load_golden("model_nf8")
    model = Model(_write_checkpoints(tmp_path, meta), 32, mma=mma)
    F, n = 2, 3
    x0, _, embed = synth.bench_inputs(F, 64, 64)
    residual = torch.randn(F * n, 64, generator=torch.Generator().manual_seed(4))
    seq = model.synthesize(x0.cuda(), residual=residual[:F].cuda(), embed=embed.cuda())
    u8 = model.synthesize_u8(x0.cuda(), residual=residual[:F].cuda(), embed=embed.cuda())
    assert u8.shape == (F, 32, 64, 64, 3) and u8.dtype == torch.uint8 and u8.is_cuda
    assert torch.equal(u8, aux.to_uint8_clips(seq)) and torch.equal(u8.cpu(), aux.to_uint8_clips(seq.cpu()))
    vids = model.sample(x0.cuda(), n, residual=residual.cuda(), embed=embed.cuda())
    v8 = model.sample_u8(x0.cuda(), n, residual=residual.cuda(), embed=embed.cuda())
    assert v8.shape == (F, n, 32, 64, 64, 3)
    assert torch.equal(v8, aux.to_uint8_clips(vids)) and torch.equal(v8.cpu(), aux.to_uint8_clips(vids.cpu()))
    model.check()


def _images(d, n, size=64, seed=1):
    from PIL import Image
    d.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (size, size, 3), dtype=np.uint8)).save(d / f"{i:02d}.png")


def _same_files(a, b, names):
    for name in names:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in b.iterdir())


@pytest.mark.parametrize("n_realiz", [1, 2])
def test_generate_samples_dev_out(tmp_path, n_realiz):
    import generate_samples
    from test_gpu_parity import _write_checkpoints
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta)
    _images(tmp_path / "imgs", 5)
    gpu = os.environ.get("HIP_VISIBLE_DEVICES", "0")
    base = ["-gpu", gpu, "-dataset", "bair", "-ckpt_path", ckpt, "-seq_length", "16", "-bs", "2", "-embed_seed", "3", "-seed", "9",
            "-img_path", str(tmp_path / "imgs") + "/", "-n_realiz", str(n_realiz)]
    generate_samples.main(base + ["-out_path", str(tmp_path / "a") + "/", "-raw_npy", str(tmp_path / "a.npy")])
    generate_samples.main(base + ["-out_path", str(tmp_path / "b") + "/", "-raw_npy", str(tmp_path / "b.npy"), "-dev_out"])
    _same_files(tmp_path / "a", tmp_path / "b", ["results.gif"])
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert a.dtype == b.dtype == np.uint8 and a.shape == (16, n_realiz * 64, 5 * 64, 3) and np.array_equal(a, b)


def test_generate_samples_dev_out_over_budget_finishes_on_the_host(tmp_path, monkeypatch):
    import generate_samples
    import i2v_pipeline
    from test_gpu_parity import _write_checkpoints
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta)
    _images(tmp_path / "imgs", 5)
    gpu = os.environ.get("HIP_VISIBLE_DEVICES", "0")
    base = ["-gpu", gpu, "-dataset", "bair", "-ckpt_path", ckpt, "-seq_length", "16", "-bs", "2", "-embed_seed", "3", "-seed", "9",
            "-img_path", str(tmp_path / "imgs") + "/"]
    generate_samples.main(base + ["-out_path", str(tmp_path / "a") + "/", "-raw_npy", str(tmp_path / "a.npy")])
    init = i2v_pipeline.FrameSink.__init__
    monkeypatch.setattr(i2v_pipeline.FrameSink, "__init__",
                        lambda self, mode="peak", **kw: init(self, mode, budget_bytes=2 * 16 * 3 * 64 * 64 * 5 * 3 // 2))   # 1.5 batches
    generate_samples.main(base + ["-out_path", str(tmp_path / "b") + "/", "-raw_npy", str(tmp_path / "b.npy"), "-dev_out"])
    _same_files(tmp_path / "a", tmp_path / "b", ["results.gif"])
    assert np.array_equal(np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy"))


def test_generate_transfer_dev_out(tmp_path):
    from PIL import Image
    import generate_transfer
    from test_gpu_parity import _write_checkpoints
    _, meta = load_golden("model_nf8")
    ckpt = _write_checkpoints(tmp_path, meta, with_embedder=True, with_encoder=True)
    rng = np.random.default_rng(1)
    for v in range(3):
        d = tmp_path / "clips" / f"v{v}"
        d.mkdir(parents=True)
        for i in range(17):
            Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(d / f"{i:03d}.png")
    base = ["-gpu", os.environ.get("HIP_VISIBLE_DEVICES", "0"), "-dataset", "bair", "-ckpt_path", ckpt, "-seq_length", "17", "-bs", "2",
            "-img_path", str(tmp_path / "clips") + "/"]
    generate_transfer.main(base + ["-out_path", str(tmp_path / "a") + "/"])
    generate_transfer.main(base + ["-out_path", str(tmp_path / "b") + "/", "-dev_out"])
    _same_files(tmp_path / "a", tmp_path / "b", [f"transfer_{i}.gif" for i in range(3)])
    gif = Image.open(tmp_path / "b" / "transfer_1.gif")
    assert gif.n_frames == 17 and gif.size == (4 * 64, 64)


def test_visualize_endpoint_dev_out(tmp_path):
    import yaml
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
    base = ["-gpu", os.environ.get("HIP_VISIBLE_DEVICES", "0"), "-ckpt_path", ckpt, "-img_path", str(tmp_path / "imgs") + "/",
            "-cond_npy", str(tmp_path / "cond.npy"), "-n_samples", "3", "-n_realiz", "3", "-bs", "2", "-seq_length", "16",
            "-embed_seed", "1", "-seed", "4"]
    visualize_endpoint.main(base + ["-out_path", str(tmp_path / "a") + "/"])
    visualize_endpoint.main(base + ["-out_path", str(tmp_path / "b") + "/", "-dev_out"])
    _same_files(tmp_path / "a", tmp_path / "b", [f"endpoint_{i}.{ext}" for i in range(3) for ext in ("gif", "png")])
