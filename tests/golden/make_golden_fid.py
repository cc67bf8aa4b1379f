"""Writes tests/golden/fid_*.npz from the REFERENCE's own ``metrics.FID.inception`` and ``metrics.FID.FID_Score`` (CPU, torch + scipy).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_fid.py [--only feats,blocks,score] [--check]

It imports the reference's two modules with stand-in modules in ``sys.modules`` for the duration of the import, here only: a ``torchvision``
whose ``models.inception_v3(...)`` and ``models.inception.Inception{A,B,C,D,E}`` / ``BasicConv2d`` are THIS script's statement of the public
torchvision graph (the layer table of tests/fid_common.py; the reference's FIDInception* classes derive from them and bring the pytorch-fid
patches), ``load_state_dict_from_url`` bound to the seeded synthesiser of tests/fid_common.py (no code path reaches the network), and an
``imageio`` without function.  Small inputs are regenerated from their seeds; results and statistics are stored -- never weights or
reference text.

Fixtures:
  fid_feats_299  block 3 [N, 2048] of two 16 x 16 frames and of one 64 x 48 frame, resized to 299 x 299 by the reference's forward
  fid_blocks     blocks 0-2 of the 64 x 48 frame as (shape, mean, L2), and the holder's state_dict key list
  fid_score      calculate_FID's two halves (get_activations per set on the CPU, calculate_frechet_distance) for two sets of 20 images at 32 x 32
                 with batch_size = 8 (2 batches used, 4 images dropped): the reference's
                 value (scipy sqrtm on its fp32 activations), the float64 ``eigh`` value on the fp32 and on the float64 activations, the
                 float64 activations themselves, and the value of all 20 images (what the streaming accumulator computes)
Scalar gate as in make_golden_dtfvd._gate: 10 x the reference's own fp32-vs-float64 relative deviation, 1e-6 when that is below 1e-7."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("I2V_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
import fid_common as fc  # noqa: E402

GATE_FLOOR = 1e-6
SEED_W = 81


# ---- the public torchvision Inception3 graph, stated from the layer table (fid_common.block_units)
class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class _Block(nn.Module):
    KIND = None

    def _build(self, cin, par):
        for suffix, (ci, co, kernel, stride, padding) in fc.block_units(self.KIND, cin, par).items():
            setattr(self, suffix, BasicConv2d(ci, co, kernel_size=kernel, stride=stride, padding=padding))


class InceptionA(_Block):
    KIND = "A"

    def __init__(self, in_channels, pool_features):
        super().__init__()
        self._build(in_channels, pool_features)


class InceptionB(_Block):
    KIND = "B"

    def __init__(self, in_channels):
        super().__init__()
        self._build(in_channels, None)

    def forward(self, x):
        dbl = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([self.branch3x3(x), dbl, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(_Block):
    KIND = "C"

    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        self._build(in_channels, channels_7x7)


class InceptionD(_Block):
    KIND = "D"

    def __init__(self, in_channels):
        super().__init__()
        self._build(in_channels, None)

    def forward(self, x):
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(_Block):
    KIND = "E"

    def __init__(self, in_channels):
        super().__init__()
        self._build(in_channels, None)


class Inception3(nn.Module):
    def __init__(self, num_classes=1000, aux_logits=True, pretrained=False, **kwargs):
        super().__init__()
        assert not aux_logits and not pretrained
        for key, cin, cout, kernel, stride, padding in fc.STEM:
            setattr(self, key, BasicConv2d(cin, cout, kernel_size=kernel, stride=stride, padding=padding))
        self.Mixed_5b, self.Mixed_5c, self.Mixed_5d = InceptionA(192, 32), InceptionA(256, 64), InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b, self.Mixed_6c, self.Mixed_6d, self.Mixed_6e = InceptionC(768, 128), InceptionC(768, 160), InceptionC(768, 160), InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b, self.Mixed_7c = InceptionE(1280), InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)


_REF = None


def ref_modules():
    """(inception module, FID_Score module) of the reference, imported under the stand-ins."""
    global _REF
    if _REF is not None:
        return _REF
    purge = lambda: [sys.modules.pop(k) for k in list(sys.modules) if k == "metrics" or k.startswith("metrics.")]  # noqa: E731
    purge()
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.inception = types.ModuleType("torchvision.models.inception")
    tv.models.utils = types.ModuleType("torchvision.models.utils")
    tv.models.utils.load_state_dict_from_url = lambda url, progress=True: fc.torch_state_dict(SEED_W)
    tv.models.inception_v3 = Inception3
    for cls in (InceptionA, InceptionB, InceptionC, InceptionD, InceptionE, BasicConv2d):
        setattr(tv.models.inception, cls.__name__, cls)
    io = types.ModuleType("imageio")
    io.imread = None
    stand = {"torchvision": tv, "torchvision.models": tv.models, "torchvision.models.inception": tv.models.inception,
             "torchvision.models.utils": tv.models.utils, "imageio": io}
    saved = {k: sys.modules.get(k) for k in stand}
    sys.modules.update(stand)
    sys.path.insert(0, REF)
    try:
        _REF = (importlib.import_module("metrics.FID.inception"), importlib.import_module("metrics.FID.FID_Score"))
    finally:
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        purge()
    return _REF


def ref_inception(blocks=(3,)):
    return ref_modules()[0].InceptionV3(output_blocks=list(blocks)).eval()     # resize_input=True, normalize_input=False: the reference's call


def pack(meta, **arrays):
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def _gate(rel):
    return {"measured": rel, "floored": bool(rel < 1e-7), "gate_rel": GATE_FLOOR if rel < 1e-7 else 10 * rel}


FRAMES = {"16x16": {"seed": 82, "n": 2, "h": 16, "w": 16}, "64x48": {"seed": 83, "n": 1, "h": 64, "w": 48}}


def frames(tag):
    f = FRAMES[tag]
    return torch.from_numpy(fc.clips(f["seed"], f["n"], 1, f["h"], f["w"], signed=True))[:, 0].contiguous()


def make_feats():
    model = ref_inception()
    arrays = {}
    with torch.no_grad():
        for tag in FRAMES:
            arrays[f"block3_{tag}"] = model(frames(tag))[0].flatten(1).numpy()
    for a in arrays.values():
        assert np.isfinite(a).all() and (np.count_nonzero(a, axis=1) >= 1024).all(), "degenerate features"
    meta = {"fixture": "fid_feats_299", "weights": {"seed": SEED_W}, "frames": FRAMES, "generator": "fvd_common.clips(seed, n, 1, h, w)[:, 0]",
            "note": "block3_<tag>: InceptionV3()(frames)[0] flattened to [n, 2048]; resize_input=True, normalize_input=False"}
    return pack(meta, **arrays)


def make_blocks():
    model = ref_inception((0, 1, 2))
    with torch.no_grad():
        outs = model(frames("64x48"))
    stats = {str(b): {"shape": list(t.shape), "mean": float(t.double().mean()), "l2": float(t.double().norm())} for b, t in enumerate(outs)}
    inner = ref_modules()[0].fid_inception_v3()
    meta = {"fixture": "fid_blocks", "weights": {"seed": SEED_W}, "frame": FRAMES["64x48"], "blocks": stats,
            "state_dict": [[k, list(v.shape)] for k, v in inner.state_dict().items() if not k.startswith("fc.")],
            "ignored": [[k, list(v.shape)] for k, v in inner.state_dict().items() if k.startswith("fc.")],
            "dims": {str(k): v for k, v in ref_modules()[0].InceptionV3.BLOCK_INDEX_BY_DIM.items()}}
    return pack(meta, blocks=np.asarray([[s["mean"], s["l2"]] for s in stats.values()]))


def make_score(seed=84, n=20, size=32, batch=8):
    from metrics_eigh import calculate_frechet_distance as eigh_fd
    inc_mod, score = ref_modules()
    gen = torch.from_numpy(fc.clips(seed, n, 1, size, size, signed=True))[:, 0].contiguous()
    orig = torch.from_numpy(fc.clips(seed + 1, n, 1, size, size, signed=True))[:, 0].contiguous()
    model = ref_inception()
    a32 = [score.get_activations(d, model, batch, 2048, cuda=False) for d in (gen, orig)]
    used = a32[0].shape[0]
    assert used == (n // batch) * batch == 16
    model64 = ref_inception().double()
    a64 = [score.get_activations(d.double(), model64, batch, 2048, cuda=False) for d in (gen, orig)]
    all64 = [score.get_activations(d.double(), model64, n, 2048, cuda=False) for d in (gen, orig)]
    for a in a32 + a64:
        assert np.isfinite(a).all() and np.count_nonzero(np.abs(a).sum(0)) >= 1024, "degenerate activations"
    st32, st64, st_all = [fc.frechet_stats(a) for a in a32], [fc.frechet_stats(a) for a in a64], [fc.frechet_stats(a) for a in all64]
    v32, v64 = eigh_fd(*st32[0], *st32[1]), eigh_fd(*st64[0], *st64[1])
    v_all = eigh_fd(*st_all[0], *st_all[1])
    sq = score.calculate_frechet_distance(*st32[0], *st32[1])      # the reference's own formulation (scipy sqrtm)
    r_prec, r_form = abs(v32 - v64) / abs(v64), abs(float(np.real(sq)) - v32) / abs(v32)
    meta = {"fixture": "fid_score", "weights": {"seed": SEED_W}, "images": {"seed": seed, "n": n, "h": size, "w": size, "batch_size": batch, "used": used},
            "fid_fp32_eigh": v32, "fid_fp64_eigh": v64, "fid_fp32_sqrtm": float(np.real(sq)), "fid_fp32_sqrtm_imag": float(np.abs(np.imag(sq))),
            "fid_all_fp64_eigh": v_all, "ref_fp32_vs_fp64_rel": r_prec, "eigh_vs_sqrtm_rel": r_form, "gate": _gate(r_prec),
            "note": "gen = clips(seed, n, 1, h, w)[:, 0], orig = clips(seed + 1, ...)[:, 0].  16 of 20 images are used (2 batches of 8; the "
                    "reference drops the rest): both covariances have rank 15.  fid_fp32_sqrtm is the reference's calculate_frechet_distance "
                    "(scipy sqrtm) on its fp32 activations, the *_eigh values the package's float64 eigenvalue formulation; fid_all_fp64_eigh uses "
                    "all 20 images (the streaming accumulator's value)"}
    return pack(meta, act64=np.stack(a64), fid=np.asarray([v32, v64, v_all]))


JOBS = {"feats": lambda: {"fid_feats_299": make_feats()}, "blocks": lambda: {"fid_blocks": make_blocks()}, "score": lambda: {"fid_score": make_score()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="feats,blocks,score")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    # the package's float64 eigh formulation (metrics/PyTorch_FVD/FVD_logging.py), loaded by file under a private name: the reference's
    # `metrics` package must stay the only one of that name while its modules are imported
    import importlib.util
    pkg = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
    sys.path.insert(0, pkg)                       # FVD_logging imports i2v_native and metrics.PyTorch_FVD.I3D
    spec = importlib.util.spec_from_file_location("metrics_eigh", os.path.join(pkg, "metrics", "PyTorch_FVD", "FVD_logging.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules["metrics_eigh"] = mod
    sys.path.remove(pkg)
    for k in [k for k in sys.modules if k == "metrics" or k.startswith("metrics.")]:
        sys.modules.pop(k)
    for job in args.only.split(","):
        for name, arrays in JOBS[job]().items():
            path = os.path.join(HERE, name + ".npz")
            if args.check:
                with np.load(path) as old:
                    worst = 0.0
                    for k in arrays:
                        if k == "meta":
                            assert bytes(old[k]) == bytes(arrays[k]), f"{name}: meta differs"
                        else:
                            a, b = old[k].astype(np.float64), arrays[k].astype(np.float64)
                            assert a.shape == b.shape, f"{name}.{k}: shape {b.shape}, committed {a.shape}"
                            diff = float(np.max(np.abs(a - b)))
                            # the reference runs in fp32 on the CPU: another BLAS or thread count may reorder its sums, nothing more
                            assert diff <= 1e-5 * float(np.max(np.abs(a))), f"{name}.{k}: max-abs difference {diff} from the committed fixture"
                            worst = max(worst, diff)
                print(f"{name}: max-abs difference {worst}")
            else:
                np.savez_compressed(path, **arrays)
                print(f"wrote {path} ({os.path.getsize(path)} bytes)", flush=True)


if __name__ == "__main__":
    main()
