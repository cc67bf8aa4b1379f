"""Writes tests/golden/vgg_*.npz from the REFERENCE's own ``stage2_cINN.AE.modules.vgg16`` and ``LPIPS`` (CPU, torch).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_vgg.py [--only taps,big,lpips,diversity] [--check]

It imports the reference's ``vgg16``, ``LPIPS``, ``normalize_tensor`` and ``spatial_average`` with stand-in modules in ``sys.modules`` for the
duration of the import, here only: a ``torchvision`` whose ``models.vgg16(pretrained)`` returns this script's own configuration-D
``Sequential`` filled from the seeded synthesiser of tests/vgg_common.py, and ``requests`` / ``tqdm`` stand-ins without function.  The LPIPS
module's ``get_ckpt_path`` is rebound to a temporary file written from the synthesiser before ``LPIPS()`` is constructed, so no code
path reaches the network; the reference constructors are never called unpatched.  Small inputs are regenerated from their seeds;
results and statistics are stored -- never weights or reference text.  ``metrics.Diversity.VGG`` is NOT imported (kornia, .cuda()): the
diversity expectation is the reference's ``vgg16`` behind ``F.interpolate(size=(224, 224), mode='bilinear', align_corners=False)`` of the
normalised frames, put through its pair loop (``vgg_common.pair_mean``).

Fixtures:
  vgg_taps_16    five taps of randn [2, 3, 16, 16]
  vgg_taps_odd   five taps of randn [1, 3, 35, 29]: every pool floors, the last map is 2 x 1
  vgg_224        relu5_3 and per-tap (shape, mean, L2) of one 20 x 24 frame behind the diversity input stage, both align_corners values
  vgg_lpips      LPIPS.forward of 12 image pairs at 32 x 32 and at 24 x 40: per image, fp32 and with the module in .double(); the CLI rule
  vgg_diversity  N = 2, R = 3, T = 2 at 16 x 16: the pair mean in fp32 and float64
Scalar gates as in make_golden_dtfvd._gate: 10 x the reference's own fp32-vs-fp64 relative deviation, 1e-6 when that is below 1e-7."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("I2V_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
import vgg_common as vc  # noqa: E402

GATE_FLOOR = 1e-6
SEED_W, SEED_LIN = 41, 42


def config_d(seed):
    """torchvision's vgg16 graph (features only matter) with the synthesiser's weights."""
    layers, cin = [], 3
    for v in (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M'):
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    m = nn.Module()
    m.features = nn.Sequential(*layers)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vc.vgg_state_dict(seed).items()}, strict=True)
    return m


_REF = None


def ref_modules():
    """(vgg16 module, LPIPS module) of the reference, imported under the stand-ins."""
    global _REF
    if _REF is not None:
        return _REF
    purge = lambda: [sys.modules.pop(k) for k in list(sys.modules) if k == "stage2_cINN" or k.startswith("stage2_cINN.")]  # noqa: E731
    purge()
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = lambda pretrained=True: config_d(SEED_W)
    tq = types.ModuleType("tqdm")
    tq.tqdm = None
    stand = {"torchvision": tv, "torchvision.models": tv.models, "requests": types.ModuleType("requests"), "tqdm": tq}
    saved = {k: sys.modules.get(k) for k in stand}
    sys.modules.update(stand)
    sys.path.insert(0, REF)
    try:
        _REF = (importlib.import_module("stage2_cINN.AE.modules.vgg16"), importlib.import_module("stage2_cINN.AE.modules.LPIPS"))
    finally:
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        purge()
    return _REF


def ref_vgg():
    return ref_modules()[0].vgg16(pretrained=True, requires_grad=False).eval()


def ref_lpips():
    mod = ref_modules()[1]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vgg.pth")
        vc.save_lin_file(path, SEED_LIN)
        mod.get_ckpt_path = lambda name, root=None, check=False: path     # no download, no cache directory
        return mod.LPIPS().eval()


def pack(meta, **arrays):
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def _gate(rel):
    return {"measured": rel, "floored": bool(rel < 1e-7), "gate_rel": GATE_FLOOR if rel < 1e-7 else 10 * rel}


def tap_stats(taps):
    return {n: {"shape": list(t.shape), "mean": float(t.double().mean()), "l2": float(t.double().norm())} for n, t in zip(vc.TAPS, taps)}


def make_taps(name, shape, seed):
    model = ref_vgg()
    x = vc.randn(seed, shape)
    with torch.no_grad():
        taps = model(x)
    meta = {"fixture": name, "weights": {"seed": SEED_W}, "input": {"seed": seed, "shape": list(shape), "generator": "i3d_units_common.randn"},
            "state_dict": [[k, list(v.shape)] for k, v in model.state_dict().items()], "taps": tap_stats(taps)}
    return pack(meta, **{n: t.numpy() for n, t in zip(vc.TAPS, taps)})


def diversity_input(frames, align_corners, dtype):
    """metrics/Diversity/VGG.py:29, 36 with the kornia calls written out: (x + 1) / 2, Normalize(ImageNet), Resize((224, 224))."""
    x = (frames.to(dtype) + 1) / 2
    mean = torch.tensor(vc.IMAGENET_MEAN).to(dtype).view(1, 3, 1, 1)
    std = torch.tensor(vc.IMAGENET_STD).to(dtype).view(1, 3, 1, 1)
    return F.interpolate((x - mean) / std, size=(224, 224), mode="bilinear", align_corners=align_corners)


def make_224(seed=51):
    model = ref_vgg()
    frame = torch.from_numpy(vc.clips(seed, 1, 1, 20, 24, signed=True))[0]
    arrays, stats = {}, {}
    for ac in (False, True):
        with torch.no_grad():
            taps = model(diversity_input(frame, ac, torch.float32))
        arrays[f"relu5_3_ac{int(ac)}"] = taps[4].numpy()
        stats[f"ac{int(ac)}"] = tap_stats(taps)
    meta = {"fixture": "vgg_224", "weights": {"seed": SEED_W}, "frame": {"seed": seed, "n": 1, "t": 1, "h": 20, "w": 24, "signed": True},
            "taps": stats, "note": "relu5_3_ac<align_corners>: vgg16(F.interpolate(normalize((x + 1) / 2), (224, 224), bilinear, align_corners))"}
    return pack(meta, **arrays)


def make_lpips(seed=61, n=12):
    arrays, sizes = {}, {}
    for tag, (h, w) in (("32x32", (32, 32)), ("24x40", (24, 40))):
        a = torch.from_numpy(vc.clips(seed, n, 1, h, w, signed=True))[:, 0]
        b = torch.from_numpy(vc.clips(seed + 1, n, 1, h, w, signed=True))[:, 0]
        b = (0.7 * a + 0.3 * b).contiguous()            # a perturbed copy, as a generated frame is of its real one
        with torch.no_grad():
            v32 = ref_lpips()(a, b).flatten().numpy().astype(np.float32)
            v64 = ref_lpips().double()(a.double(), b.double()).flatten().numpy()
        s32, s64 = vc.lpips_score_rule(v32), vc.lpips_score_rule(v64)
        rel_img = float(np.max(np.abs(v32.astype(np.float64) - v64) / np.abs(v64)))
        rel = abs(s32 - s64) / abs(s64)
        arrays[f"lpips32_{tag}"], arrays[f"lpips64_{tag}"] = v32, v64
        sizes[tag] = {"h": h, "w": w, "score_fp32": s32, "score_fp64": s64, "ref_fp32_vs_fp64_rel": rel, "gate": _gate(rel),
                      "per_image_ref_fp32_vs_fp64_rel": rel_img, "per_image_gate": _gate(rel_img)}
        seed += 2
    model = ref_lpips()
    meta = {"fixture": "vgg_lpips", "weights": {"seed": SEED_W, "lin_seed": SEED_LIN}, "n": n, "first_seed": 61, "sizes": sizes,
            "state_dict": [[k, list(v.shape)] for k, v in model.state_dict().items()],
            "note": "image i of a size: a = clips(seed, n, 1, h, w)[:, 0], b = 0.7 a + 0.3 clips(seed + 1, ...)[:, 0]; seeds 61/62 at 32x32, 63/64 at "
                    "24x40.  score_*: the CLI rule (mean over floor(n / 10) batch means)"}
    return pack(meta, **arrays)


def make_diversity(seed=71, N=2, R=3, T=2, S=16):
    videos = torch.from_numpy(vc.clips(seed, N * R, T, S, S, signed=True)).reshape(N, R, T, 3, S, S)

    def run(model, dtype):
        div = []
        with torch.no_grad():
            for video in videos:
                fmap = model(diversity_input(video.reshape(-1, 3, S, S), False, dtype))
                div += vc.pair_mean(fmap, R, T)
        return np.asarray(div, dtype=np.float64)
    d32, d64 = run(ref_vgg(), torch.float32), run(ref_vgg().double(), torch.float64)
    v32, v64 = float(d32.mean()), float(d64.mean())
    rel = abs(v32 - v64) / abs(v64)
    meta = {"fixture": "vgg_diversity", "weights": {"seed": SEED_W}, "clips": {"seed": seed, "n": N, "r": R, "t": T, "h": S, "w": S, "signed": True},
            "diversity_fp32": v32, "diversity_fp64": v64, "ref_fp32_vs_fp64_rel": rel, "gate": _gate(rel), "align_corners": False,
            "note": "video [n, r] is row n * R + r of clips(seed, N * R, T, ...).  terms: the N R (R - 1) 5 values of the reference's loop order"}
    return pack(meta, terms32=d32, terms64=d64, diversity=np.asarray([v32, v64]))


JOBS = {
    "taps": lambda: {"vgg_taps_16": make_taps("vgg_taps_16", (2, 3, 16, 16), 43), "vgg_taps_odd": make_taps("vgg_taps_odd", (1, 3, 35, 29), 44)},
    "big": lambda: {"vgg_224": make_224()},
    "lpips": lambda: {"vgg_lpips": make_lpips()},
    "diversity": lambda: {"vgg_diversity": make_diversity()},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="taps,big,lpips,diversity")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
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
                            worst = max(worst, float(np.max(np.abs(old[k].astype(np.float64) - arrays[k].astype(np.float64)))))
                print(f"{name}: max-abs difference {worst}")
            else:
                np.savez_compressed(path, **arrays)
                print(f"wrote {path} ({os.path.getsize(path)} bytes)", flush=True)


if __name__ == "__main__":
    main()
