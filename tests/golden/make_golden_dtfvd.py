"""Writes tests/golden/dtfvd_*.npz from the REFERENCE's own ``metrics.DTFVD.ID3``, ``ID3_32`` and ``DTFVD_Score`` (CPU, torch + scipy).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_dtfvd.py [--only i3d,repeat,shapes,end2end,diversity] [--check]

It imports the reference modules, fills ``InceptionI3D(18, 1)`` from the seeded synthesiser of tests/dtfvd_common.py (the weights are
never committed), runs it on the CPU and stores inputs where they are small, results and bring-up statistics -- never weights or
reference text.  ``DTFVD_Score`` imports ``kornia`` and never uses it: an empty stand-in module is put into ``sys.modules`` while the
reference is imported, here only.  ``metrics.Diversity.I3D`` is NOT imported (it pulls in TensorFlow): the diversity expectation is the
reference's ``embedding_I3D`` output put through its pair formula in numpy float64 (``dtfvd_common.pair_diversity``).
``--check`` regenerates into memory and prints the max-abs difference to the committed files (expected: 0).

Fixtures:
  dtfvd_i3d16_t16 / _t9 / _t24, dtfvd_i3d32_t32 / _t40   get_representation of the resized clip (no de-normalisation), per end-point
                                                         (shape, mean, L2), the state_dict key list
  dtfvd_repeat      calculate_FVD's input rule (resize, repeat x 3, first 16 frames) -> get_activations rows, T_in = 6 and 20; for
                    T_in = 20 embedding_I3D (plain truncation) gives the same rows, which is asserted here
  dtfvd_shapes      end-point shapes at 224 x 224 for T in {16, 9, 24, 32, 40}, both lengths (None where the reference raises)
  dtfvd_end2end     two sets of 24 clips: activations in fp32 and with the module in .double(), the distance by the package's eigh
                    formulation on both, by the reference's sqrtm formulation on the fp32 ones, and the relative differences
  dtfvd_diversity   embedding_I3D of [N = 3, R = 4] clips, fp32 and .double(), and the pair mean of both
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
REF = os.environ.get("I2V_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
import dtfvd_common as dc  # noqa: E402

NUM_CLASSES = 18   # DTFVD_Score.load_model: InceptionI3D(18, 1)
GATE_FLOOR = 1e-6


def _import_from(root, names, stand_ins=()):
    """Import ``metrics.*`` from one tree (the reference and the package use the same import path)."""
    for k in [k for k in sys.modules if k == "metrics" or k.startswith("metrics.")]:
        del sys.modules[k]
    added = [n for n in stand_ins if n not in sys.modules]
    for n in added:
        sys.modules[n] = types.ModuleType(n)
    sys.path.insert(0, root)
    try:
        return [importlib.import_module(n) for n in names]
    finally:
        sys.path.remove(root)
        for n in added:
            del sys.modules[n]
        for k in [k for k in sys.modules if k == "metrics" or k.startswith("metrics.")]:
            del sys.modules[k]


_REF = None


def ref_modules():
    global _REF
    if _REF is None:
        _REF = _import_from(REF, ("metrics.DTFVD.ID3", "metrics.DTFVD.ID3_32", "metrics.DTFVD.DTFVD_Score"), stand_ins=("kornia",))
    return _REF


def package_frechet():
    (m,) = _import_from(PKG, ("metrics.PyTorch_FVD.FVD_logging",))
    return m.calculate_frechet_distance


def ref_model(length, seed):
    id3, id3_32, _ = ref_modules()
    model = (id3_32 if length == 32 else id3).InceptionI3D(NUM_CLASSES, 1)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in dc.dti3d_state_dict(seed, NUM_CLASSES).items()}, strict=True)
    model.eval()
    return model


def resize(clips):
    """The first statement of every DTFVD_Score entry point: [N, T, 3, H, W] -> 224 x 224, bilinear, align_corners=True; no denorm."""
    return F.interpolate(clips.reshape(-1, *clips.shape[2:]), mode='bilinear', size=(224, 224), align_corners=True).reshape(*clips.shape[:2], 3, 224,
                                                                                                                               224)


def run_with_endpoints(model, x):
    """get_representation with (shape, mean, L2) of every layer's output; (None, stats) when the reference raises (AvgPool on too few steps)."""
    stats, hooks = {}, []
    for name, layer in model.layers.items():
        if name in ("Dropout_5", "logits"):
            continue

        def hook(_m, _i, out, name=name):
            o = out.detach().double()
            stats[name] = (list(out.shape), float(o.mean()), float(o.norm()))
        hooks.append(layer.register_forward_hook(hook))
    try:
        with torch.no_grad():
            rep = model.get_representation(x)
    except RuntimeError:
        rep = None
    for h in hooks:
        h.remove()
    return rep, stats


def pack(meta, **arrays):
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def make_i3d(name, length, B, T, S, seed_w, seed_c):
    model = ref_model(length, seed_w)
    clip = dc.clips(seed_c, B, T, S, S, signed=True)
    rep, stats = run_with_endpoints(model, resize(torch.from_numpy(clip)).permute(0, 2, 1, 3, 4))
    meta = {"fixture": name, "length": length, "weights": {"seed": seed_w, "num_classes": NUM_CLASSES},
            "clips": {"seed": seed_c, "n": B, "t": T, "h": S, "w": S, "signed": True},
            "state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()],
            "endpoints": {k: {"shape": v[0], "mean": v[1], "l2": v[2]} for k, v in stats.items()}}
    arrays = {"features": rep.numpy()}
    if clip.nbytes <= 256 * 1024:
        arrays["clips"] = clip
    return pack(meta, **arrays)


def make_repeat(seed_w=7, seed_c=8, B=2, S=32):
    _, _, score = ref_modules()
    model = ref_model(16, seed_w)
    arrays, cases = {}, []
    for i, t_in in enumerate((6, 20)):
        clip = torch.from_numpy(dc.clips(seed_c + i, B, t_in, S, S, signed=True))
        data = resize(clip).repeat(1, 3, 1, 1, 1)[:, :16]                      # calculate_FVD :173-176
        rows = score.get_activations(data, model, B, False)
        if t_in >= 16:
            assert np.array_equal(rows, score.embedding_I3D(model, clip, B, False))   # plain truncation is the same rule
        arrays[f"rows_t{t_in}"] = rows.astype(np.float32)
        cases.append({"seed": seed_c + i, "n": B, "t": t_in, "h": S, "w": S, "signed": True})
    meta = {"fixture": "dtfvd_repeat", "length": 16, "weights": {"seed": seed_w, "num_classes": NUM_CLASSES}, "cases": cases,
            "note": "rows_t<T_in>: get_activations of resize(clip).repeat(1, 3, 1, 1, 1)[:, :16] (frame t reads source frame t % T_in), values "
                    "as they are (no de-normalisation)"}
    return pack(meta, **arrays)


def make_shapes():
    shapes = {}
    for length in (16, 32):
        model = ref_model(length, 1)
        per_t = {}
        for T in (16, 9, 24, 32, 40):
            _, stats = run_with_endpoints(model, torch.zeros(1, 3, T, 224, 224))
            per_t[str(T)] = {name: (stats[name][0] if name in stats else None) for name in model.layers if name not in ("Dropout_5", "logits")}
        shapes[str(length)] = per_t
    return pack({"fixture": "dtfvd_shapes", "H": 224, "W": 224, "shapes": shapes,
                 "note": "None: the reference raises at this end-point (fewer time steps than the average pool's kernel)"})


def _gate(rel):
    return {"measured": rel, "floored": bool(rel < 1e-7), "gate_rel": GATE_FLOOR if rel < 1e-7 else 10 * rel}


def make_end2end(seed_w=21, seed_gen=22, seed_orig=23, n=24, batch=8):
    _, _, score = ref_modules()
    model = ref_model(16, seed_w)
    gen = torch.from_numpy(dc.clips(seed_gen, n, 16, 32, 32, signed=True))
    orig = torch.from_numpy(dc.clips(seed_orig, n, 16, 32, 32, signed=False))

    def acts(m, dtype):   # calculate_FVD :173-180, one set at a time
        return [score.get_activations(resize(d.to(dtype)).repeat(1, 3, 1, 1, 1)[:, :16], m, batch, False) for d in (gen, orig)]
    g32, o32 = acts(model, torch.float32)
    g64, o64 = acts(model.double(), torch.float64)
    stats = lambda a: (a.mean(0), np.cov(a, rowvar=False))  # noqa: E731
    eigh = package_frechet()
    v32 = float(eigh(*stats(g32), *stats(o32)))
    v64 = float(eigh(*stats(g64), *stats(o64)))
    sq = score.calculate_frechet_distance(*stats(g32), *stats(o32))   # the reference's calculate_FVD value
    sq32, sq_imag = float(np.real(sq)), float(np.abs(np.imag(sq)))
    r_prec, r_form = abs(v32 - v64) / abs(v64), abs(v32 - sq32) / abs(sq32)
    meta = {"fixture": "dtfvd_end2end", "length": 16, "weights": {"seed": seed_w, "num_classes": NUM_CLASSES},
            "gen": {"seed": seed_gen, "n": n, "t": 16, "h": 32, "w": 32, "signed": True},
            "orig": {"seed": seed_orig, "n": n, "t": 16, "h": 32, "w": 32, "signed": False}, "batch_size": batch,
            "fvd_fp32_eigh": v32, "fvd_fp64_eigh": v64, "fvd_fp32_sqrtm": sq32, "fvd_fp32_sqrtm_imag": sq_imag,
            "ref_fp32_vs_fp64_rel": r_prec, "eigh_vs_sqrtm_rel": r_form, "gate": _gate(r_prec),
            "note": "24 clips, 1024 features: both covariances have rank 23.  fvd_fp32_sqrtm is the reference's own calculate_frechet_distance "
                    "(scipy sqrtm) on its fp32 activations, the *_eigh values the package's float64 eigenvalue formulation.  The GPU result may "
                    "deviate from the fp32 values by gate.gate_rel = 10 x ref_fp32_vs_fp64_rel (1e-6 if that figure is below 1e-7: "
                    "gate.floored); the CPU test gates eigh vs sqrtm at 10 x eigh_vs_sqrtm_rel"}
    return pack(meta, act_gen=g32.astype(np.float32), act_orig=o32.astype(np.float32), act_gen64=g64, act_orig64=o64,
                fvd=np.asarray([v32, v64, sq32], dtype=np.float64))


def make_diversity(seed_w=31, seed_c=32, N=3, R=4):
    _, _, score = ref_modules()
    model = ref_model(16, seed_w)
    seq1 = torch.from_numpy(dc.clips(seed_c, N * R, 16, 32, 32, signed=True)).reshape(N, R, 16, 3, 32, 32)

    def embed(m, dtype):   # compute_DTI3D_diversity :47-52
        return np.stack([score.embedding_I3D(m, seq, 20, False) for seq in seq1.to(dtype).transpose(0, 1)], 1)
    e32 = embed(model, torch.float32)
    e64 = embed(model.double(), torch.float64)
    d32, d64 = dc.pair_diversity(e32), dc.pair_diversity(e64)
    rel = abs(d32 - d64) / abs(d64)
    meta = {"fixture": "dtfvd_diversity", "length": 16, "weights": {"seed": seed_w, "num_classes": NUM_CLASSES},
            "clips": {"seed": seed_c, "n": N, "r": R, "t": 16, "h": 32, "w": 32, "signed": True},
            "diversity_fp32": d32, "diversity_fp64": d64, "ref_fp32_vs_fp64_rel": rel, "gate": _gate(rel),
            "note": "clip [n, r] is row n * R + r of clips(seed, N * R, ...).  diversity_*: the unscaled pair mean (the reference prints it x 1000) "
                    "over the R (R - 1) ordered pairs; the reference's loop hard-codes 5 realizations"}
    return pack(meta, embed=e32.astype(np.float32), embed64=e64, diversity=np.asarray([d32, d64], dtype=np.float64))


JOBS = {
    "i3d": lambda: {"dtfvd_i3d16_t16": make_i3d("dtfvd_i3d16_t16", 16, 2, 16, 64, 1, 2), "dtfvd_i3d16_t9": make_i3d("dtfvd_i3d16_t9", 16, 1, 9, 32, 3, 4),
                    "dtfvd_i3d16_t24": make_i3d("dtfvd_i3d16_t24", 16, 1, 24, 32, 5, 6),
                    "dtfvd_i3d32_t32": make_i3d("dtfvd_i3d32_t32", 32, 1, 32, 32, 9, 10),
                    "dtfvd_i3d32_t40": make_i3d("dtfvd_i3d32_t40", 32, 1, 40, 32, 11, 12)},
    "repeat": lambda: {"dtfvd_repeat": make_repeat()},
    "shapes": lambda: {"dtfvd_shapes": make_shapes()},
    "end2end": lambda: {"dtfvd_end2end": make_end2end()},
    "diversity": lambda: {"dtfvd_diversity": make_diversity()},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="i3d,repeat,shapes,end2end,diversity")
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
