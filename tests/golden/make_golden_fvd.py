"""Writes tests/golden/fvd_*.npz from the REFERENCE's own ``metrics.PyTorch_FVD.I3D`` and ``FVD_logging`` (CPU, torch + scipy).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_fvd.py [--only i3d,shapes,frechet,end2end] [--check]

It imports the reference modules, fills ``I3D`` from the seeded synthesiser of tests/fvd_common.py (so the 49 MB of weights is never
committed), runs it on the CPU and stores inputs where they are small, results and bring-up statistics -- never weights or reference
text.  ``--check`` regenerates into memory and prints the max-abs difference to the committed files (expected: 0).

Fixtures:
  fvd_i3d_t16 / fvd_i3d_t9 / fvd_i3d_128   logits of preprocess(clip) -> I3D for three clip geometries, per end-point (shape, mean, L2)
  fvd_shapes                               end-point shapes at 224 x 224 for T in {16, 9, 10, 17}
  fvd_frechet                              calculate_frechet_distance on two seeded 1024 x 400 sets, and a closed-form pair
  fvd_end2end                              I3D(16) + calculate_FVD on two sets of 48 clips, fp32 and with the module in .double()
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
REF = os.environ.get("I2V_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
import fvd_common as fc  # noqa: E402

ENDPOINTS = ("conv3d_1a_7x7", "maxPool3d_2a_3x3", "conv3d_2b_1x1", "conv3d_2c_3x3", "maxPool3d_3a_3x3", "mixed_3b", "mixed_3c",
             "maxPool3d_4a_3x3", "mixed_4b", "mixed_4c", "mixed_4d", "mixed_4e", "mixed_4f", "maxPool3d_5a_2x2", "mixed_5b", "mixed_5c",
             "avg_pool", "conv3d_0c_1x1")


def _import_from(root, names):
    """Import ``metrics.PyTorch_FVD.*`` from one tree (the reference and the package use the same import path)."""
    for k in [k for k in sys.modules if k == "metrics" or k.startswith("metrics.")]:
        del sys.modules[k]
    sys.path.insert(0, root)
    try:
        return [importlib.import_module(n) for n in names]
    finally:
        sys.path.remove(root)
        for k in [k for k in sys.modules if k == "metrics" or k.startswith("metrics.")]:
            del sys.modules[k]


def ref_modules():
    return _import_from(REF, ("metrics.PyTorch_FVD.I3D", "metrics.PyTorch_FVD.FVD_logging"))


def ref_model(ref_i3d, seed, num_classes):
    model = ref_i3d.I3D(num_classes, "rgb")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in fc.i3d_state_dict(seed, num_classes).items()}
    model.load_state_dict(sd)
    model.eval()
    return model


def run_with_endpoints(model, x):
    stats, hooks = {}, []
    for name in ENDPOINTS:
        def hook(_m, _i, out, name=name):
            o = out.detach().double()
            stats[name] = (list(out.shape), float(o.mean()), float(o.norm()))
        hooks.append(getattr(model, name).register_forward_hook(hook))
    with torch.no_grad():
        logits = model(x)[1]
    for h in hooks:
        h.remove()
    return logits, stats


def pack(meta, **arrays):
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def make_i3d(name, B, T, S, seed_w, seed_c, num_classes=400):
    ref_i3d, ref_fvd = ref_modules()
    model = ref_model(ref_i3d, seed_w, num_classes)
    clip = fc.clips(seed_c, B, T, S, S, signed=True)
    x, _ = ref_fvd.preprocess(torch.from_numpy(clip), torch.from_numpy(clip[:1]))   # resize to 224 x 224, denorm (min < 0)
    logits, stats = run_with_endpoints(model, x.permute(0, 2, 1, 3, 4))
    meta = {"fixture": name, "weights": {"seed": seed_w, "num_classes": num_classes}, "clips": {"seed": seed_c, "n": B, "t": T, "h": S, "w": S,
                                                                                                 "signed": True},
            "state_dict": [[k, list(s), d] for k, s, d in ((k, tuple(v.shape), str(v.dtype).replace("torch.", ""))
                                                           for k, v in model.state_dict().items())],
            "endpoints": {k: {"shape": v[0], "mean": v[1], "l2": v[2]} for k, v in stats.items()}}
    arrays = {"logits": logits.numpy()}
    if clip.nbytes <= 256 * 1024:
        arrays["clips"] = clip
    return pack(meta, **arrays)


def make_shapes():
    ref_i3d, _ = ref_modules()
    model = ref_model(ref_i3d, 1, 400)
    shapes = {}
    for T in (16, 9, 10, 17):
        _, stats = run_with_endpoints(model, torch.zeros(1, 3, T, 224, 224))
        shapes[str(T)] = {k: v[0] for k, v in stats.items()}
    return pack({"fixture": "fvd_shapes", "H": 224, "W": 224, "shapes": shapes})


def package_frechet():
    (m,) = _import_from(PKG, ("metrics.PyTorch_FVD.FVD_logging",))
    return m.calculate_frechet_distance


def make_frechet(seed=11, seed_cf=12):
    _, ref_fvd = ref_modules()
    a1, a2 = fc.frechet_sets(seed)
    mu1, s1, mu2, s2 = a1.mean(0), np.cov(a1, rowvar=False), a2.mean(0), np.cov(a2, rowvar=False)
    ref = float(ref_fvd.calculate_frechet_distance(mu1, s1, mu2, s2))
    ours = float(package_frechet()(mu1, s1, mu2, s2))
    m1, sig, m2, exact = fc.frechet_closed_form(seed_cf)
    ref_cf = float(ref_fvd.calculate_frechet_distance(m1, sig, m2, sig))
    ours_cf = float(package_frechet()(m1, sig, m2, sig))
    meta = {"fixture": "fvd_frechet", "sets": {"seed": seed, "n": 1024, "d": 400}, "closed_form": {"seed": seed_cf, "n": 1024, "d": 400},
            "reference": ref, "eigh_vs_sqrtm_rel": abs(ours - ref) / abs(ref),
            "closed_form_exact": exact, "closed_form_reference": ref_cf, "closed_form_eigh_vs_sqrtm_abs": abs(ours_cf - ref_cf),
            "note": "eigh_vs_sqrtm_rel: |eigenvalue formulation - reference sqrtm formulation| / reference, both float64, measured on the CPU "
                    "when this file was made; the test gates at 10 x this figure"}
    return pack(meta, reference=np.asarray([ref, ref_cf, exact], dtype=np.float64))


def make_end2end(seed_w=21, seed_gen=22, seed_orig=23, n=48, batch=16):
    ref_i3d, ref_fvd = ref_modules()
    model = ref_model(ref_i3d, seed_w, 16)
    gen = torch.from_numpy(fc.clips(seed_gen, n, 16, 32, 32, signed=True))
    orig = torch.from_numpy(fc.clips(seed_orig, n, 16, 32, 32, signed=False))
    # the reference's get_activations allocates 400 columns whatever the model: run its two halves by hand for the activations,
    # then its own calculate_frechet_distance -- this is calculate_FVD line by line for a 16-class module
    def fvd(m, dtype):
        g, o = ref_fvd.preprocess(gen, orig)
        acts = []
        for data in (g, o):
            rows = []
            for i in range(n // batch):
                with torch.no_grad():
                    rows.append(m(data[i * batch:(i + 1) * batch].to(dtype).permute(0, 2, 1, 3, 4))[1].cpu().numpy().astype(np.float64))
            acts.append(np.concatenate(rows, 0))
        (a1, a2) = acts
        val = ref_fvd.calculate_frechet_distance(a1.mean(0), np.cov(a1, rowvar=False), a2.mean(0), np.cov(a2, rowvar=False))
        return float(val), a1, a2
    v32, g32, o32 = fvd(model, torch.float32)
    v64, _, _ = fvd(model.double(), torch.float64)
    meta = {"fixture": "fvd_end2end", "weights": {"seed": seed_w, "num_classes": 16},
            "gen": {"seed": seed_gen, "n": n, "t": 16, "h": 32, "w": 32, "signed": True},
            "orig": {"seed": seed_orig, "n": n, "t": 16, "h": 32, "w": 32, "signed": False}, "batch_size": batch,
            "fvd_fp32": v32, "fvd_fp64": v64, "ref_fp32_vs_fp64_rel": abs(v32 - v64) / abs(v64),
            "note": "the allowed relative deviation of the GPU result from fvd_fp32 is 10 x ref_fp32_vs_fp64_rel"}
    return pack(meta, act_gen=g32, act_orig=o32, fvd=np.asarray([v32, v64], dtype=np.float64))


JOBS = {
    "i3d": lambda: {"fvd_i3d_t16": make_i3d("fvd_i3d_t16", 2, 16, 64, 1, 2), "fvd_i3d_t9": make_i3d("fvd_i3d_t9", 1, 9, 32, 3, 4),
                    "fvd_i3d_128": make_i3d("fvd_i3d_128", 1, 16, 128, 5, 6)},
    "shapes": lambda: {"fvd_shapes": make_shapes()},
    "frechet": lambda: {"fvd_frechet": make_frechet()},
    "end2end": lambda: {"fvd_end2end": make_end2end()},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="i3d,shapes,frechet,end2end")
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
                print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
