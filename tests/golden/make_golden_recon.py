"""Writes tests/golden/recon.npz from the REFERENCE's own ``stage1_VAE.modules.loss`` functions ``KL``, ``fmap_loss`` and ``hinge_loss`` (CPU).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_recon.py [--check]

The reference module imports ``pytorch_lightning.metrics.functional`` (ssim, psnr), ``wandb`` and its LPIPS module at the top; none of the
three functions uses them.  They are replaced by empty stand-in modules in ``sys.modules`` for the duration of the import, here only, as
make_golden_vgg.py does for torchvision.  Inputs are regenerated from their seeds (``inputs`` below); the fixture stores results only --
no weights, no reference text.  PSNR and SSIM have no fixture: the reference holds no code of its own for them and the library is not
installed; tests/recon_common.py states their formulas."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("I2V_REFERENCE", "/root/reference")

KL_CASES = ((1, 1), (3, 64), (130, 64))
FMAP_SHAPES = ((2, 8, 4, 6, 6), (2, 16, 2, 3, 3), (2, 1, 1, 2, 2))
HINGE_SHAPE = (5, 1, 3, 3)


def randn(seed, shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def inputs():
    """{name: tensors}, shared with tests/test_host_recon.py (which imports this function)."""
    out = {}
    for b, d in KL_CASES:
        out[f"kl_{b}x{d}"] = (randn(600 + b, (b, d)), 0.5 * randn(700 + b, (b, d)) - 0.3)
    out["fmap"] = ([randn(800 + i, s) for i, s in enumerate(FMAP_SHAPES)], [randn(850 + i, s) for i, s in enumerate(FMAP_SHAPES)])
    out["hinge"] = (randn(900, HINGE_SHAPE), randn(901, HINGE_SHAPE) + 0.5)
    return out


def ref_loss():
    """The reference's stage1_VAE.modules.loss, imported under the stand-ins."""
    names = ("pytorch_lightning", "pytorch_lightning.metrics", "pytorch_lightning.metrics.functional", "wandb", "stage2_cINN", "stage2_cINN.AE",
             "stage2_cINN.AE.modules", "stage2_cINN.AE.modules.LPIPS", "stage1_VAE", "stage1_VAE.modules", "stage1_VAE.modules.loss")
    saved = {k: sys.modules.pop(k, None) for k in names}
    stand = {k: types.ModuleType(k) for k in names[:8]}
    stand["pytorch_lightning.metrics.functional"].ssim = stand["pytorch_lightning.metrics.functional"].psnr = None
    stand["stage2_cINN.AE.modules.LPIPS"].LPIPS = None
    for k in ("stage2_cINN", "stage2_cINN.AE", "stage2_cINN.AE.modules", "pytorch_lightning", "pytorch_lightning.metrics"):
        stand[k].__path__ = []
    sys.modules.update(stand)
    sys.path.insert(0, REF)
    try:
        return importlib.import_module("stage1_VAE.modules.loss")
    finally:
        sys.path.remove(REF)
        for k in names:
            sys.modules.pop(k, None)
            if saved[k] is not None:
                sys.modules[k] = saved[k]


def build():
    mod, x = ref_loss(), inputs()
    arrays, meta = {}, {"fixture": "recon", "kl_cases": [list(c) for c in KL_CASES], "fmap_shapes": [list(s) for s in FMAP_SHAPES],
                        "hinge_shape": list(HINGE_SHAPE), "source": "stage1_VAE/modules/loss.py: KL :10-12, fmap_loss :14-21, hinge_loss :24-32"}
    for b, d in KL_CASES:
        mu, lv = x[f"kl_{b}x{d}"]
        arrays[f"kl_{b}x{d}"] = np.array([float(mod.KL(mu, lv)), float(mod.KL(mu.double(), lv.double()))])   # fp32, float64
    f1, f2 = x["fmap"]
    arrays["fmap"] = np.array([float(mod.fmap_loss(f1, f2, "L1")), float(mod.fmap_loss(f1, f2, "L2"))])
    fake, orig = x["hinge"]
    arrays["hinge"] = np.array([float(mod.hinge_loss(fake, orig, "disc")), float(mod.hinge_loss(fake, orig, "gen"))])
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    arrays, path = build(), os.path.join(HERE, "recon.npz")
    if args.check:
        old = np.load(path)
        for k, v in arrays.items():
            assert np.array_equal(old[k], v), k
        print("recon.npz matches")
        return
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)", flush=True)


if __name__ == "__main__":
    main()
