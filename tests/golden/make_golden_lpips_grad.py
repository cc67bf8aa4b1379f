"""Writes tests/golden/vgg_lpips_grad.npz: the gradients of the REFERENCE's own ``LPIPS`` module with respect to both arguments (CPU, torch,
the module in ``.double()``, the synthetic weights of tests/vgg_common.py).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_lpips_grad.py [--check]

The reference module is imported by ``make_golden_vgg.ref_lpips`` (stand-in ``torchvision`` / ``requests`` / ``tqdm``, the checkpoint path
rebound to a file written from the synthesiser: no code path reaches the network).  For every size of ``lpips_grad_common.GOLDEN``:
``out = LPIPS(x0, x1)`` on ``GOLDEN_N`` pairs regenerated from their seeds, ``(weights * out.flatten()).sum().backward()`` with the weights of
``lpips_grad_common.e2e_weights``; stored are the two gradients [N, 3, H, W] and the values [N] in float64 -- results, never weights or text."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import lpips_grad_common as lg  # noqa: E402
from make_golden_vgg import SEED_LIN, SEED_W, pack, ref_lpips  # noqa: E402


def make():
    assert (SEED_W, SEED_LIN) == (lg.SEED_W, lg.SEED_LIN)
    model = ref_lpips().double()
    arrays, sizes = {}, {}
    for tag, g in lg.GOLDEN.items():
        a, b, wts = lg.golden_frames(tag)
        x0, x1 = a.double().requires_grad_(True), b.double().requires_grad_(True)
        out = model(x0, x1)
        (wts * out.flatten()).sum().backward()
        arrays[f"grad_input_{tag}"], arrays[f"grad_target_{tag}"] = x0.grad.numpy(), x1.grad.numpy()
        arrays[f"lpips64_{tag}"] = out.detach().flatten().numpy()
        sizes[tag] = {"h": g["h"], "w": g["w"], "seed": g["seed"], "n": lg.GOLDEN_N, "weights": wts.tolist(),
                      "grad_input_l2": float(x0.grad.norm()), "grad_target_l2": float(x1.grad.norm())}
    meta = {"fixture": "vgg_lpips_grad", "weights": {"seed": SEED_W, "lin_seed": SEED_LIN}, "sizes": sizes, "gate_rel_l2": lg.TOL_L2,
            "note": "pair i of a size: a = clips(seed, n, 1, h, w)[:, 0], b = 0.7 a + 0.3 clips(seed + 1, ...)[:, 0]; "
                    "(weights * LPIPS(a, b).flatten()).sum().backward() with the reference module in .double()"}
    return pack(meta, **arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    arrays = make()
    path = os.path.join(HERE, "vgg_lpips_grad.npz")
    if args.check:
        with np.load(path) as old:
            worst = 0.0
            for k in arrays:
                if k == "meta":
                    assert json.loads(bytes(old[k]).decode()) == json.loads(bytes(arrays[k]).decode()), "meta differs"
                else:
                    worst = max(worst, float(np.max(np.abs(old[k] - arrays[k]))))
        print(f"vgg_lpips_grad: max-abs difference {worst}")
    else:
        np.savez_compressed(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
