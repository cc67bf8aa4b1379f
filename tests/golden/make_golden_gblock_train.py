"""Writes tests/golden/gblock_train_{i}.npz (one set of keys, split by size) from the REFERENCE's own ``decoder.GeneratorBlock`` (CPU, torch autograd, the module in ``.double()``).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_gblock_train.py [--check]

``Spade.forward`` hard-codes ``.cuda()`` (normalization_layer.py:20); on a GPU-less host ``Tensor.cuda`` is made the identity before the
reference is imported, as make_golden.py does.

Per fixture of ``gblock_train_common.FIXTURES`` (parameters and inputs are seeded numpy draws that the tests regenerate, not stored), the
module in ``.train()`` mode and the loss sum(c out):
  {tag}.out, {tag}.dx, {tag}.dz           float64 output, gradients rounded to fp32
  {tag}.u.<conv>, {tag}.v.<conv>          weight_u / weight_v after the forward (float64)
  {tag}.g.<parameter key>                 every parameter gradient, rounded to fp32
  a.sgd_losses, a.sgd_losses_f32, a.sgd_scale   fixture A: the loss before each of six plain SGD steps (lr ``SGD_LR``) in float64 and in
                                          fp32, and sum |c out| per step, the scale the loss is compared on
``--check`` prints, and the run asserts, that the reference's own fp32 run stays inside the relative-L2 gate of 1e-4 on every tensor for
these seeds (``ZERO_GRADS`` on their own scale), and that its fp32 SGD losses stay within 1e-4 of the scale at this learning rate.  Results only, never text."""
import argparse
import os
import sys

import numpy as np
import torch

torch.Tensor.cuda = lambda self, *a, **k: self  # see the docstring

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gblock_train_common as gc  # noqa: E402


def ref_module(cfg, sd, dtype):
    sys.path.insert(0, os.environ["I2V_REFERENCE"])
    from stage1_VAE.modules.decoder import GeneratorBlock
    m = GeneratorBlock(cfg["n_in"], cfg["n_out"], cfg["spectral"], cfg["z_dim"])
    own = m.state_dict()
    assert set(own) == set(sd), (sorted(own), sorted(sd))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dtype).train()


def run(cfg, sd, dtype):
    x, z, img, c = (t.to(dtype) for t in gc.inputs(cfg))
    m = ref_module(cfg, sd, dtype)
    x.requires_grad_(True)
    z.requires_grad_(True)
    out = m(x, z, img)
    (c * out).sum().backward()
    res = {"out": out.detach(), "dx": x.grad, "dz": z.grad}
    for k, p in m.named_parameters():
        res["g." + k] = p.grad
    for k, b in m.named_buffers():
        res[("u." if k.endswith("_u") else "v.") + k.rsplit(".", 1)[0]] = b.detach().clone()
    return res


def sgd(cfg, sd, dtype):
    x, z, img, c = (t.to(dtype) for t in gc.inputs(cfg))
    m = ref_module(cfg, sd, dtype)
    losses, scale = [], []
    for _ in range(gc.SGD_STEPS):
        m.zero_grad()
        out = m(x, z, img)
        loss = (c * out).sum()
        loss.backward()
        losses.append(float(loss))
        scale.append(float((c * out).abs().sum()))
        with torch.no_grad():
            for p in m.parameters():
                p -= gc.SGD_LR * p.grad
    return np.array(losses), np.array(scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="print the distances, write nothing")
    args = ap.parse_args()
    store = {}
    for tag, cfg in gc.FIXTURES.items():
        sd = gc.synthetic_state(cfg)
        r64, r32 = run(cfg, sd, torch.float64), run(cfg, sd, torch.float32)
        scale = gc.block(sd, *gc.inputs(cfg)[:3], cfg, gc.inputs(cfg)[3])["scale"]
        worst = max((gc.rel(r32[k], r64[k], scale.get(k[2:])), k) for k in r64)
        print(f"fixture {tag}: the reference's fp32 run against its float64 run, worst rel-L2 {worst[0]:.2e} ({worst[1]})")
        assert worst[0] <= gc.TOL_L2 / 4, worst
        for k, v in r64.items():
            v = v.detach().numpy()
            store[f"{tag}.{k}"] = v if k == "out" or k[:2] in ("u.", "v.") else v.astype(np.float32)
        if tag == "a":
            l64, s64 = sgd(cfg, sd, torch.float64)
            l32, _ = sgd(cfg, sd, torch.float32)
            dist = np.abs(l32 - l64) / s64
            print(f"fixture a: SGD lr {gc.SGD_LR}: losses {l64}, |fp32 - float64| / scale {dist}")
            assert dist.max() <= gc.TOL_L2 / 4 and len(set(np.round(l64, 6))) == gc.SGD_STEPS
            store["a.sgd_losses"], store["a.sgd_losses_f32"], store["a.sgd_scale"] = l64, l32, s64
    if not args.check:
        # greedily into files of at most 700 KB of raw data, so that every committed file stays well below 1 MiB
        files, size = [{}], 0
        for k, v in store.items():
            if size + v.nbytes > 700_000 and files[-1]:
                files.append({})
                size = 0
            files[-1][k] = v
            size += v.nbytes
        for i, part in enumerate(files):
            path = os.path.join(HERE, f"gblock_train_{i}.npz")
            np.savez_compressed(path, **part)
            print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
