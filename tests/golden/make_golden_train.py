#!/usr/bin/env python
"""Generate the gradient fixture ``flow_grad_ctrl_h128.npz`` (+ ``flow_grad_ctrl_h128_block1.npz``) FROM THE REFERENCE'S OWN
MODULES AND AUTOGRAD.

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    python tests/golden/make_golden_train.py

Same conventions as ``make_golden.py``: it imports ``stage2_cINN.modules.flow_blocks`` from the reference (torch-only, CPU),
loads deterministic synthetic weights from ``i2v_synth`` and stores only the synthesiser arguments, the inputs and the
results -- never weights or reference text.  One configuration: ``ConditionalFlow(64, 94, hidden_dim=128, hidden_depth=2,
n_flows=2, control=True)`` (block 0 in mode 'normal', block 1 in mode 'cond': both first-layer shapes), B = 6, loss
``mean(0.5 ||z~||^2) - mean(logdet)``; stored: z~, logdet, the loss, d_x, d_embed and the gradient of every parameter.

The 0.41 M fp32 gradients are incompressible (1.6 MB) and no file in this repository may exceed 1 MiB, so the ONE run is
written as two files: ``flow_grad_ctrl_h128.npz`` (inputs, outputs, d_x, d_embed, gradients of block 0) and
``flow_grad_ctrl_h128_block1.npz`` (gradients of block 1).  ``load()`` below puts them together again; the tests use it.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("I2V_REFERENCE", "/root/reference")

spec = importlib.util.spec_from_file_location(
    "i2v_synth", os.path.join(REPO, "image2video-synthesis-using-cinns_amd", "i2v_synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def main():
    sys.path.insert(0, REF)
    from stage2_cINN.modules import flow_blocks as ref_fb
    args = dict(seed=7, n_flows=2, embedding_dim=94, hidden_dim=128, control=True)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.flow_state_dict(**args).items()}
    flow = ref_fb.ConditionalFlow(64, 94, 128, 2, 2, conditioning_option="None", control=True)
    flow.load_state_dict(sd)
    x = rnd(21, 6, 64).requires_grad_(True)
    embed = rnd(22, 6, 94).requires_grad_(True)
    zt, logdet = flow(x, embed)
    loss = (0.5 * zt.reshape(6, -1).pow(2).sum(1)).mean() - logdet.mean()
    loss.backward()
    arrays = {"x": x.detach(), "embed": embed.detach(), "zt": zt.detach().reshape(6, -1), "logdet": logdet.detach(),
              "loss": loss.detach(), "d_x": x.grad, "d_embed": embed.grad}
    for k, p in flow.named_parameters():
        assert p.grad is not None and float(p.grad.norm()) > 0, k
        arrays["grad." + k] = p.grad
    arrays = {k: v.numpy() for k, v in arrays.items()}
    meta = dict(synth=args, hidden_depth=2, batch=6, loss="mean(0.5*sum(zt^2)) - mean(logdet)")
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    parts = {PARTS[1]: {k: v for k, v in arrays.items() if k.startswith("grad.sub_layers.1.")}}
    parts[PARTS[0]] = {k: v for k, v in arrays.items() if k not in parts[PARTS[1]]}
    for name, part in parts.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 2 ** 20, name
        print(f"{name}  {os.path.getsize(path) / 1e3:.0f} kB, {len(part)} arrays")


PARTS = ("flow_grad_ctrl_h128.npz", "flow_grad_ctrl_h128_block1.npz")


def load(golden_dir=HERE):
    """{name: array} of the whole fixture (both files)."""
    out = {}
    for name in PARTS:
        with np.load(os.path.join(golden_dir, name)) as f:
            out.update({k: f[k] for k in f.files})
    return out


if __name__ == "__main__":
    main()
