"""Writes tests/golden/patch_disc.npz and tests/golden/patch_disc_grads.npz from the REFERENCE's own ``NLayerDiscriminator`` (CPU, torch, the
module in ``.double()``), at ndf 16, n_layers 3 (``patch_disc_common.FIXTURE_CFG``).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_patch_disc.py [--check]

patch_disc.npz: the parameters and buffers as constructed under seed 4100 (fp32); one training-mode forward + backward of the 'disc'
hinge on the 4 fake / 4 real frames of ``patch_disc_common.train_inputs`` from ``initialized = 0`` -- both outputs, both input gradients and
the updated weight_u, weight_v, loc, scale in float64; the eval-mode outputs of the module in that state for ``EVAL_SHAPES``; and the losses
of six plain SGD steps (lr 1e-3) from the constructed state.  patch_disc_grads.npz: every parameter gradient of that training step,
rounded to fp32 (two files keep each below the size limit of a committed file).  Results and parameters only, never text."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import patch_disc_common as pc  # noqa: E402


def ref_module():
    sys.path.insert(0, os.environ["I2V_REFERENCE"])
    from stage1_VAE.modules.patch_disc import NLayerDiscriminator
    torch.manual_seed(pc.SEED_MODULE)
    return NLayerDiscriminator(dict(pc.FIXTURE_CFG))


def make():
    base = ref_module()
    main = {"p." + k: v.detach().numpy().copy() for k, v in base.state_dict().items()}
    fake, real = pc.train_inputs()

    net = copy.deepcopy(base).double().train()
    f64, r64 = fake.double().requires_grad_(True), real.double().requires_grad_(True)
    pred_f, pred_r = net(f64), net(r64)
    loss = pc.hinge_disc(pred_f, pred_r)
    loss.backward()
    main.update(train_pred_fake=pred_f.detach().numpy(), train_pred_real=pred_r.detach().numpy(), train_loss=np.float64(loss.item()),
                train_dx_fake=f64.grad.numpy(), train_dx_real=r64.grad.numpy())
    for k, v in net.state_dict().items():
        if k.endswith(("weight_u", "weight_v", "loc", "scale", "initialized")):
            main["after." + k] = v.detach().numpy().copy()
    grads = {k: p.grad.numpy().astype(np.float32) for k, p in net.named_parameters()}

    net.eval()
    with torch.no_grad():
        for tag in pc.EVAL_SHAPES:
            main["eval_" + tag] = net(pc.eval_inputs(tag).double()).numpy()

    losses = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        net = copy.deepcopy(base).to(dt).train()
        seq = []
        for _ in range(pc.SGD_STEPS):
            net.zero_grad()
            loss = pc.hinge_disc(net(fake.to(dt)), net(real.to(dt)))
            loss.backward()
            with torch.no_grad():
                for p in net.parameters():
                    p -= pc.SGD_LR * p.grad
            seq.append(float(loss.detach()))
        losses[name] = seq
    main["sgd_losses"] = np.array(losses["f64"], dtype=np.float64)
    main["sgd_losses_f32"] = np.array(losses["f32"], dtype=np.float64)
    meta = {"fixture": "patch_disc", "cfg": pc.FIXTURE_CFG, "seed_module": pc.SEED_MODULE, "seed_data": pc.SEED_DATA, "sgd_lr": pc.SGD_LR,
            "note": "p.*: state_dict as constructed; after.*: buffers / ActNorm parameters after the training forwards (no optimiser step)"}
    main["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return main, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    for name, arrays in zip(("patch_disc.npz", "patch_disc_grads.npz"), make()):
        path = os.path.join(HERE, name)
        if args.check:
            with np.load(path) as old:
                assert set(old.files) == set(arrays), set(old.files) ^ set(arrays)
                worst = max(float(np.max(np.abs(old[k].astype(np.float64) - np.asarray(arrays[k]).astype(np.float64)))) for k in arrays)
            print(f"{name}: worst |old - new| = {worst:.3e}")
            assert worst <= 1e-12, worst
        else:
            np.savez_compressed(path, **arrays)
            print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
