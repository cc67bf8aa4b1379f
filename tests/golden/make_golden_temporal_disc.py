"""Writes tests/golden/temporal_disc_*.npz from the REFERENCE's own ``resnet3D.Discriminator`` (CPU, torch, the module in ``.double()``).

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_temporal_disc.py [--check]

The reference starts its layers from ``inplanes = 64`` whatever ``channels[0]`` is, so it cannot run below a 64-wide stem.  The fixtures use
reduced widths; the module is therefore built through a subclass whose ``inplanes`` starts at ``channels[0]`` (a property that replaces the
first assignment) -- the one change, and none at the shipped widths.

Fixture A (``temporal_disc_common.CFG_A``, seed 5100; two fake and two real clips of 12 frames at 64 x 64):
  temporal_disc_a_params{i}.npz   the state dict as constructed (fp32), split so that every file stays below 1 MiB
  temporal_disc_a_grads{i}.npz    every parameter gradient of the training forward + 'disc' hinge backward, rounded to fp32
  temporal_disc_a_dx_{fake,real,gen}{clip}.npz   the input gradients of that step and of the generator loss, per clip, rounded to fp32
  temporal_disc_a.npz             both preds, the feature maps' checksums (sum, sum of squares) and layer 3's in full, the updated u and v,
                                  the generator loss of loss.py:127-135, the value of gradient_penalty, the eval-mode outputs at T = 12 and
                                  T = 5, the losses of six plain SGD steps (lr 1e-3) in float64 and in fp32
Fixture B (``CFG_B``; parameters from ``temporal_disc_common.synthetic_state``, which the tests regenerate; three clips of 4 frames at 32 x 32;
the loss is sum(pred * d_pred) + sum(fmap_i * d_fmap_i) with the seeded upstream gradients of ``upstream_b``):
  temporal_disc_b.npz             pred, the feature maps, the input gradient (float64); fixture C (B without the max pool at 16 x 16): forward
  temporal_disc_b_grads{i}.npz    every parameter gradient, rounded to fp32
Results and parameters only, never text."""
import argparse
import copy
import glob
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import temporal_disc_common as tc  # noqa: E402

LIMIT = 900 * 1024   # raw bytes per file: below 1 MiB with the archive's overhead


def ref_class():
    sys.path.insert(0, os.environ["I2V_REFERENCE"])
    from stage1_VAE.modules.resnet3D import Discriminator

    class FromStemWidth(Discriminator):
        def __init__(self, dic):
            self.__dict__["_c0"] = dic["channels"][0]
            super().__init__(dic)

        @property
        def inplanes(self):
            return self.__dict__["_inplanes"]

        @inplanes.setter
        def inplanes(self, value):
            self.__dict__["_inplanes"] = value if "_inplanes" in self.__dict__ else self.__dict__["_c0"]

    return FromStemWidth


def split(prefix, arrays):
    """{file name: {key: array}}: the arrays in order, a new file whenever the next one would pass LIMIT"""
    files, cur, size = {}, {}, 0
    for k, v in arrays.items():
        if cur and size + v.nbytes > LIMIT:
            files[f"{prefix}{len(files)}.npz"] = cur
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    files[f"{prefix}{len(files)}.npz"] = cur
    return files


def checksums(fmaps):
    return np.array([[float(f.detach().sum()), float(f.detach().pow(2).sum())] for f in fmaps], dtype=np.float64)


def make_a(cls):
    torch.manual_seed(tc.SEED_A)
    base = cls(dict(tc.CFG_A))
    files = split("temporal_disc_a_params", {k: v.detach().numpy().copy() for k, v in base.state_dict().items()})
    fake, real = tc.clips_a()
    main = {}

    net = copy.deepcopy(base).double().train()
    f64, r64 = fake.double().requires_grad_(True), real.double().requires_grad_(True)
    (pred_f, fm_f), (pred_r, fm_r) = net(f64), net(r64)
    loss = tc.hinge_disc(pred_f, pred_r)
    loss.backward()
    main.update(train_pred_fake=pred_f.detach().numpy(), train_pred_real=pred_r.detach().numpy(), train_loss=np.float64(loss.item()),
                train_fmaps_fake=checksums(fm_f), train_fmaps_real=checksums(fm_r), train_fmap3_fake=fm_f[3].detach().numpy(),
                train_fmap3_real=fm_r[3].detach().numpy())
    for k, v in net.state_dict().items():
        if k.endswith(("weight_u", "weight_v")):
            main["after." + k] = v.detach().numpy().copy()
    files.update(split("temporal_disc_a_grads", {k: p.grad.numpy().astype(np.float32) for k, p in net.named_parameters()}))
    for name, g in (("fake", f64.grad), ("real", r64.grad)):
        for i in range(2):
            files[f"temporal_disc_a_dx_{name}{i}.npz"] = {"dx": g[i].numpy().astype(np.float32)}

    net.eval()
    with torch.no_grad():
        for t in (12, 5):
            main[f"eval_t{t}"] = net(tc.clips_a_eval(t).double())[0].numpy()

    net = copy.deepcopy(base).double().train()
    f64 = fake.double().requires_grad_(True)
    (pred_f, fm_f), (pred_r, fm_r) = net(f64), net(real.double())
    coup = -pred_f.mean()
    fm = sum((a - b).abs().mean() for a, b in zip(fm_f, fm_r)) / 4
    l_temp = 1 * coup + 10 * fm
    l_temp.backward()
    main.update(gen_coup=np.float64(coup.item()), gen_fmap=np.float64(fm.item()), gen_loss=np.float64(l_temp.item()))
    for i in range(2):
        files[f"temporal_disc_a_dx_gen{i}.npz"] = {"dx": f64.grad[i].numpy().astype(np.float32)}

    net = copy.deepcopy(base).double().train()
    r64 = real.double().requires_grad_(True)
    pred, _ = net(r64)
    grad = torch.autograd.grad(pred.mean(), r64, create_graph=True)[0]
    main["gp_value"] = np.float64(grad.pow(2).reshape(2, -1).sum(1).mean().item())

    losses = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        net = copy.deepcopy(base).to(dt).train()
        seq = []
        for _ in range(tc.SGD_STEPS):
            net.zero_grad()
            loss = tc.hinge_disc(net(fake.to(dt))[0], net(real.to(dt))[0])
            loss.backward()
            with torch.no_grad():
                for p in net.parameters():
                    p -= tc.SGD_LR * p.grad
            seq.append(float(loss.detach()))
        losses[name] = seq
    main["sgd_losses"] = np.array(losses["f64"], dtype=np.float64)
    main["sgd_losses_f32"] = np.array(losses["f32"], dtype=np.float64)
    meta = {"fixture": "temporal_disc_a", "cfg": tc.CFG_A, "seed_module": tc.SEED_A, "seed_data": tc.SEED_A_DATA, "sgd_lr": tc.SGD_LR,
            "note": "after.*: u and v after the two training forwards (no optimiser step); the eval outputs are of that state"}
    main["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    files["temporal_disc_a.npz"] = main
    return files


def make_b(cls):
    files, main = {}, {}
    net = cls(dict(tc.CFG_B))
    net.load_state_dict(tc.synthetic_state(tc.CFG_B, tc.SEED_B))
    net = net.double().train()
    x = tc.clips_b().double().requires_grad_(True)
    d_pred, d_fmaps = tc.upstream_b()
    pred, fmaps = net(x)
    loss = (pred * d_pred.double()).sum() + sum((f * g.double()).sum() for f, g in zip(fmaps, d_fmaps))
    loss.backward()
    main.update(b_pred=pred.detach().numpy(), b_dx=x.grad.numpy(), **{f"b_fmap{i}": f.detach().numpy() for i, f in enumerate(fmaps)})
    for k, v in net.state_dict().items():
        if k.endswith(("weight_u", "weight_v")):
            main["b_after." + k] = v.detach().numpy().copy()
    files.update(split("temporal_disc_b_grads", {k: p.grad.numpy().astype(np.float32) for k, p in net.named_parameters()}))

    net = cls(dict(tc.CFG_C))
    net.load_state_dict(tc.synthetic_state(tc.CFG_C, tc.SEED_B))
    net = net.double().train()
    with torch.no_grad():
        pred, fmaps = net(tc.clips_c().double())
    main.update(c_pred=pred.numpy(), **{f"c_fmap{i}": f.numpy() for i, f in enumerate(fmaps)})
    files["temporal_disc_b.npz"] = main
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    cls = ref_class()
    files = dict(make_a(cls), **make_b(cls))
    if not args.check:
        for old in glob.glob(os.path.join(HERE, "temporal_disc_*.npz")):
            os.remove(old)
    for name, arrays in files.items():
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
            assert os.path.getsize(path) < 1 << 20, name


if __name__ == "__main__":
    main()
