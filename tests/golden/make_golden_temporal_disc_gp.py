"""Writes tests/golden/disc3d_gp_*.npz from the REFERENCE's own ``resnet3D.Discriminator`` (CPU, torch): the gradient penalty of
loss.py:35-43 and its gradient at every parameter through torch's double backward (``create_graph=True``, then ``.backward()``), with the
module in ``.double()`` and in fp32.

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_temporal_disc_gp.py [--check]

The module class, the configs, the seeds and the clips are those of make_golden_temporal_disc.py / temporal_disc_common.py:
  fixture A  ``CFG_A`` with the stored parameters of temporal_disc_a_params*.npz, the two REAL clips of 12 x 64 x 64
  fixture B  ``CFG_B``, ``synthetic_state(CFG_B, SEED_B)``, ``clips_b()`` [3, 3, 4, 32, 32]
  fixture C  ``CFG_C``, ``synthetic_state(CFG_C, SEED_B)``, ``clips_c()`` [3, 3, 4, 16, 16]
Per fixture X in (a, b, c), one training-mode forward (one power iteration), L_GP = mean_b |d mean(pred) / d x_b|^2, ``L_GP.backward()``:
  disc3d_gp_X.npz            l_gp (float64), l_gp_f32, ``dist.<key>``: per parameter the relative L2 distance of the fp32 run's gradient from
                             the float64 run's, ``none``: the names whose gradient autograd leaves at None (stored as zeros);
                             A only: ``sgd_pairs`` / ``sgd_pairs_f32`` [6, 2] = (L_d_t, L_GP) of six plain SGD steps (``SGD_LR``) of
                             ``(L_d_t + 10 L_GP).backward()`` on both clip sets in float64 and in fp32
  disc3d_gp_X_grads{i}.npz   every parameter's penalty gradient of the float64 run, rounded to fp32, split below 1 MiB
Results only, never text."""
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
sys.path.insert(0, HERE)
import temporal_disc_common as tc  # noqa: E402
from make_golden_temporal_disc import ref_class, split  # noqa: E402

W_GP = 10.0


def penalty(pred, x):
    """loss.py:35-43 restated: the graph of the input gradient is kept, so that the penalty can be differentiated again"""
    g = torch.autograd.grad(pred.mean(), x, create_graph=True)[0]
    return g.pow(2).reshape(x.size(0), -1).sum(1).mean()


def penalty_grads(net, x):
    net.zero_grad()
    x = x.clone().requires_grad_(True)
    pred, _ = net(x)
    l_gp = penalty(pred, x)
    l_gp.backward()
    return float(l_gp.detach()), {k: None if p.grad is None else p.grad.detach().double().numpy().copy() for k, p in net.named_parameters()}


def one_fixture(name, base, x):
    """base: the module in fp32, as constructed"""
    l64, g64 = penalty_grads(copy.deepcopy(base).double().train(), x.double())
    l32, g32 = penalty_grads(copy.deepcopy(base).float().train(), x.float())
    main = {"l_gp": np.float64(l64), "l_gp_f32": np.float64(l32)}
    none = [k for k, v in g64.items() if v is None]
    assert none == [k for k, v in g32.items() if v is None]
    main["none"] = np.frombuffer(json.dumps(none).encode(), dtype=np.uint8)
    grads = {}
    for k, v in g64.items():
        if v is None:
            shape = dict(base.named_parameters())[k].shape
            grads[k] = np.zeros(tuple(shape), dtype=np.float32)
            main["dist." + k] = np.float64(0.0)
        else:
            grads[k] = v.astype(np.float32)
            main["dist." + k] = np.float64(np.linalg.norm((g32[k] - v).ravel()) / max(np.linalg.norm(v.ravel()), 1e-300))
    files = split(f"disc3d_gp_{name}_grads", grads)
    return main, files


def sgd_pairs(base, fake, real, dt):
    net = copy.deepcopy(base).to(dt).train()
    out = []
    for _ in range(tc.SGD_STEPS):
        net.zero_grad()
        r = real.to(dt).clone().requires_grad_(True)
        pred_f, _ = net(fake.to(dt))
        pred_r, _ = net(r)
        l_d = tc.hinge_disc(pred_f, pred_r)
        l_gp = penalty(pred_r, r)
        (l_d + W_GP * l_gp).backward()
        with torch.no_grad():
            for p in net.parameters():
                if p.grad is not None:
                    p -= tc.SGD_LR * p.grad
        out.append([float(l_d.detach()), float(l_gp.detach())])
    return np.array(out, dtype=np.float64)


def load(pattern):
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, pattern))):
        with np.load(path) as a:
            out.update({k: a[k] for k in a.files})
    return out


def make(cls):
    files = {}
    base = cls(dict(tc.CFG_A))
    base.load_state_dict({k: torch.from_numpy(v) for k, v in load("temporal_disc_a_params*.npz").items()})
    fake, real = tc.clips_a()
    main, f = one_fixture("a", base, real)
    files.update(f)
    main["sgd_pairs"] = sgd_pairs(base, fake, real, torch.float64)
    main["sgd_pairs_f32"] = sgd_pairs(base, fake, real, torch.float32)
    files["disc3d_gp_a.npz"] = main
    for name, cfg, clips in (("b", tc.CFG_B, tc.clips_b), ("c", tc.CFG_C, tc.clips_c)):
        base = cls(dict(cfg))
        base.load_state_dict(tc.synthetic_state(cfg, tc.SEED_B))
        main, f = one_fixture(name, base, clips())
        files.update(f)
        files[f"disc3d_gp_{name}.npz"] = main
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    files = make(ref_class())
    if not args.check:
        for old in glob.glob(os.path.join(HERE, "disc3d_gp_*.npz")):
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
