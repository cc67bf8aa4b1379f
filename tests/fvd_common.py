"""Shared by the FVD tests and by tests/golden/make_golden_fvd.py: a numpy-only, seeded synthesiser of a full Kinetics-I3D
``state_dict`` (metrics/PyTorch_FVD/I3D.py of the reference: 57 conv units, 49 MB at 400 classes -- never committed, always
regenerated), a seeded procedural clip generator and the seeded activation sets of the Frechet fixture.

Everything here is a pure function of its arguments (``numpy.random.default_rng(seed)``), so the generator script and the tests see
the same bits."""
import json
import os

import numpy as np

MIXED = (("mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("mixed_5c", 832, (384, 192, 384, 48, 128, 128)))


def i3d_units(num_classes, in_channels=3):
    """[(name, cin, cout, kernel, has_bn, has_bias)] in the order of the reference module's state_dict."""
    u = [("conv3d_1a_7x7", in_channels, 64, 7, True, False), ("conv3d_2b_1x1", 64, 64, 1, True, False),
         ("conv3d_2c_3x3", 64, 192, 3, True, False)]
    for name, cin, o in MIXED:
        u += [(name + ".branch_0", cin, o[0], 1, True, False), (name + ".branch_1.0", cin, o[1], 1, True, False),
              (name + ".branch_1.1", o[1], o[2], 3, True, False), (name + ".branch_2.0", cin, o[3], 1, True, False),
              (name + ".branch_2.1", o[3], o[4], 3, True, False), (name + ".branch_3.1", cin, o[5], 1, True, False)]
    u.append(("conv3d_0c_1x1", 1024, num_classes, 1, False, True))
    return u


def i3d_state_dict_spec(num_classes, in_channels=3):
    """[(key, shape, dtype name)] of the reference state_dict, in its order."""
    spec = []
    for name, cin, cout, k, bn, bias in i3d_units(num_classes, in_channels):
        spec.append((name + ".conv3d.weight", (cout, cin, k, k, k), "float32"))
        if bias:
            spec.append((name + ".conv3d.bias", (cout,), "float32"))
        if bn:
            for s in ("weight", "bias", "running_mean", "running_var"):
                spec.append((name + ".batch3d." + s, (cout,), "float32"))
            spec.append((name + ".batch3d.num_batches_tracked", (), "int64"))
    return spec


def i3d_state_dict(seed, num_classes, in_channels=3):
    """Seeded weights: conv weights N(0, 2 / fan_in) (the ReLU-preserving scale, so activations stay O(1) through all 22 conv
    depths), BatchNorm weight in [0.8, 1.2], bias and running_mean N(0, 0.1^2), running_var in [0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, cin, cout, k, bn, bias in i3d_units(num_classes, in_channels):
        fan_in = cin * k ** 3
        sd[name + ".conv3d.weight"] = (rng.standard_normal((cout, cin, k, k, k)) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        if bias:
            sd[name + ".conv3d.bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        if bn:
            sd[name + ".batch3d.weight"] = rng.uniform(0.8, 1.2, cout).astype(np.float32)
            sd[name + ".batch3d.bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            sd[name + ".batch3d.running_mean"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            sd[name + ".batch3d.running_var"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
            sd[name + ".batch3d.num_batches_tracked"] = np.asarray(0, dtype=np.int64)
    return sd


def clips(seed, n, t, h, w, signed=True):
    """[n, t, 3, h, w] float32 procedural clips: per clip a few drifting sinusoidal gratings and a moving Gaussian blob per colour
    channel plus a little noise; values in [-1, 1] (signed) or [0, 1]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    tt = np.arange(t, dtype=np.float64)[:, None, None]
    out = np.empty((n, t, 3, h, w), dtype=np.float32)
    for i in range(n):
        for c in range(3):
            v = np.zeros((t, h, w))
            for _ in range(3):
                fx, fy, sp, ph, amp = rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-0.6, 0.6), rng.uniform(0, 6.28), rng.uniform(0.2, 0.5)
                v += amp * np.sin(fx * xx[None] + fy * yy[None] + sp * tt + ph)
            cx, cy, vx, vy, s = rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.06, 0.06), rng.uniform(-0.06, 0.06), rng.uniform(0.1, 0.4)
            v += np.exp(-((xx[None] - cx - vx * tt) ** 2 + (yy[None] - cy - vy * tt) ** 2) / (2 * s * s))
            v += 0.05 * rng.standard_normal((t, h, w))
            out[i, :, c] = np.tanh(v)
    if not signed:
        out = (out + 1.0) * 0.5
    return np.ascontiguousarray(out.astype(np.float32))


def frechet_sets(seed, n=1024, d=400):
    """Two float64 activation sets [n, d], correlated (a random mixing matrix with a decaying spectrum) and full rank."""
    rng = np.random.default_rng(seed)
    sets = []
    for k in range(2):
        mix = rng.standard_normal((d, d)) / np.sqrt(d) * (0.2 + np.linspace(1.5, 0.0, d))[None, :] + 0.3 * np.eye(d)
        mu = rng.standard_normal(d) * (0.5 + 0.5 * k)
        sets.append(rng.standard_normal((n, d)) @ mix + mu)
    return sets


def frechet_closed_form(seed, n=1024, d=400):
    """Equal covariance, shifted means: (mu1, sigma, mu2, sigma) and the exact distance ||mu1 - mu2||^2."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((d, d)) / np.sqrt(d)
    sigma = a @ a.T + 0.1 * np.eye(d)
    mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
    return mu1, sigma, mu2, float(((mu1 - mu2) ** 2).sum())


def load_fixture(name):
    from conftest import GOLDEN
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        arrays = {k: f[k] for k in f.files if k != "meta"}
        meta = json.loads(bytes(f["meta"]).decode())
    return arrays, meta
