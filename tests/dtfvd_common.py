"""Shared by the DTFVD tests and by tests/golden/make_golden_dtfvd.py: a numpy-only, seeded synthesiser of the dynamic-texture I3D
``state_dict`` (metrics/DTFVD/ID3.py and ID3_32.py of the reference: the same 58 conv units and the same keys for both lengths; about
49 MB -- never committed, always regenerated).  It follows the scheme of ``fvd_common.i3d_state_dict``; the clip generator and the
fixture loader are the ones of ``fvd_common``.

Everything here is a pure function of its arguments (``numpy.random.default_rng(seed)``), so the generator script and the tests see
the same bits."""
import numpy as np

from fvd_common import clips, load_fixture  # noqa: F401  (re-exported)

MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))


def dti3d_units(num_classes, in_channels=3):
    """[(name, cin, cout, kernel, has_bn, has_bias)] in the order of the reference module's state_dict."""
    u = [("Conv3d_1a_7x7", in_channels, 64, 7, True, False), ("Conv3d_2b_1x1", 64, 64, 1, True, False),
         ("Conv3d_2c_3x3", 64, 192, 3, True, False)]
    for name, cin, o in MIXED:
        u += [(name + ".b0", cin, o[0], 1, True, False), (name + ".b1a", cin, o[1], 1, True, False),
              (name + ".b1b", o[1], o[2], 3, True, False), (name + ".b2a", cin, o[3], 1, True, False),
              (name + ".b2b", o[3], o[4], 3, True, False), (name + ".b3b", cin, o[5], 1, True, False)]
    u.append(("logits", 1024, num_classes, 1, False, True))
    return u


def dti3d_state_dict_spec(num_classes, in_channels=3):
    """[(key, shape, dtype name)] of the reference state_dict, in its order."""
    spec = []
    for name, cin, cout, k, bn, bias in dti3d_units(num_classes, in_channels):
        spec.append((name + ".conv3d.weight", (cout, cin, k, k, k), "float32"))
        if bias:
            spec.append((name + ".conv3d.bias", (cout,), "float32"))
        if bn:
            for s in ("weight", "bias", "running_mean", "running_var"):
                spec.append((name + ".bn." + s, (cout,), "float32"))
            spec.append((name + ".bn.num_batches_tracked", (), "int64"))
    return spec


def dti3d_state_dict(seed, num_classes, in_channels=3):
    """Seeded weights: conv weights N(0, 2 / fan_in), BatchNorm weight in [0.8, 1.2], bias and running_mean N(0, 0.1^2), running_var in
    [0.5, 1.5] (with eps 1e-5 against 1e-3 a variance of 0.5 moves the scale by 1e-3 relative: far above the 1e-4 gate)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, cin, cout, k, bn, bias in dti3d_units(num_classes, in_channels):
        fan_in = cin * k ** 3
        sd[name + ".conv3d.weight"] = (rng.standard_normal((cout, cin, k, k, k)) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        if bias:
            sd[name + ".conv3d.bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        if bn:
            sd[name + ".bn.weight"] = rng.uniform(0.8, 1.2, cout).astype(np.float32)
            sd[name + ".bn.bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            sd[name + ".bn.running_mean"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            sd[name + ".bn.running_var"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
            sd[name + ".bn.num_batches_tracked"] = np.asarray(0, dtype=np.int64)
    return sd


def pair_diversity(embed):
    """The reference's pair loop (metrics/Diversity/I3D.py:53-57, with R in place of its hard-coded 5) on embeddings [N, R, D] in float64:
    the mean over all ordered pairs i != j of ``((embed[:, i] - embed[:, j]) ** 2).mean()``."""
    embed = np.asarray(embed, dtype=np.float64)
    r = embed.shape[1]
    div = [((embed[:, i] - embed[:, j]) ** 2).mean() for i in range(r) for j in range(r) if i != j]
    return float(np.mean(div))
