"""Writes tests/golden/i3d_units.npz from the REFERENCE's own layer modules in ``.double()`` (CPU, torch): ``Unit3Dpy``,
``MaxPool3dTFPadding`` and ``Mixed`` of metrics/PyTorch_FVD/I3D.py, ``Unit3D``, ``MaxPool3dSamePadding`` and ``InceptionModule`` of
metrics/DTFVD/ID3.py.

Run once on the build machine (needs the reference checkout, ``I2V_REFERENCE``; never runs on the GPU machine):

    I2V_REFERENCE=/path/to/reference python tests/golden/make_golden_i3d_units.py [--check]

Every module is built as the reference network builds it, filled from the seeded synthesiser of tests/fvd_common.py /
tests/dtfvd_common.py (weights are never committed) and run on the seeded inputs of tests/i3d_units_common.py at that module's
``fixture_cases()`` -- the thinned list: batch 1 and small maps.  Only OUTPUTS are stored (float64): tests/test_host_i3d_units.py pins
the float64 oracles of i3d_units_common.py to them at 1e-12 relative.  ``--check`` regenerates into memory and prints the max-abs
difference to the committed file (expected: 0)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("I2V_REFERENCE")
sys.path.insert(0, os.path.join(REPO, "tests"))
import i3d_units_common as uc  # noqa: E402


def ref_modules():
    if not REF:
        raise SystemExit("set I2V_REFERENCE to the reference checkout")
    for k in [k for k in sys.modules if k == "metrics" or k.startswith("metrics.")]:
        del sys.modules[k]
    sys.path.insert(0, REF)
    try:
        return importlib.import_module("metrics.PyTorch_FVD.I3D"), importlib.import_module("metrics.DTFVD.ID3")
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "metrics" or k.startswith("metrics.")]:
            del sys.modules[k]


def _fill(module, variant, prefix):
    sd = uc.state_dict(variant)
    sub = {k[len(prefix) + 1:]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith(prefix + ".")}
    module.load_state_dict(sub, strict=True)
    return module.double().eval()


def ref_unit(mods, variant, unit):
    key, cin, cout, k, s, bn = uc.unit_spec(variant, unit)
    head = unit == uc.UNIT_HEAD
    if variant == "kin":
        m = mods[0].Unit3Dpy(cin, cout, kernel_size=(k, k, k), stride=(s, s, s), activation=None if head else "relu", use_bias=head, use_bn=not head)
    else:
        m = mods[1].Unit3D(in_channels=cin, output_channels=cout, kernel_size=[k, k, k], stride=(s, s, s), padding=0,
                           activation_fn=None if head else torch.nn.functional.relu, use_batch_norm=not head, use_bias=head)
    return _fill(m, variant, key)


def ref_mixed(mods, variant, block):
    name, cin, o = uc.fc.MIXED[uc.BLOCKS.index(block)]
    if variant == "kin":
        return _fill(mods[0].Mixed(cin, list(o)), variant, name)
    return _fill(mods[1].InceptionModule(cin, list(o), name), variant, name[0].upper() + name[1:])


def ref_pool(mods, variant, kernel, stride):
    if variant == "kin":
        return mods[0].MaxPool3dTFPadding(kernel_size=kernel, stride=stride, padding="SAME")
    return mods[1].MaxPool3dSamePadding(kernel_size=list(kernel), stride=stride, padding=0)


def make():
    mods = ref_modules()
    units, mixed, pools = uc.fixture_cases()
    arrays = {}
    with torch.no_grad():
        for c in units:
            arrays["unit/" + c["id"]] = ref_unit(mods, c["variant"], c["unit"])(uc.unit_input(c).double()).numpy()
        for c in mixed:
            x = uc.randn(c["seed"], (c["shape"][0], uc.fc.MIXED[uc.BLOCKS.index(c["block"])][1], *c["shape"][1:]))
            arrays["mixed/" + c["id"]] = ref_mixed(mods, c["variant"], c["block"])(x.double()).numpy()
        for c in pools:
            arrays["pool/" + c["id"]] = ref_pool(mods, c["variant"], c["kernel"], c["stride"])(uc.pool_input(c).double()).numpy()
    meta = {"fixture": "i3d_units", "weights": uc.WEIGHT_SEED, "classes": uc.CLASSES, "keys": sorted(arrays),
            "note": "float64 outputs of the reference's layer modules in .double() at i3d_units_common.fixture_cases(); inputs and weights are "
                    "regenerated from their seeds"}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    arrays = make()
    path = os.path.join(HERE, "i3d_units.npz")
    if args.check:
        worst = 0.0
        with np.load(path) as old:
            assert sorted(old.files) == sorted(arrays), "key list differs"
            for k in arrays:
                if k == "meta":
                    assert bytes(old[k]) == bytes(arrays[k]), "meta differs"
                else:
                    worst = max(worst, float(np.max(np.abs(old[k] - arrays[k]))))
        print(f"i3d_units: max-abs difference {worst}")
    else:
        np.savez_compressed(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)", flush=True)


if __name__ == "__main__":
    main()
