"""Digests of the motion encoder and the conditioning embedder for A/B runs of changes to their host code: for every case of
tests/encoder_cfgs.py one sha256 over ``mu | logvar`` with the answer of ``i2v_encoder3d_workspace_bytes``, and for the five shapes of
tests/test_gpu_encoder_configs.py::test_embedder_shapes plus 64 x 64 with B = 64 of each norm one sha256 over the embedding with the
answer of ``i2v_embedder_workspace_bytes``.  Two builds of the library compute the same function iff the two outputs are equal, e.g.

    python tools/enc_bits.py > a.txt;  I2V_LIB_PATH=<other build, relative to the repository> python tools/enc_bits.py > b.txt

The statistics kernels accumulate fp64 sums with atomics, so a digest may differ between two runs of ONE build: run one build twice
first and compare only the lines that were stable.  The ``size`` lines have no such freedom.  The digests depend on the toolchain, so
they are compared between builds on one machine, never stored."""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "image2video-synthesis-using-cinns_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402

import encoder_cfgs as ec      # noqa: E402
import i2v_native              # noqa: E402
import i2v_synth as synth      # noqa: E402

EMBEDDER_SHAPES = (("in", 64, 128, 2), ("bn", 128, 64, 1), ("in", 256, 256, 1), ("bn", 64, 64, 5), ("bn", 256, 64, 3),
                   ("in", 64, 64, 64), ("bn", 64, 64, 64))


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def sha(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


def main():
    torch.set_grad_enabled(False)
    L = i2v_native.lib()
    for name, case in ec.CASES.items():
        a = case["synth"]
        h = i2v_native.NativeEncoder3D(a["z_dim"], a["channels"], a["stride_s"], case["stride_t"])
        h.load(T(synth.encoder3d_state_dict(**a)))
        x = (2 * torch.rand(*case["x_shape"], generator=torch.Generator().manual_seed(case["x_seed"])) - 1).cuda()
        B, _, frames, H, W = x.shape
        print(f"encoder size {name} {L.i2v_encoder3d_workspace_bytes(h._h, B, frames, H, W)}", flush=True)
        _, mu, logvar = h.forward(x)
        print(f"encoder digest {name} {sha(mu, logvar)}", flush=True)
    for norm, H, W, B in EMBEDDER_SHAPES:
        e = i2v_native.NativeEmbedder(64, norm == "bn")
        e.load(T(synth.embedder_state_dict(seed=3, z_dim=64, norm=norm)))
        x = (2 * torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(9)) - 1).cuda()
        print(f"embedder {norm} size {H}x{W} B={B} {L.i2v_embedder_workspace_bytes(e._h, B, H, W)}", flush=True)
        print(f"embedder {norm} digest {H}x{W} B={B} {sha(e.forward(x))}", flush=True)


if __name__ == "__main__":
    main()
