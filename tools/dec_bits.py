"""Digests of the stage-1 decoder for A/B runs of host-code changes: one line per case with the workspace size, the kernel code every
3x3x3 conv ran (i2v_dec_get_layer_profile) and a sha256 over the output bytes -- the whole decoder in every matrix-core mode, the
prepare / cancel / realizations entry points, the stand-alone GeneratorBlock and norm layers, and one embedder forward (which shares the
normalisation helpers).  Two builds of the library compute the same function iff the two outputs are equal, e.g.

    python tools/dec_bits.py > a.txt;  I2V_LIB_PATH=<other build, relative to the repository> python tools/dec_bits.py > b.txt

The statistics kernels accumulate fp64 sums with atomics, so a digest may differ between two runs of ONE build: run one build twice
first and compare only the lines that were stable.  The digests depend on the toolchain, so they are compared between builds on one
machine, never stored."""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "image2video-synthesis-using-cinns_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402

import i2v_native              # noqa: E402
import i2v_synth as synth      # noqa: E402

ZD, B, SIZE = 64, 3, 64
MODES = (0, 1, 3, "auto")


def T(sd, prefix=""):
    return {k[len(prefix):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith(prefix)}


def sha(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.cpu().numpy().tobytes())
    return m.hexdigest()


def rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).cuda().contiguous()


def decoder(sd, nf, mma):
    d = i2v_native.NativeDecoder(nf, ZD, [2, 1], [2, 1], True, i2v_native.parse_mma(mma))   # 16 x 64 x 64 frames
    d.load(sd)
    d.set_profile(True)
    return d


def line(name, d, out, frames, K=1):
    codes = "".join(str(d.KERNEL_NAMES.index(r["kernel"])) for r in d.get_layer_profile())
    d.set_profile(True)   # (resets the totals for the next case on this handle)
    print(f"{name} ws={d.workspace_bytes(frames, SIZE, SIZE, K)} kernels={codes} {sha(out)}", flush=True)


def main():
    torch.set_grad_enabled(False)
    gen = torch.Generator().manual_seed(3)
    img, img2 = rand(gen, B, 3, SIZE, SIZE, scale=0.5), rand(gen, B, 3, SIZE, SIZE, scale=0.5)
    motion, motion6 = rand(gen, B, ZD), rand(gen, 6, ZD)
    sds = {nf: T(synth.decoder_state_dict(seed=5, channel_factor=nf, z_dim=ZD)) for nf in (8, 32)}
    for wino4 in (None, "2"):
        if wino4:
            os.environ["I2V_DEC_WINO4"] = wino4     # read at create
        for nf in (8, 32):
            for mma in MODES:
                d = decoder(sds[nf], nf, mma)
                line(f"dec nf={nf} mma={mma} wino4={wino4 or 'default'}", d, d.forward(img, motion), B)
        os.environ.pop("I2V_DEC_WINO4", None)
    d = decoder(sds[8], 8, 1)
    d.prepare(img)
    line("prepare + matching forward", d, d.forward(img, motion), B)
    d.prepare(img)
    line("prepare + forward on other frames", d, d.forward(img2, motion), B)
    d.prepare(img)
    i2v_native._check(i2v_native.lib().i2v_dec_prepare_cancel(d._h), "i2v_dec_prepare_cancel")
    line("prepare_cancel + forward", d, d.forward(img, motion), B)
    line("realizations 2 x 3", d, d.forward(img[:2], motion6, realizations=3), 2, 3)
    # stand-alone blocks: g_1 of a channel_factor 2 decoder (32 -> 16, learned shortcut), head_0 of a channel_factor 1 one (16 -> 16)
    blocks = {"learned 32->16": (T(synth.decoder_state_dict(seed=5, channel_factor=2, z_dim=ZD), "g_1."), 32, 16),
              "identity 16->16": (T(synth.decoder_state_dict(seed=5, channel_factor=1, z_dim=ZD), "head_0."), 16, 16)}
    z = rand(gen, B, ZD)
    for name, (sd, n_in, n_out) in blocks.items():
        x = rand(gen, B, n_in, 8, 16, 16)
        for mma in (0, 1):
            g = i2v_native.NativeGBlock(n_in, n_out, ZD, True, mma)
            g.load(sd)
            out = g.forward(x, z, img)
            print(f"gblock {name} mma={mma} status={g.status()} {sha(out)}", flush=True)
    sd = blocks["learned 32->16"][0]
    for kind, prefix, C, cond in (("spade", "norm_0.", 32, img), ("adain", "norm_1.", 16, z), ("norm3d", "norm_s.", 32, None)):
        n = i2v_native.NativeNorm(kind, C, ZD, mma=0)
        n.load(T(sd, prefix))
        print(f"norm {kind} {sha(n.forward(rand(gen, B, C, 8, 16, 16), cond))}", flush=True)
    e = i2v_native.NativeEmbedder(ZD, False)
    e.load(T(synth.embedder_state_dict(seed=5, z_dim=ZD, norm="in")))
    print(f"embedder {sha(e.forward(img))}", flush=True)


if __name__ == "__main__":
    main()
