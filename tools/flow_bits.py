"""Digests of the cINN pass for A/B runs of host-code changes: prints one sha256 per case over the bytes of z (inverse), z~ and the
log-det (forward), for the case table of test_flow_fold_keeps_the_bits (both I2V_FLOW_FOLD settings) and the switch table of
tests/test_gpu_flow_sched.py (folded, unfolded and generic chain).  Two builds of the library compute the same function iff the two
outputs are equal, e.g.

    python tools/flow_bits.py > a.txt;  I2V_LIB_PATH=<other build, relative to the repository> python tools/flow_bits.py > b.txt

The digests depend on the toolchain (expf, fmaf contraction), so they are compared between builds on one machine, never stored."""
import hashlib
import itertools
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

FOLD_CASES = [dict(emb=64, hidden=512, depth=2, nfl=20, control=False, f16=0, Bs=(64, 8, 3, 150)),
              dict(emb=128, hidden=512, depth=2, nfl=20, control=False, f16=1, Bs=(24, 130)),
              dict(emb=94, hidden=512, depth=2, nfl=20, control=True, f16=0, Bs=(21,)),
              dict(emb=64, hidden=256, depth=1, nfl=3, control=False, f16=0, Bs=(70, 5)),
              dict(emb=64, hidden=384, depth=3, nfl=2, control=False, f16=0, Bs=(33,))]
FLAGS = list(itertools.product((False, True), (False, True), ("lrelu", "none")))   # skip_actnorm, skip_shuffle, activation
CHAINS = {"folded": ("I2V_FLOW_FOLD", "1"), "unfolded": ("I2V_FLOW_FOLD", "0"), "generic": ("I2V_FLOW_TILE", "0")}


def handle(chain, sd, **kw):
    var, val = CHAINS[chain]
    os.environ[var] = val          # read at create (I2V_FLOW_TILE) / load (I2V_FLOW_FOLD) only
    try:
        h = i2v_native.NativeFlow(**kw)
        h.load(sd)
    finally:
        del os.environ[var]
    return h


def digest(h, x, e):
    zt, ld = h.forward(x, e)
    z = h.inverse(x, e)
    z2 = h.inverse(x, e)           # the replayed graph
    assert torch.equal(z, z2)
    m = hashlib.sha256()
    for t in (z, zt, ld):
        m.update(t.cpu().numpy().tobytes())
    return m.hexdigest()


def main():
    torch.set_grad_enabled(False)
    T = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}   # noqa: E731
    _, residual, embed = synth.bench_inputs(150, 64, 128)
    for n, c in enumerate(FOLD_CASES):
        sd = T(synth.flow_state_dict(seed=11, embedding_dim=c["emb"], n_flows=c["nfl"], hidden_dim=c["hidden"], hidden_depth=c["depth"],
                                     control=c["control"]))
        for chain in ("unfolded", "folded"):
            h = handle(chain, sd, in_channels=64, embedding_dim=c["emb"], hidden_dim=c["hidden"], hidden_depth=c["depth"], n_flows=c["nfl"],
                       control=1 if c["control"] else 0, linear_f16=c["f16"])
            for B in c["Bs"]:
                x, e = residual[:B].cuda().contiguous(), embed[:B, :c["emb"]].cuda().contiguous()
                print(f"fold_case{n} {chain} B={B} {digest(h, x, e)}", flush=True)
    sd = T(synth.flow_state_dict(seed=5, n_flows=2, embedding_dim=64, hidden_dim=128, hidden_depth=1))
    for skip_an, skip_sh, act in FLAGS:
        for chain in CHAINS:
            h = handle(chain, sd, in_channels=64, embedding_dim=64, hidden_dim=128, hidden_depth=1, n_flows=2, activation=act,
                       skip_actnorm=skip_an, skip_shuffle=skip_sh)
            for B in (3, 17):
                x, e = residual[:B].cuda().contiguous(), embed[:B, :64].cuda().contiguous()
                print(f"flags skip_actnorm={int(skip_an)} skip_shuffle={int(skip_sh)} activation={act} {chain} B={B} {digest(h, x, e)}", flush=True)


if __name__ == "__main__":
    main()
