#!/usr/bin/env python
"""A/B of several realizations per start frame: ``Model.sample(x_0, K)`` (the start-frame work once per frame) against
``Model.synthesize(x_0.repeat_interleave(K, 0))`` at the same F*K samples, back to back in one process.

    python tools/realizations_bench.py [--steps 20] [--warmup 3] [--json out.json]

Cases: BAIR 64x64 nf = 64 (F x K = 64x1, 16x4, 8x8) and Landscape 128x128 nf = 32 (32x1, 8x4); decoder modes mma = 1 and fp16;
"decoder" = the conditioning embedding given (``embed=``), "pixels" = the ResNet-50 embedder run on the start frames (synthetic weights,
``i2v_synth.embedder_state_dict``).  Per case: median ms per call over ``--steps`` timed calls (HIP events around each call, after
``--warmup`` calls), the arms interleaved call by call, and the decoder workspace of either arm.  The weights are the deterministic
synthetic ones of bench.py.  Prints one JSON object per case."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = [("bair64", 64, 1), ("bair64", 16, 4), ("bair64", 8, 8), ("land128", 32, 1), ("land128", 8, 4)]
CFG = {"bair64": dict(nf=64, emb=64, img=64, ups=[2, 1], upt=[2, 1]), "land128": dict(nf=32, emb=128, img=128, ups=[2, 2], upt=[2, 1])}


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def make_model(cfg, mma, pixels):
    """A get_model.Model on the synthetic weights (no checkpoint files): the same attributes Model.__init__ sets."""
    import i2v_synth as synth
    from get_model import Model
    from stage1_VAE.modules.decoder import Generator
    from stage2_cINN.AE.modules.AE import ResnetEncoder
    from stage2_cINN.modules.INN import SupervisedTransformer
    embedder = None
    if pixels:
        embedder = ResnetEncoder({"deterministic": False, "in_size": cfg["img"], "norm": "in", "encoder_type": "resnet50",
                                  "z_dim": cfg["emb"]})
        embedder.load_state_dict(T(synth.embedder_state_dict(seed=3, z_dim=cfg["emb"], norm="in")))
        embedder = embedder.cuda().eval()
    m = Model.__new__(Model)
    torch.nn.Module.__init__(m)
    gen = Generator({"channel_factor": cfg["nf"], "z_dim": 64, "upsample_s": cfg["ups"], "upsample_t": cfg["upt"], "spectral_norm": True,
                     "mma": mma})
    gen.load_state_dict(T(synth.decoder_state_dict(seed=7, channel_factor=cfg["nf"])))
    m.decoder = gen.cuda().eval()
    m.flow = SupervisedTransformer(flow_in_channels=64, flow_embedding_channels=cfg["emb"], n_flows=20, flow_hidden_depth=2,
                                   flow_mid_channels=512, flow_conditioning_option="None", dic=None, control=False,
                                   embedder=embedder).cuda()
    m.flow.flow.load_state_dict(T(synth.flow_state_dict(seed=7, embedding_dim=cfg["emb"])))
    m.flow.eval()
    m.z_dim, m.vid_length, m.config, m.overlap, m._prefetch = 64, 16, None, True, None
    return m


def run_case(name, F, K, mma, pixels, steps, warmup):
    import i2v_synth as synth
    cfg = CFG[name]
    model = make_model(cfg, mma, pixels)
    x0, _, emb = synth.bench_inputs(F, cfg["img"], cfg["emb"])
    x0, emb = x0.cuda(), emb.cuda()
    residual = torch.randn(F * K, 64, generator=torch.Generator().manual_seed(1)).cuda()
    x_rep, emb_rep = x0.repeat_interleave(K, 0).contiguous(), emb.repeat_interleave(K, 0).contiguous()
    e_sh, e_rep = (None, None) if pixels else (emb, emb_rep)
    arms = {"shared": lambda: model.sample(x0, K, residual=residual, embed=e_sh),
            "repeated": lambda: model.synthesize(x_rep, residual=residual, embed=e_rep)}
    out = {k: f() for k, f in arms.items()}
    torch.cuda.synchronize()
    same = bool(torch.equal(out["shared"].reshape(F * K, *out["shared"].shape[2:]), out["repeated"]))
    del out
    times = {k: [] for k in arms}
    for i in range(warmup + steps):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
    model.check()
    h = model.decoder.native()
    ws = {"shared": h.workspace_bytes(F, cfg["img"], cfg["img"], K), "repeated": h.workspace_bytes(F * K, cfg["img"], cfg["img"], 1)}
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"config": name, "F": F, "K": K, "mma": mma, "input": "pixels" if pixels else "decoder", "steps": steps,
            "shared_ms": round(med["shared"], 3), "repeated_ms": round(med["repeated"], 3),
            "gain_pct": round(100.0 * (med["repeated"] - med["shared"]) / med["repeated"], 2),
            "shared_min_ms": round(min(times["shared"]), 3), "repeated_min_ms": round(min(times["repeated"]), 3),
            "ws_shared_mib": round(ws["shared"] / 2**20, 1), "ws_repeated_mib": round(ws["repeated"] / 2**20, 1), "bit_identical": same}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mma", nargs="*", default=["1", "fp16"])
    ap.add_argument("--input", nargs="*", default=["decoder", "pixels"])
    ap.add_argument("--config", nargs="*", default=["bair64", "land128"])
    ap.add_argument("--json", type=str, help="also write the rows to this file (JSON list)")
    args = ap.parse_args(argv)
    torch.set_grad_enabled(False)
    rows = []
    for mma in args.mma:
        for inp in args.input:
            for name, F, K in CASES:
                if name not in args.config:
                    continue
                r = run_case(name, F, K, int(mma) if mma.isdigit() else mma, inp == "pixels", args.steps, args.warmup)
                print(json.dumps(r), flush=True)
                rows.append(r)
                torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if not all(r["bit_identical"] for r in rows):
        raise SystemExit("realizations_bench: the shared path differs from the repeated one")


if __name__ == "__main__":
    main()
