#!/usr/bin/env python
"""A/B of the output stage: today's host path (``seq.cpu()`` + ``convert_seq2gif`` + ``astype(uint8)``) against the device path
(``i2v_pipeline.FrameSink``: peak + interleave kernels, one pinned uint8 copy), in one process, the arms alternating.

    python tools/frames_out_bench.py [--steps 10] [--warmup 2] [--stream 20] [--launches 100] [--json out.json] [--md out.md]

Per case (BAIR 64x64 nf = 64 B = 64 and Landscape 128x128 nf = 32 B = 32, T = 16; decoder modes mma = 1 and fp16):
  * handover: host-visible time per batch from "decoder enqueued" to "uint8 array usable on the host" (host clock; the decoder's own
    time is inside both arms), median and min..max, plus the decoder-only step of the same run (enqueue + synchronise);
  * stream: ``--stream`` batches through a UNIT-mode sink (convert + double-buffered copy under the next decoder), wall time per batch
    against the decoder-only step time: how much of the hand-over is hidden;
  * kernels: the two kernels by HIP events over ``--launches`` launches each, bytes moved / time (GB/s).
The weights are the deterministic synthetic ones of bench.py.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image2video-synthesis-using-cinns_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = {"bair64": dict(nf=64, img=64, ups=[2, 1], upt=[2, 1], batch=64), "land128": dict(nf=32, img=128, ups=[2, 2], upt=[2, 1], batch=32)}
HBM_ACHIEVABLE_GBS = 6300.0   # float4 copy on this GPU (the microarchitecture guide's measured figure)


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}


def run_case(name, mma, steps, warmup, n_stream, launches):
    import i2v_native
    import i2v_synth as synth
    from i2v_pipeline import FrameSink
    from stage1_VAE.modules.decoder import Generator
    from utils import auxiliaries as aux
    cfg = CFG[name]
    B = cfg["batch"]
    gen = Generator({"channel_factor": cfg["nf"], "z_dim": 64, "upsample_s": cfg["ups"], "upsample_t": cfg["upt"], "spectral_norm": True, "mma": mma})
    gen.load_state_dict(T(synth.decoder_state_dict(seed=7, channel_factor=cfg["nf"])))
    gen = gen.cuda().eval()
    x0, _, _ = synth.bench_inputs(B, cfg["img"], 64)
    x0 = x0.cuda()
    z = torch.randn(B, 64, generator=torch.Generator().manual_seed(1)).cuda()
    sink = FrameSink("peak")

    def arm_decoder():
        gen(x0, z)
        torch.cuda.synchronize()

    def arm_host():
        seq = gen(x0, z)
        return aux.convert_seq2gif(seq.cpu()).astype(np.uint8)

    def arm_device():
        sink.add(gen(x0, z))
        sink.finish()
        return sink.result()

    with torch.no_grad():
        same = bool(np.array_equal(arm_host(), arm_device()))
        arms = {"decoder_only": arm_decoder, "host_path": arm_host, "frame_sink": arm_device}
        times = {k: [] for k in arms}
        for i in range(warmup + steps):
            for k, f in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                dt = (time.perf_counter() - t0) * 1e3
                if i >= warmup:
                    times[k].append(dt)
        # a stream of batches, UNIT mode: convert + copy of batch i under the decoder of batch i + 1
        unit = FrameSink("unit")
        per = {"decoder_only": [], "unit_sink": []}
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n_stream):
                gen(x0, z)
            torch.cuda.synchronize()
            t_dec = (time.perf_counter() - t0) * 1e3 / n_stream
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            unit.add(gen(x0, z))
            for i in range(1, n_stream):
                unit.add(gen(x0, z))
                unit.result()
            unit.result()
            t_unit = (time.perf_counter() - t0) * 1e3 / n_stream
            if rep:                                # the first repetition warms the pinned buffers up
                per["decoder_only"].append(t_dec)
                per["unit_sink"].append(t_unit)
        # the two kernels alone
        seq = gen(x0, z)
        peak = torch.zeros(1, device="cuda")
        out = torch.empty(16, seq.shape[3], B * seq.shape[4], 3, dtype=torch.uint8, device="cuda")
        kern = {}
        for kname, fn, nbytes in (("frames_peak_kernel", lambda: i2v_native.frames_peak(seq, out=peak), seq.numel() * 4),
                                  ("frames_to_u8_kernel[peak]", lambda: i2v_native.frames_to_u8(seq, peak=peak, out=out, mode="peak"), seq.numel() * 5),
                                  ("frames_to_u8_kernel[unit]", lambda: i2v_native.frames_to_u8(seq, out=out, mode="unit"), seq.numel() * 5)):
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / launches
            kern[kname] = {"us_per_call": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1),
                           "share_of_achievable_hbm": round(nbytes / us / 1e3 / HBM_ACHIEVABLE_GBS, 3), "launches": launches}
    assert gen.native().status() == 0
    h, d, dec = (statistics.median(times[k]) for k in ("host_path", "frame_sink", "decoder_only"))
    return {"config": name, "batch": B, "mma": mma, "frames_mb_fp32": round(seq.numel() * 4 / 1e6, 1), "bytes_equal": same,
            "handover": {k: spread(v) for k, v in times.items()},
            "host_over_sink": round(h / d, 2), "tail_ms_host": round(h - dec, 3), "tail_ms_sink": round(d - dec, 3),
            "stream_unit": {"batches": n_stream, "decoder_only_ms_per_batch": [round(v, 3) for v in per["decoder_only"]],
                            "unit_sink_ms_per_batch": [round(v, 3) for v in per["unit_sink"]],
                            "exposed_ms_per_batch": round(statistics.median(per["unit_sink"]) - statistics.median(per["decoder_only"]), 3)},
            "kernels": kern}


def markdown(rows):
    out = ["# Output stage: host path vs FrameSink (one MI355X, one process, arms alternating)", "",
           "Host-visible ms per batch from \"decoder enqueued\" to \"uint8 strip usable on the host\"; median (min..max).", "",
           "| config | mma | fp32 MB | decoder only | host path | FrameSink | host / sink | tail host | tail sink | bytes equal |", "|---|---|---|---|---|---|---|---|---|---|"]

    def f(s):
        return f"{s['median_ms']:.2f} ({s['min_ms']:.2f}..{s['max_ms']:.2f})"
    for r in rows:
        hv = r["handover"]
        out.append(f"| {r['config']} B={r['batch']} | {r['mma']} | {r['frames_mb_fp32']} | {f(hv['decoder_only'])} | {f(hv['host_path'])} | {f(hv['frame_sink'])} | "
                   f"{r['host_over_sink']} | {r['tail_ms_host']} | {r['tail_ms_sink']} | {r['bytes_equal']} |")
    out += ["", "UNIT-mode stream (convert + double-buffered pinned copy under the next decoder), ms per batch:", "",
            "| config | mma | batches | decoder only | with the sink | exposed |", "|---|---|---|---|---|---|"]
    for r in rows:
        s = r["stream_unit"]
        out.append(f"| {r['config']} B={r['batch']} | {r['mma']} | {s['batches']} | {s['decoder_only_ms_per_batch']} | {s['unit_sink_ms_per_batch']} | {s['exposed_ms_per_batch']} |")
    out += ["", f"Kernels alone (HIP events over back-to-back launches; achievable HBM = {HBM_ACHIEVABLE_GBS / 1e3:.1f} TB/s):", "",
            "| config | kernel | us / call | MB moved | GB/s | share of achievable HBM |", "|---|---|---|---|---|---|"]
    for r in rows:
        if r["mma"] != rows[0]["mma"]:
            continue                        # the kernels do not depend on the decoder mode
        for k, v in r["kernels"].items():
            out.append(f"| {r['config']} B={r['batch']} | {k} | {v['us_per_call']} | {v['bytes'] / 1e6:.1f} | {v['GBps']} | {v['share_of_achievable_hbm']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stream", type=int, default=20)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--json", type=str)
    ap.add_argument("--md", type=str)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_out_bench needs a GPU")
    rows = []
    for name in ("bair64", "land128"):
        for mma in (1, "fp16"):
            rows.append(run_case(name, mma, args.steps, args.warmup, args.stream, args.launches))
            print(json.dumps(rows[-1]), flush=True)
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)
    if args.md:
        open(args.md, "w").write(markdown(rows))


if __name__ == "__main__":
    main()
