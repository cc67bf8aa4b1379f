"""A/B of the DTFVD feature path on one MI355X -> profiles/dtfvd_ab.md (+ .json).

  python tools/dtfvd_bench.py [--repeats 5] [--side 128] [--out DIR] [--step-timeout 240]

Single-process measurements, each GPU step in a child process of its own under its own ``timeout`` (a step that does not end clean stops
the script; nothing more is started on the GPU):
  * clips/s of the dynamic-texture I3D's feature forward (``InceptionI3D.forward_frames``: input stage + network + average pool) at
    B = 20 for T = 16 (length-16 network) and T = 32 (length-32 network), events on the stream, warm-up, median and spread;
  * the host-round-trip alternative on the same box -- the reference's order of work: the batch to the host, a CPU bilinear resize to
    224 x 224, back to the device, the same native network (``get_representation``) -- wall clock.
No number of this path appears in any document of the project unless this script wrote it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "image2video-synthesis-using-cinns_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def step(T, side, repeats, B=20):
    """One measurement (runs in the child process): prints one JSON line."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import dtfvd_common as dc
    from metrics.DTFVD import ID3, ID3_32
    length = 32 if T > 16 else 16
    model = (ID3_32 if length == 32 else ID3).InceptionI3D(18, 1)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in dc.dti3d_state_dict(1, 18).items()}, strict=True)
    model = model.cuda().eval()
    clips = torch.from_numpy(dc.clips(9, 4, T, side, side)).cuda().repeat(B // 4, 1, 1, 1, 1).contiguous()

    def device():
        return model.forward_frames(clips)

    def host_round_trip():
        h = clips.cpu()
        h = F.interpolate(h.reshape(-1, 3, side, side), mode="bilinear", size=(224, 224), align_corners=True).reshape(B, T, 3, 224, 224)
        return model.get_representation(h.cuda().permute(0, 2, 1, 3, 4))[:, :, 0]
    for _ in range(2):
        device()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        device()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    err = float((device() - host_round_trip()).norm() / device().norm())
    wall = []
    for _ in range(max(2, repeats // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_round_trip()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    spread = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "repeats": len(v)}  # noqa: E731
    print(json.dumps({"device_name": torch.cuda.get_device_name(0), "T": T, "length": length, "B": B, "side": side, "device": spread(ms),
                      "host_round_trip": spread(wall), "device_clips_per_s": B / statistics.median(ms) * 1e3,
                      "host_round_trip_clips_per_s": B / statistics.median(wall) * 1e3, "rel_l2_device_vs_round_trip": err}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--side", type=int, default=128, help="height and width of the clips (the texture models are 128 x 128)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of dtfvd_ab.md / dtfvd_ab.json")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--step", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step is not None:
        return step(args.step, args.side, args.repeats)
    rows = []
    for T in (16, 32):
        r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(T), "--side",
                            str(args.side), "--repeats", str(args.repeats)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"dtfvd_bench: the T = {T} step ended with status {r.returncode}; nothing more is run")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "dtfvd_ab.json"), "w") as f:
        json.dump(rows, f, indent=1)
    s = args.side
    lines = ["# DTFVD feature forward on the device: measured figures", "",
             f"Device: {rows[0]['device_name']}.  `tools/dtfvd_bench.py`, B = 20 clips of {s} x {s}, one process per row.  Device path: events on the stream, "
             f"{args.repeats} repeats after 2 warm-up runs.  Host round trip: wall clock around the reference's order of work (batch to the host, CPU bilinear "
             "resize to 224 x 224, back to the device, the same native network).  Median (min .. max).", "",
             "| T | network | device ms | device clips/s | host round trip ms | round-trip clips/s | ratio | rel-L2 device vs round trip |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        a, b = r["device"], r["host_round_trip"]
        lines.append(f"| {r['T']} | length {r['length']} | {a['median_ms']:.2f} ({a['min_ms']:.2f} .. {a['max_ms']:.2f}) | {r['device_clips_per_s']:.1f} | "
                     f"{b['median_ms']:.1f} ({b['min_ms']:.1f} .. {b['max_ms']:.1f}) | {r['host_round_trip_clips_per_s']:.1f} | "
                     f"{b['median_ms'] / a['median_ms']:.2f}x | {r['rel_l2_device_vs_round_trip']:.2e} |")
    lines += ["", "The round-trip figure depends on the host (CPU resize, PCIe copies) as much as on the GPU; it is the alternative on THIS box, not a constant."]
    with open(os.path.join(out, "dtfvd_ab.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", os.path.join(out, "dtfvd_ab.md"))


if __name__ == "__main__":
    main()
