"""A/B of the FVD path on one MI355X -> profiles/fvd_ab.md (+ .json).

  python tools/fvd_bench.py [--repeats 5] [--quick] [--out DIR]

Measures (warm-up, events on the stream, several repeats, median and spread reported):
  * clips/s of ``I3D.forward_frames`` at B = 20 (the reference's batch) and B = 64 for 64 x 64 and 128 x 128 clips of 16 frames, next to
    the SAME network in stock PyTorch-ROCm ops on the same GPU (``torch_i3d`` below: F.conv3d / F.batch_norm / F.max_pool3d on the
    module's own parameters, fed the same 224 x 224 input the native input stage produces);
  * one FVD pass over a synthetic set of decoded clips in the package's order of work (frames stay on the device, streaming
    statistics) against the reference's order of work (all frames to the host, CPU resize of the whole set, batches of 20 back);
  * the end-to-end tolerance record: the reference's fp32 and fp64 FVD values of tests/golden/fvd_end2end.npz, their ratio, the GPU result.
The per-kernel share of the fp32 matrix-core peak needs a ``rocprofv3 --kernel-trace --stats`` run of its own (not done by this script)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "image2video-synthesis-using-cinns_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
import fvd_common as fc  # noqa: E402
from metrics.PyTorch_FVD import FVD_logging as fvd  # noqa: E402
from metrics.PyTorch_FVD.I3D import I3D, MIXED, get_padding_shape  # noqa: E402


def _unit(m, x, k=1, stride=1, relu=True):
    if k > 1:
        pt = get_padding_shape(k, stride, x.shape[2] % stride if stride > 1 else 0)
        ps = get_padding_shape(k, stride)
        x = F.pad(x, (*ps, *ps, *pt))
    x = F.conv3d(x, m.conv3d.weight, m.conv3d.bias, stride=stride)
    if hasattr(m, "batch3d"):
        b = m.batch3d
        x = F.batch_norm(x, b.running_mean, b.running_var, b.weight, b.bias, False, 0.0, b.eps)
    return F.relu(x) if relu else x


def _pool(x, kt, k, st, s):
    pt = get_padding_shape(kt, st, x.shape[2] % st if st > 1 else 0)
    ps = get_padding_shape(k, s)
    return F.max_pool3d(F.pad(x, (*ps, *ps, *pt)), (kt, k, k), (st, s, s), ceil_mode=True)


@torch.no_grad()
def torch_i3d(model, x):
    """The network in stock torch ops: x [B, 3, T, 224, 224] -> logits."""
    x = _unit(model.conv3d_1a_7x7, x, 7, 2)
    x = _pool(x, 1, 3, 1, 2)
    x = _unit(model.conv3d_2c_3x3, _unit(model.conv3d_2b_1x1, x), 3)
    x = _pool(x, 1, 3, 1, 2)
    for name, _cin, _o in MIXED:
        m = getattr(model, name)
        x = torch.cat((_unit(m.branch_0, x), _unit(m.branch_1[1], _unit(m.branch_1[0], x), 3), _unit(m.branch_2[1], _unit(m.branch_2[0], x), 3),
                       _unit(m.branch_3[1], _pool(x, 3, 3, 1, 1))), 1)
        if name == "mixed_3c":
            x = _pool(x, 3, 3, 2, 2)
        if name == "mixed_4f":
            x = _pool(x, 2, 2, 2, 2)
    x = _unit(model.conv3d_0c_1x1, F.avg_pool3d(x, (2, 7, 7), (1, 1, 1)), relu=False)
    return x.squeeze(3).squeeze(3).mean(2)


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of fvd_ab.md / fvd_ab.json")
    ap.add_argument("--quick", action="store_true", help="B = 20 only, small FVD set")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = True
    res = {"device": torch.cuda.get_device_name(0), "forward": [], "notes": []}
    model = I3D(400)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fc.i3d_state_dict(1, 400).items()})
    model = model.cuda().eval()
    for side in (64, 128):
        for B in ((20,) if args.quick else (20, 64)):
            clips = torch.from_numpy(fc.clips(9, 4, 16, side, side)).cuda().repeat(B // 4, 1, 1, 1, 1).contiguous()
            nat = timed(lambda: model.forward_frames(clips, True), args.repeats)
            x224 = (F.interpolate(clips.reshape(-1, 3, side, side), mode="bilinear", size=(224, 224), align_corners=True)
                    .reshape(B, 16, 3, 224, 224).add(1).div(2).permute(0, 2, 1, 3, 4).contiguous())
            ref = timed(lambda: torch_i3d(model, x224), args.repeats)
            err = float((model.forward_frames(clips, True) - torch_i3d(model, x224)).norm() / torch_i3d(model, x224).norm())
            res["forward"].append({"side": side, "B": B, "native": nat, "stock_torch": ref, "native_clips_per_s": B / nat["median_ms"] * 1e3,
                                   "stock_clips_per_s": B / ref["median_ms"] * 1e3, "rel_l2_native_vs_stock": err})
            print(res["forward"][-1], flush=True)
            del clips, x224
            torch.cuda.empty_cache()

    # one FVD pass: device order of work vs the reference's order of work (same native network on both sides)
    n = 40 if args.quick else 200
    gen = torch.from_numpy(fc.clips(10, 8, 16, 64, 64)).cuda().repeat(n // 8, 1, 1, 1, 1).contiguous()
    orig = torch.from_numpy(fc.clips(11, 8, 16, 64, 64)).cuda().repeat(n // 8, 1, 1, 1, 1).contiguous()

    def device_pass():
        acc = fvd.FVDAccumulator(model)
        for i in range(0, n, 20):
            acc.update(gen[i:i + 20], "gen")
            acc.update(orig[i:i + 20], "orig")
        return acc.state()

    def host_pass():
        sets = []
        for d in (gen, orig):
            h = d.cpu()
            h = F.interpolate(h.reshape(-1, 3, 64, 64), mode="bilinear", size=(224, 224), align_corners=True).reshape(n, 16, 3, 224, 224)
            sets.append((h + 1.0) / 2.0)
        acts = []
        for h in sets:
            rows = [model.forward_frames(h[i:i + 20].cuda(), False).cpu().numpy() for i in range(0, n, 20)]
            acts.append(np.concatenate(rows))
        return acts

    def wall(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": reps}
    res["fvd_pass"] = {"clips_per_set": n, "device_order": wall(device_pass, 3), "reference_order": wall(host_pass, 2)}
    print(res["fvd_pass"], flush=True)

    arr, meta = fc.load_fixture("fvd_end2end")
    m16 = I3D(16)
    m16.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fc.i3d_state_dict(meta["weights"]["seed"], 16).items()})
    m16 = m16.cuda().eval()
    sets = [torch.from_numpy(fc.clips(m["seed"], m["n"], m["t"], m["h"], m["w"], signed=m["signed"])).cuda() for m in (meta["gen"], meta["orig"])]
    got = fvd.calculate_FVD(m16, sets[0], sets[1], meta["batch_size"])
    res["end2end"] = {"reference_fp32": meta["fvd_fp32"], "reference_fp64": meta["fvd_fp64"], "reference_fp32_vs_fp64_rel": meta["ref_fp32_vs_fp64_rel"],
                      "allowed_rel": 10 * meta["ref_fp32_vs_fp64_rel"], "gpu": got, "gpu_vs_reference_fp32_rel": abs(got - meta["fvd_fp32"]) / abs(meta["fvd_fp32"]),
                      "gpu_vs_reference_fp64_rel": abs(got - meta["fvd_fp64"]) / abs(meta["fvd_fp64"])}
    _, fm = fc.load_fixture("fvd_frechet")
    res["frechet"] = {"eigh_vs_sqrtm_rel_at_fixture_time": fm["eigh_vs_sqrtm_rel"], "gate": 10 * fm["eigh_vs_sqrtm_rel"]}
    print(res["end2end"], flush=True)

    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "fvd_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# FVD on the device: measured figures", "", f"Device: {res['device']}.  Events on the stream, {args.repeats} repeats after 2 warm-up runs; median (min .. max).", "",
             "## I3D forward, 16-frame clips (input stage included) vs the same network in stock PyTorch-ROCm ops", "",
             "| clip | B | native ms | native clips/s | stock torch ms | stock clips/s | speed-up | rel-L2 native vs stock |", "|---|---|---|---|---|---|---|---|"]
    for r in res["forward"]:
        a, b = r["native"], r["stock_torch"]
        lines.append(f"| {r['side']}x{r['side']} | {r['B']} | {a['median_ms']:.2f} ({a['min_ms']:.2f} .. {a['max_ms']:.2f}) | {r['native_clips_per_s']:.0f} | "
                     f"{b['median_ms']:.2f} ({b['min_ms']:.2f} .. {b['max_ms']:.2f}) | {r['stock_clips_per_s']:.0f} | {b['median_ms'] / a['median_ms']:.2f}x | "
                     f"{r['rel_l2_native_vs_stock']:.2e} |")
    p = res["fvd_pass"]
    lines += ["", f"## One FVD pass, {p['clips_per_set']} clips per set (64x64x16), batches of 20, wall clock", "",
              f"* device order of work (frames stay on the GPU, streaming statistics): {p['device_order']['median_ms']:.1f} ms "
              f"({p['device_order']['min_ms']:.1f} .. {p['device_order']['max_ms']:.1f})",
              f"* the reference's order of work (frames to the host, CPU resize of the whole set, batches back; same native network): "
              f"{p['reference_order']['median_ms']:.1f} ms ({p['reference_order']['min_ms']:.1f} .. {p['reference_order']['max_ms']:.1f})", "",
              "## Tolerances", ""]
    e = res["end2end"]
    lines += [f"* end to end (`fvd_end2end`): reference fp32 {e['reference_fp32']!r}, reference fp64 {e['reference_fp64']!r}, their relative difference "
              f"{e['reference_fp32_vs_fp64_rel']:.3e}; allowed 10 x = {e['allowed_rel']:.3e}; GPU {e['gpu']!r} = {e['gpu_vs_reference_fp32_rel']:.3e} from the fp32 value "
              f"({e['gpu_vs_reference_fp64_rel']:.3e} from the fp64 value)",
              f"* Frechet function (`fvd_frechet`): eigenvalue vs sqrtm formulation {res['frechet']['eigh_vs_sqrtm_rel_at_fixture_time']:.3e} relative (CPU, at fixture "
              f"time); gate 10 x = {res['frechet']['gate']:.3e}", "",
              "Not measured here: the share of the fp32 matrix-core peak of the three heaviest convs (needs a `rocprofv3 --kernel-trace --stats` run of its own)."]
    with open(os.path.join(out, "fvd_ab.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", os.path.join(out, "fvd_ab.md"))


if __name__ == "__main__":
    main()
