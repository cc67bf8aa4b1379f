"""Timing of the native FID Inception-v3 trunk on one MI355X -> profiles/fid_ab.md (+ .json).

  python tools/fid_bench.py [--repeats 5] [--batch 50] [--out DIR] [--step-timeout 300]

Single-process measurements, each GPU step in a child process of its own under its own ``timeout`` (a step that does not end clean stops
the script; nothing more is started on the GPU):
  * ``64`` / ``128``: ms of ``InceptionV3.forward`` (input stage: bilinear to 299 x 299, then the trunk to block 3) on a batch of source
    frames of that size, images per second, and the fraction of the 157 TFLOP/s fp32-MFMA peak that the trunk's convolution FLOPs over the
    WHOLE forward time amount to (an end-to-end figure, pools and the input stage in the time -- not a kernel's share of peak);
    as a yardstick the same trunk written with ``torch.nn.functional`` (conv2d, batch_norm, max / avg pools; fp32, same GPU, same
    synthesised weights, TF32-free) on the same input, and the relative L2 distance of the two results;
  * ``groups``: per layer group (the stem, Mixed_5b-5d, 6a, 6b-6e, 7a, 7b-7c) at the shapes behind a 299 x 299 input: ms of the group
    through ``i2v_inception_features`` (stem) / ``i2v_inception_mixed_forward`` (blocks), ms of its pools alone through
    ``i2v_inception_pool``, and from the two the share of the group's time that the convolution kernel takes; the group's convolution
    GFLOP and what they amount to over the group's time.
Events on the stream, 2 warm-up runs, median and spread.  No number of this path appears in any document of the project unless this script
wrote it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "image2video-synthesis-using-cinns_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_TFLOPS = 157.0
SEED = 1
GROUPS = (("stem", ()), ("Mixed_5b-5d", (0, 1, 2)), ("Mixed_6a", (3,)), ("Mixed_6b-6e", (4, 5, 6, 7)), ("Mixed_7a", (8,)), ("Mixed_7b-7c", (9, 10)))


def _time(fn, repeats):
    import torch
    for _ in range(2):
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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def _model(blocks=(3,)):
    import fid_common as fc
    from metrics.FID.inception import InceptionV3
    m = InceptionV3(output_blocks=list(blocks))
    m.load_state_dict(fc.torch_state_dict(SEED))
    return m.cuda().eval()


def _out(size, kernel, stride, padding):
    return tuple((s + 2 * p - k) // stride + 1 for s, k, p in zip(size, kernel, padding))


def conv_flops(side=299):
    """{group: convolution FLOPs per image} at a side x side trunk input, and the map in front of every Mixed block."""
    import fid_common as fc
    flops, maps = {g: 0.0 for g, _ in GROUPS}, {}
    d = (side, side)
    for i, (key, cin, cout, kernel, stride, padding) in enumerate(fc.STEM):
        d = _out(d, kernel, stride, padding)
        flops["stem"] += 2.0 * d[0] * d[1] * cin * cout * kernel[0] * kernel[1]
        if i in (2, 4):
            d = _out(d, (3, 3), 2, (0, 0))
    for gname, idx in GROUPS[1:]:
        for bi in idx:
            name, kind, cin, par = fc.MIXED[bi]
            maps[bi] = d
            units = fc.block_units(kind, cin, par)
            outd = None
            for pre, lasts in fc.block_branches(kind, par):
                h = d
                for step in list(pre) + [None]:
                    for s in ([step] if step is not None else lasts):
                        if isinstance(s, int):
                            o = _out(h, (3, 3), 2 if s == fc.POOL_MAX_S2 else 1, (0, 0) if s == fc.POOL_MAX_S2 else (1, 1))
                        else:
                            ci, co, kernel, stride, padding = units[s]
                            o = _out(h, kernel, stride, padding)
                            flops[gname] += 2.0 * o[0] * o[1] * ci * co * kernel[0] * kernel[1]
                    h = o
                outd = h
            d = outd
    return flops, maps


def torch_trunk(sd, x):
    """The FID trunk to block 3 in torch.nn.functional, fp32, on x [N, 3, 299, 299]; ``sd``: the state_dict as device tensors."""
    import torch
    import torch.nn.functional as F
    import fid_common as fc

    def unit(key, h):
        _, _, _, stride, padding = fc.UNITS[key]
        h = F.conv2d(h, sd[key + ".conv.weight"], stride=stride, padding=padding)
        return F.relu(F.batch_norm(h, sd[key + ".bn.running_mean"], sd[key + ".bn.running_var"], sd[key + ".bn.weight"], sd[key + ".bn.bias"], False, 0.0,
                                   fc.BN_EPS))

    def pool(kind, h):
        if kind == fc.POOL_MAX_S2:
            return F.max_pool2d(h, 3, 2)
        return F.max_pool2d(h, 3, 1, 1) if kind == fc.POOL_MAX_S1 else F.avg_pool2d(h, 3, 1, 1, count_include_pad=False)
    h = x
    for i, u in enumerate(fc.STEM):
        h = unit(u[0], h)
        if i in (2, 4):
            h = F.max_pool2d(h, 3, 2)
    for name, kind, cin, par in fc.MIXED:
        outs = []
        for pre, lasts in fc.block_branches(kind, par):
            t = h
            for step in pre:
                t = pool(step, t) if isinstance(step, int) else unit(f"{name}.{step}", t)
            outs += [pool(s, t) if isinstance(s, int) else unit(f"{name}.{s}", t) for s in lasts]
        h = torch.cat(outs, 1)
    return h.mean((2, 3))


def step_forward(side, batch, repeats):
    import torch
    import fid_common as fc
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m = _model()
    frames = torch.from_numpy(fc.clips(3, batch, 1, side, side))[:, 0].contiguous().cuda()
    native = _time(lambda: m(frames), repeats)
    sd = {k: v.cuda() for k, v in fc.torch_state_dict(SEED).items() if v.dtype == torch.float32}
    with torch.no_grad():
        def yard():
            return torch_trunk(sd, torch.nn.functional.interpolate(frames, size=(299, 299), mode="bilinear", align_corners=False))
        torch_t = _time(yard, repeats)
        a, b = m(frames)[0].flatten(1).double(), yard().double()
    flops = sum(conv_flops()[0].values())
    print(json.dumps({"device_name": torch.cuda.get_device_name(0), "side": side, "batch": batch, "native": native, "torch_functional": torch_t,
                      "images_per_s": batch / (native["median_ms"] * 1e-3), "torch_images_per_s": batch / (torch_t["median_ms"] * 1e-3),
                      "conv_gflop_per_image": flops / 1e9,
                      "conv_flops_over_forward_time_fraction_of_peak": batch * flops / (native["median_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12),
                      "rel_l2_native_vs_torch": float((a - b).norm() / b.norm())}))


def step_groups(batch, repeats):
    import torch
    import fid_common as fc
    import i2v_native
    m = _model((1,))
    native = m.native()
    flops, maps = conv_flops()
    x = torch.randn(batch, 299, 299, 4, device="cuda")
    x[..., 3] = 0
    rows = []
    for gname, idx in GROUPS:
        if gname == "stem":
            whole = _time(lambda: native.features(x, (1,)), repeats)
            p0, p1 = torch.randn(batch, 147, 147, 64, device="cuda"), torch.randn(batch, 71, 71, 192, device="cuda")
            pools = _time(lambda: (i2v_native.inception_pool(p0, fc.POOL_MAX_S2), i2v_native.inception_pool(p1, fc.POOL_MAX_S2)), repeats)
            shape = "299 -> 35"
        else:
            ins = [torch.relu(torch.randn(batch, *maps[bi], fc.MIXED[bi][2], device="cuda")) for bi in idx]
            outs = [native.mixed(bi, t) for bi, t in zip(idx, ins)]
            whole = _time(lambda: [native.mixed(bi, t, o) for bi, t, o in zip(idx, ins, outs)], repeats)
            kinds = [(t, next(s for pre, lasts in fc.block_branches(fc.MIXED[bi][1], fc.MIXED[bi][3]) for s in list(pre) + list(lasts) if isinstance(s, int)))
                     for bi, t in zip(idx, ins)]
            pools = _time(lambda: [i2v_native.inception_pool(t, k) for t, k in kinds], repeats)
            shape = f"{maps[idx[0]][0]} x {maps[idx[0]][1]}"
        conv_ms = max(whole["median_ms"] - pools["median_ms"], 0.0)
        rows.append({"group": gname, "map": shape, "conv_gflop_per_image": flops[gname] / 1e9, "whole": whole, "pools": pools,
                     "conv_share_of_group": conv_ms / whole["median_ms"],
                     "conv_flops_over_group_time_fraction_of_peak": batch * flops[gname] / (whole["median_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12)})
    total = sum(r["whole"]["median_ms"] for r in rows)
    for r in rows:
        r["share_of_trunk"] = r["whole"]["median_ms"] / total
    print(json.dumps({"device_name": torch.cuda.get_device_name(0), "batch": batch, "groups": rows, "sum_ms": total}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50, help="images per forward (calculate_FID's batch_size in eval_synthesis_quality.py)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of fid_ab.md / fid_ab.json")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "groups":
        return step_groups(args.batch, args.repeats)
    if args.step:
        return step_forward(int(args.step), args.batch, args.repeats)
    res = {}
    for name in ("64", "128", "groups"):
        r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--batch",
                            str(args.batch), "--repeats", str(args.repeats)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"fid_bench: the {name} step ended with status {r.returncode}; nothing more is run")
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(name, res[name], flush=True)
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "fid_ab.json"), "w") as f:
        json.dump(res, f, indent=1)

    def span(u):
        return f"{u['median_ms']:.2f} ({u['min_ms']:.2f} .. {u['max_ms']:.2f})"
    lines = ["# Native FID Inception-v3 trunk: measured figures", "",
             f"Device: {res['64']['device_name']}.  `tools/fid_bench.py`, one process per step, events on the stream, {args.repeats} repeats after 2 "
             "warm-up runs.  Median (min .. max).  Synthesised weights (tests/fid_common.py); exact fp32 on both sides (no TF32).", "",
             f"`InceptionV3.forward` (input stage to 299 x 299, trunk to block 3), batch {args.batch}; yardstick: the same trunk in "
             "`torch.nn.functional` on the same GPU.  The fraction of the peak is the trunk's convolution FLOPs "
             f"({res['64']['conv_gflop_per_image']:.2f} GFLOP per image) over the WHOLE forward time against the {PEAK_TFLOPS:.0f} TFLOP/s fp32-MFMA "
             "peak: an end-to-end figure, not a kernel's share of peak.", "",
             "| source frames | native ms | native images/s | conv FLOPs / forward time, of peak | torch.nn.functional ms | torch images/s | "
             "rel-L2 native vs torch |", "|---|---|---|---|---|---|---|"]
    for k in ("64", "128"):
        r = res[k]
        lines.append(f"| {k} x {k} | {span(r['native'])} | **{r['images_per_s']:.0f}** | {100 * r['conv_flops_over_forward_time_fraction_of_peak']:.1f} % | "
                     f"{span(r['torch_functional'])} | {r['torch_images_per_s']:.0f} | {r['rel_l2_native_vs_torch']:.1e} |")
    lines += ["", f"Layer groups at the shapes behind a 299 x 299 input, batch {args.batch}, random inputs: the group through "
              "`i2v_inception_features` (stem, input stage excluded) or `i2v_inception_mixed_forward` (blocks), its pools alone through "
              "`i2v_inception_pool`; the convolution kernel's share of the group is (group - pools) / group (launch gaps count as convolution time).", "",
              "| group | map | conv GFLOP / image | group ms | pools ms | conv kernel share of the group | group share of the trunk | conv FLOPs / group "
              "time, of peak |", "|---|---|---|---|---|---|---|---|"]
    for r in res["groups"]["groups"]:
        lines.append(f"| {r['group']} | {r['map']} | {r['conv_gflop_per_image']:.2f} | {span(r['whole'])} | {span(r['pools'])} | "
                     f"{100 * r['conv_share_of_group']:.1f} % | {100 * r['share_of_trunk']:.1f} % | "
                     f"{100 * r['conv_flops_over_group_time_fraction_of_peak']:.1f} % |")
    with open(os.path.join(out, "fid_ab.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", os.path.join(out, "fid_ab.md"))


if __name__ == "__main__":
    main()
