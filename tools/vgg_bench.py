"""Timing of the native VGG-16 trunk and of LPIPS on one MI355X -> profiles/vgg_ab.md (+ .json).

  python tools/vgg_bench.py [--repeats 5] [--batch 5] [--out DIR] [--step-timeout 240]

Single-process measurements, each GPU step in a child process of its own under its own ``timeout`` (a step that does not end clean stops
the script; nothing more is started on the GPU):
  * ``layers``: ms of every convolution of the trunk at the shape it has behind a 224 x 224 input (``i2v_native.NativeVGG.features`` is
    timed as a whole; the layers one by one through ``i2v_vgg_conv_unit``, end to end: an upper bound), the fraction of the 157 TFLOP/s
    fp32-MFMA peak, and ms per 224 x 224 image for the whole trunk with its input stage;
  * ``lpips``: ms of ``LPIPS.forward`` on 10 image pairs at 64 x 64 and at 128 x 128.
Events on the stream, 2 warm-up runs, median and spread.  No number of this path appears in any document of the project unless this
script wrote it."""
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


def _models(lin):
    import torch
    import vgg_common as vc
    from stage2_cINN.AE.modules.LPIPS import LPIPS
    from stage2_cINN.AE.modules.vgg16 import vgg16
    own = {k: torch.from_numpy(v) for k, v in zip(vc.holder_keys(), vc.vgg_state_dict(1).values())}
    if not lin:
        m = vgg16(pretrained=False)
        m.load_state_dict(own, strict=True)
        return m.cuda().eval()
    m = LPIPS()
    sd = {"net." + k: v for k, v in own.items()}
    sd.update({k: torch.from_numpy(v) for k, v in vc.lin_state_dict(2).items()})
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval()


def step_layers(batch, repeats):
    import torch
    import i2v_native
    import vgg_common as vc
    m = _models(False)
    frames = torch.from_numpy(vc.clips(3, batch, 1, 128, 128))[:, 0].contiguous().cuda()
    native = m.native()

    def whole():
        return native.features(i2v_native.vgg_input_stage(frames, i2v_native.VGG_INPUT_DIVERSITY, (224, 224), False))
    total = _time(whole, repeats)
    rows, side, flops_all = [], 224, 0.0
    sd = vc.vgg_state_dict(1)
    for idx, cin, cout in vc.CONVS:
        flops = 2.0 * batch * side * side * 9 * cin * cout
        flops_all += flops
        rows.append({"layer": f"features.{idx}", "cin": cin, "cout": cout, "side": side, "gflop": flops / 1e9})
        if idx in vc.POOL_AFTER:
            side //= 2
    # per layer: the unit entry END TO END (pack + upload + launch + synchronise): an upper bound of the kernel's time, flagged as such
    for r, (idx, cin, cout) in zip(rows, vc.CONVS):
        x = torch.randn(batch, r["side"], r["side"], 4 if cin == 3 else cin, device="cuda")
        w, b = torch.from_numpy(sd[f"features.{idx}.weight"]), torch.from_numpy(sd[f"features.{idx}.bias"])
        r["unit_call"] = _time(lambda: i2v_native.vgg_conv_unit(x, w, b), repeats)
    print(json.dumps({"device_name": torch.cuda.get_device_name(0), "batch": batch, "trunk": total, "gflop_per_image": flops_all / batch / 1e9,
                      "ms_per_image": total["median_ms"] / batch,
                      "fraction_of_peak": flops_all / (total["median_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12), "layers": rows}))


def step_lpips(side, repeats):
    import torch
    import vgg_common as vc
    m = _models(True)
    a = torch.from_numpy(vc.clips(5, 10, 1, side, side))[:, 0].contiguous().cuda()
    b = torch.from_numpy(vc.clips(6, 10, 1, side, side))[:, 0].contiguous().cuda()
    print(json.dumps({"device_name": torch.cuda.get_device_name(0), "side": side, "pairs": 10, "lpips": _time(lambda: m(a, b), repeats)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=5, help="images per trunk forward (one group of the diversity score: n_realiz)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of vgg_ab.md / vgg_ab.json")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "layers":
        return step_layers(args.batch, args.repeats)
    if args.step:
        return step_lpips(int(args.step), args.repeats)
    res = {}
    for name in ("layers", "64", "128"):
        r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--batch",
                            str(args.batch), "--repeats", str(args.repeats)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"vgg_bench: the {name} step ended with status {r.returncode}; nothing more is run")
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(name, res[name], flush=True)
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "vgg_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
    L = res["layers"]
    t = L["trunk"]
    lines = ["# Native VGG-16 trunk and LPIPS: measured figures", "",
             f"Device: {L['device_name']}.  `tools/vgg_bench.py`, one process per step, events on the stream, {args.repeats} repeats after 2 warm-up "
             "runs.  Median (min .. max).", "",
             f"Whole trunk with its input stage (128 x 128 frames resized to 224 x 224), batch {L['batch']}: {t['median_ms']:.2f} ms "
             f"({t['min_ms']:.2f} .. {t['max_ms']:.2f}) = **{L['ms_per_image']:.2f} ms per 224 x 224 image**, {L['gflop_per_image']:.1f} GFLOP per image, "
             f"**{100 * L['fraction_of_peak']:.1f} % of the {PEAK_TFLOPS:.0f} TFLOP/s fp32-MFMA peak** (pools and the input stage included in the time).", "",
             "Per layer: `i2v_vgg_conv_unit` END TO END (host weight packing, upload, launch, stream synchronise) -- an upper bound of the kernel's "
             "time, dominated by the packing for the wide layers; the fraction of the peak it implies is a lower bound.", "",
             "| layer | Cin | Cout | map | GFLOP | unit call ms | >= fraction of peak |", "|---|---|---|---|---|---|---|"]
    for r in L["layers"]:
        u = r["unit_call"]
        lines.append(f"| {r['layer']} | {r['cin']} | {r['cout']} | {r['side']} x {r['side']} | {r['gflop']:.1f} | {u['median_ms']:.2f} ({u['min_ms']:.2f} .. "
                     f"{u['max_ms']:.2f}) | {100 * r['gflop'] * 1e9 / (u['median_ms'] * 1e-3) / (PEAK_TFLOPS * 1e12):.1f} % |")
    lines += ["", "| LPIPS.forward, 10 image pairs | ms |", "|---|---|"]
    for k in ("64", "128"):
        u = res[k]["lpips"]
        lines.append(f"| {k} x {k} | {u['median_ms']:.2f} ({u['min_ms']:.2f} .. {u['max_ms']:.2f}) |")
    with open(os.path.join(out, "vgg_ab.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", os.path.join(out, "vgg_ab.md"))


if __name__ == "__main__":
    main()
