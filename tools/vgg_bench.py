"""Timing of the native VGG-16 trunk and of LPIPS on one MI355X -> profiles/vgg_ab.md (+ .json).

  python tools/vgg_bench.py [--backward] [--repeats 5] [--batch 5] [--out DIR] [--step-timeout 240]

Single-process measurements, each GPU step in a child process of its own under its own ``timeout`` (a step that does not end clean stops
the script; nothing more is started on the GPU):
  * ``layers``: ms of every convolution of the trunk at the shape it has behind a 224 x 224 input (``i2v_native.NativeVGG.features`` is
    timed as a whole; the layers one by one through ``i2v_vgg_conv_unit``, end to end: an upper bound), the fraction of the 157 TFLOP/s
    fp32-MFMA peak, and ms per 224 x 224 image for the whole trunk with its input stage;
  * ``lpips``: ms of ``LPIPS.forward`` on 10 image pairs at 64 x 64 and at 128 x 128.
  * ``--backward`` (-> profiles/lpips_grad_ab.md): ms of LPIPS forward + backward (``LPIPS(x0, x1).mean().backward()``, the gradient at the
    second argument as in the stage-1 loss) for 160 frames at 64 x 64 and for 192 frames at 128 x 128 -- the frames per step of the
    stage-1 configs -- next to the torch-op form of the same network (``F.conv2d`` / ``relu`` / ``max_pool2d`` and the LPIPS formula in
    fp32 with autograd) on the same GPU in the same process, the two alternating; the two gradients are compared.  A record: this path
    has no number at the parent commit.
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


def _torch_lpips(sd, lin, x0, x1):
    """The torch-op form: vgg_common's oracle graph in fp32 on the device (the reference module's arithmetic)."""
    import torch
    import torch.nn.functional as F
    import vgg_common as vc
    shift, scale = (torch.tensor(v, device=x0.device).view(1, 3, 1, 1) for v in (vc.LPIPS_SHIFT, vc.LPIPS_SCALE))
    val = 0
    feats = []
    for x in (x0, x1):
        h, taps = (x - shift) / scale, []
        for idx, _, _ in vc.CONVS:
            h = torch.relu(F.conv2d(h, sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"], padding=1))
            if idx in vc.TAP_AFTER:
                taps.append(h)
            if idx in vc.POOL_AFTER:
                h = F.max_pool2d(h, 2, 2)
        feats.append(taps)
    for k, (a, b) in enumerate(zip(*feats)):
        na = a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt((b ** 2).sum(1, keepdim=True)) + 1e-10)
        val = val + (((na - nb) ** 2) * lin[k].view(1, -1, 1, 1)).sum(1, keepdim=True).mean((2, 3), keepdim=True)
    return val


def step_backward(frames, side, repeats):
    import torch
    import vgg_common as vc
    m = _models(True)
    sd = {k: torch.from_numpy(v).cuda() for k, v in vc.vgg_state_dict(1).items()}
    lin = [torch.from_numpy(v).flatten().cuda() for v in vc.lin_state_dict(2).values()]
    a = torch.from_numpy(vc.clips(5, frames, 1, side, side))[:, 0].contiguous().cuda()
    b = (0.7 * a + 0.3 * torch.from_numpy(vc.clips(6, frames, 1, side, side))[:, 0].cuda()).contiguous()
    grads = {}

    def native():
        x1 = b.clone().requires_grad_(True)
        m(a, x1).mean().backward()
        grads["native"] = x1.grad

    def torch_ops():
        x1 = b.clone().requires_grad_(True)
        _torch_lpips(sd, lin, a, x1).mean().backward()
        grads["torch"] = x1.grad

    def forward_only():
        with torch.no_grad():
            m(a, b)
    for fn in (native, torch_ops, forward_only):      # every shape warm before any window
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rel = float((grads["native"].double() - grads["torch"].double()).norm() / grads["torch"].double().norm())
    ms = {"native": [], "torch": [], "forward": []}
    for _ in range(repeats):                           # alternating: a drift of the machine hits all three alike
        for name, fn in (("native", native), ("torch", torch_ops), ("forward", forward_only)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    stat = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "repeats": len(v)} for k, v in ms.items()}
    # which of the two is right: float64 on the CPU for the first two pairs, its ReLU masks and pool arg-max those of the native run
    # (tests/lpips_grad_common.py: the gradient is discontinuous where a pre-activation crosses zero)
    import lpips_grad_common as lg
    x1 = b[:2].clone().requires_grad_(True)
    out = m(a[:2], x1)
    acts = [lg.to_nchw(t) for t in out.grad_fn.saved[1].activations()]
    out.mean().backward()
    t1 = b[:2].clone().requires_grad_(True)
    _torch_lpips(sd, lin, a[:2], t1).mean().backward()
    y1 = b[:2].cpu().double().requires_grad_(True)
    val, _, side1 = lg.lpips_masked(vc.vgg_state_dict(1), vc.lin_state_dict(2), a[:2].cpu().double(), y1, None, acts)
    val.mean().backward()
    vs64 = {"native": max(vc.rel_l2_rows(x1.grad.cpu(), y1.grad)), "torch": max(vc.rel_l2_rows(t1.grad.cpu(), y1.grad)),
            "mask_differences_native_vs_float64": lg.fragile_units(side1[1], acts)[0]}
    print(json.dumps({"device_name": torch.cuda.get_device_name(0), "frames": frames, "side": side, "grad_rel_l2_native_vs_torch": rel,
                      "grad_rel_l2_vs_float64_first_two_pairs": vs64,
                      "peak_alloc_mb": torch.cuda.max_memory_allocated() / 2 ** 20, **stat}))


BACKWARD_SHAPES = ((160, 64), (192, 128))      # (frames, side): the frames one stage-1 step puts through LPIPS at 64 x 64 and at 128 x 128


def main_backward(args):
    res = []
    for frames, side in BACKWARD_SHAPES:
        r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", f"bwd:{frames}:{side}",
                            "--repeats", str(args.repeats)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"vgg_bench: the backward step at {frames} x {side} ended with status {r.returncode}; nothing more is run")
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(res[-1], flush=True)
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    fmt = lambda u: f"{u['median_ms']:.2f} ({u['min_ms']:.2f} .. {u['max_ms']:.2f})"  # noqa: E731
    lines = ["# LPIPS as a loss: forward + backward, native against the torch-op form", "",
             f"Device: {res[0]['device_name']}.  `tools/vgg_bench.py --backward`, one process per shape, events on the stream around one whole call "
             f"(`LPIPS(x0, x1).mean().backward()`, the gradient at `x1`; host work of the call included), {args.repeats} repeats after 2 warm-up runs "
             "of every variant, the variants alternating inside each repeat.  Median (min .. max) in ms.  The torch-op form is the same "
             "network written with `F.conv2d` / `relu` / `max_pool2d` and the LPIPS formula in fp32 with autograd, on the same GPU.  A record, "
             "not a gate: this path did not exist at the parent commit.", "",
             "| frames | size | native fwd + bwd | torch ops fwd + bwd | torch / native | native forward alone (no grad) | gradient rel-L2 native vs torch "
             "| vs float64: native | vs float64: torch ops |", "|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['frames']} | {r['side']} x {r['side']} | {fmt(r['native'])} | {fmt(r['torch'])} | "
                     f"{r['torch']['median_ms'] / r['native']['median_ms']:.2f} x | {fmt(r['forward'])} | {r['grad_rel_l2_native_vs_torch']:.1e} | "
                     f"{r['grad_rel_l2_vs_float64_first_two_pairs']['native']:.1e} | {r['grad_rel_l2_vs_float64_first_two_pairs']['torch']:.1e} |")
    lines += ["", "vs float64: the worst relative L2 per image of the gradient of the first two pairs against float64 torch on the CPU whose ReLU masks "
              "and pool arg-max are those of the native run (`tests/lpips_grad_common.py`).  The two frames of a pair are close (x1 = 0.7 x0 + 0.3 noise), so "
              "the head's difference of normalised features cancels and magnifies whatever error the features carry."]
    lines += ["", "Not measured: per-kernel times of the backward pass (no profiler run was made), memory traffic, any share of a peak."]
    with open(os.path.join(out, "lpips_grad_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out, "lpips_grad_ab.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", os.path.join(out, "lpips_grad_ab.md"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=5, help="images per trunk forward (one group of the diversity score: n_realiz)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of vgg_ab.md / vgg_ab.json")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--backward", action="store_true", help="time LPIPS forward + backward instead -> lpips_grad_ab.md / .json")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "layers":
        return step_layers(args.batch, args.repeats)
    if args.step and args.step.startswith("bwd:"):
        return step_backward(*map(int, args.step.split(":")[1:]), args.repeats)
    if args.backward:
        return main_backward(args)
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
