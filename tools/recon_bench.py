"""Timing of the reconstruction metrics (csrc/i2v_recon.hip) on one MI355X -> profiles/recon_ab.md (+ .json).

  python tools/recon_bench.py [--windows 7] [--calls 200] [--out DIR]

Two variants on the same seeded frames, on the same GPU, in one process:
  * ``native``: ``stage1_VAE.modules.loss.recon_metrics`` (range pass + statistics pass, float64), then ONE read-back of the four scalars;
  * ``torch``: the torch-op restatement of the pytorch_lightning 1.2.7 formula in fp32 (reflect pad, concatenation of the five maps, grouped
    ``conv2d``, the elementwise SSIM map, crop, mean; PSNR; L1), then ONE read-back of the same four scalars (the reference reads them
    back one by one).
Shapes: (64, 16, 3, 64, 64) and (32, 16, 3, 128, 128), (B, T, C, H, W).  A window is ``--calls`` calls between two events; every variant is
warmed up at every shape, then the variants alternate window by window; median and spread over the windows.  The outputs of the variants
are compared on the same inputs before anything is timed.  No number of this path appears in any document of the project unless this
script wrote it."""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "image2video-synthesis-using-cinns_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((64, 16, 3, 64, 64), (32, 16, 3, 128, 128))


def torch_form(p, t):
    """[N, C, H, W] fp32 on the device -> (l1, mse, psnr, ssim) stacked: the library's op sequence."""
    import torch
    import torch.nn.functional as F
    c = p.shape[1]
    d = torch.arange(-5.0, 6.0, device=p.device)
    g = torch.exp(-((d / 1.5) ** 2) / 2)
    g = (g / g.sum()).unsqueeze(0)
    kernel = torch.matmul(g.t(), g).expand(c, 1, 11, 11)
    r = torch.maximum(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * r) ** 2, (0.03 * r) ** 2
    pp, tp = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat([pp, tp, pp * pp, tp * tp, pp * tp]), kernel, groups=c)
    mp, mt, epp, ett, ept = out.chunk(5)
    mpp, mtt, mpt = mp.pow(2), mt.pow(2), mp * mt
    spp, stt, spt = epp - mpp, ett - mtt, ept - mpt
    idx = ((2 * mpt + c1) * (2 * spt + c2)) / ((mpp + mtt + c1) * (spp + stt + c2))
    ssim = idx[..., 5:-5, 5:-5].mean()
    diff = p - t
    mse = (diff * diff).sum() / p.numel()
    psnr = (2 * torch.log(t.max() - t.min()) - torch.log(mse)) * (10 / math.log(10))
    return torch.stack([diff.abs().mean(), mse, psnr, ssim])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of recon_ab.md / recon_ab.json")
    args = ap.parse_args()
    import torch
    import recon_common as rc
    from stage1_VAE.modules import loss as loss_mod
    if not torch.cuda.is_available():
        raise SystemExit("recon_bench: needs a GPU; nothing is measured without one")
    torch.set_grad_enabled(False)

    def native(p, t):
        m = loss_mod.recon_metrics(p, t)
        return torch.stack([m[k] for k in ("l1", "mse", "psnr", "ssim")])

    res = {"device_name": torch.cuda.get_device_name(0), "windows": args.windows, "calls": args.calls, "shapes": []}
    for shape in SHAPES:
        real, gen = rc.pair(1000 + shape[-1], shape, 0.1)
        p5, t5 = real.cuda(), gen.cuda()
        p4, t4 = p5.reshape(-1, *shape[2:]), t5.reshape(-1, *shape[2:])
        variants = {"native": lambda: native(p5, t5).cpu(), "torch": lambda: torch_form(p4, t4).cpu()}
        outs = {k: f() for k, f in variants.items()}
        agree = {"torch_fp32_vs_native": float(((outs["torch"].double() - outs["native"]) / outs["native"]).abs().max())}
        assert agree["torch_fp32_vs_native"] < 1e-3, agree
        for f in variants.values():          # warm-up of every variant at this shape
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.windows):        # the variants alternate window by window
            for k, f in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    f()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / args.calls)
        row = {"shape": list(shape), "agreement": agree,
               "ms_per_call": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)

    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "recon_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Reconstruction metrics (PSNR, SSIM, L1): measured figures", "",
             f"Device: {res['device_name']}.  `tools/recon_bench.py`: one process, events on the stream around {args.calls} calls, {args.windows} windows per "
             "variant after 3 warm-up calls, the variants alternating window by window.  ms per call, median (min .. max).  A call ends in one "
             "read-back of the four scalars.", "",
             "`native`: `recon_metrics` (range pass + statistics pass in float64, csrc/i2v_recon.hip).  "
             "`torch`: the torch-op restatement of the pytorch_lightning 1.2.7 formula in fp32 on the same GPU.", "",
             "| shape (B, T, C, H, W) | native | torch fp32 | torch / native | fp32 torch vs native (rel.) |", "|---|---|---|---|---|"]
    for row in res["shapes"]:
        m = row["ms_per_call"]
        cell = lambda k: f"{m[k]['median']:.3f} ({m[k]['min']:.3f} .. {m[k]['max']:.3f})"   # noqa: E731
        lines.append(f"| {tuple(row['shape'])} | {cell('native')} | {cell('torch')} | {m['torch']['median'] / m['native']['median']:.2f} x | "
                     f"{row['agreement']['torch_fp32_vs_native']:.1e} |")
    with open(os.path.join(out, "recon_ab.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", os.path.join(out, "recon_ab.md"))


if __name__ == "__main__":
    main()
