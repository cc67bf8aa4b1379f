"""Times the temporal discriminator's step WITH the gradient penalty (w_GP = 10) and writes profiles/temporal_disc_gp_ab.md.

Shipped widths [64, 64, 128, 256, 512], 10 fake + 10 real clips of 12 frames, at 64 x 64 (stride_s [1, 1, 2, 2]) and at 128 x 128
(stride_s [1, 2, 2, 2]); the same seeded parameters and clips for every arm, all arms on the same GPU in ONE process, alternating round by
round:
  native-gp     i2v_train.TemporalDiscPenaltyTrainer.step: two saved forwards, hinge, two backwards, gp_backward (the clips' gradient, the
                tangent forward, the reverse pass over the pair), fused Adam
  native-plain  i2v_train.TemporalDiscTrainer.step, whose code this feature does not touch: the same step without the penalty
  torch-gp      the torch-op form of the same network (tools/temporal_disc_bench.TorchDisc) with autograd's double backward
                (``create_graph=True``), torch.optim.Adam
and, on the native path alone, ``penalty-value``: TemporalDiscTrainer.gradient_penalty, one saved forward and the input-gradient backward
that forms g (the penalty's VALUE, what the project could do before).
Each timed window is ``--iters`` calls between two device events after ``--warmup`` calls; the table gives the median and the minimum
over the rounds.  A record, not a gate: this path has no earlier number.

The split of gp_backward by kernel comes from a kernel trace taken in a run of its own (tracing slows the host; no end-to-end figure is
taken from it):

    python tools/temporal_disc_gp_bench.py --phase time --json gp_timing.json
    rocprofv3 --kernel-trace --stats -f csv -d gp_prof -o gp -- python tools/temporal_disc_gp_bench.py --phase profile
    python tools/temporal_disc_gp_bench.py --phase write --json gp_timing.json --trace 'gp_prof/**/*kernel_trace.csv' [--out ...]

``--phase profile`` runs gp_backward alone, ``--profile-calls`` times after a warm-up, at 64 x 64; ``--phase write`` cuts the trace at
the marker kernels (the tangent clip's writer starts the tangent forward, the head's dual kernel starts the reverse pass) and writes the
file.  The whole file is written by this tool; nothing in it is edited by hand."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image2video-synthesis-using-cinns_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

BATCH, FRAMES, W_GP = 10, 12, 10.0
CASES = ((64, [1, 1, 2, 2]), (128, [1, 2, 2, 2]))


def setup(size, stride_s, torch_arm=True):
    import torch
    from temporal_disc_bench import TorchDisc, cfg_of
    from stage1_VAE.modules.resnet3D import Discriminator
    cfg = cfg_of(stride_s)
    torch.manual_seed(6400)
    nat = Discriminator(cfg)
    sd = {k: v.clone() for k, v in nat.state_dict().items()}
    ref = None
    if torch_arm:
        ref = TorchDisc(cfg)
        ref.load_state_dict(sd)
        ref = ref.cuda().train()
    g = torch.Generator(device="cuda").manual_seed(6401)
    real = torch.randn(BATCH, 3, FRAMES, size, size, device="cuda", generator=g).clamp(-1, 1)
    fake = (0.5 * torch.randn(BATCH, 3, FRAMES, size, size, device="cuda", generator=g) + 0.3).clamp(-1, 1)
    return cfg, sd, nat.cuda().train(), ref, fake, real


def phase_time(args):
    import torch
    import i2v_train
    from temporal_disc_bench import hinge, timed
    from stage1_VAE.modules.resnet3D import Discriminator
    rows = []
    for size, stride_s in CASES:
        cfg, sd, nat, ref, fake, real = setup(size, stride_s)
        plain = Discriminator(cfg)
        plain.load_state_dict(sd)
        plain = plain.cuda().train()
        tr_gp = i2v_train.TemporalDiscPenaltyTrainer(nat, w_GP=W_GP)
        tr_plain = i2v_train.TemporalDiscTrainer(plain)
        opt = torch.optim.Adam(ref.parameters(), lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5)

        def torch_gp():
            x = real.detach().requires_grad_(True)
            pred_f, pred_r = ref(fake)[0], ref(x)[0]
            g = torch.autograd.grad(pred_r.mean(), x, create_graph=True)[0]
            loss = hinge(pred_f, pred_r) + W_GP * g.pow(2).reshape(BATCH, -1).sum(1).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()

        # the two forms compute the same penalty: compared once, in eval mode, before anything is trained
        nat.eval(), ref.eval()
        x = real.detach().requires_grad_(True)
        g = torch.autograd.grad(ref(x)[0].mean(), x)[0]
        with torch.no_grad():
            agree = float(nat.forward_with_penalty(real)[2]) / float(g.pow(2).reshape(BATCH, -1).sum(1).mean()) - 1.0
        nat.train(), ref.train()
        h = nat._handle()
        n, _, t, hh, ww = real.shape
        sizes = {"saved": h.saved_bytes(n, t, hh, ww), "gp_saved": h.gp_saved_bytes(n, t, hh, ww), "workspace": h.workspace_bytes(n, t, hh, ww),
                 "gp_workspace": h.gp_workspace_bytes(n, t, hh, ww)}
        arms = {"native-gp": lambda: tr_gp.step(fake, real), "native-plain": lambda: tr_plain.step(fake, real), "torch-gp": torch_gp,
                "penalty-value": lambda: tr_plain.gradient_penalty(real)}
        times = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn, args.iters))
        rows.append({"size": size, "times": times, "agree": agree, "sizes": sizes})
        print(size, {k: f"{statistics.median(v):.3f} ms" for k, v in times.items()}, f"L_GP native / torch - 1 = {agree:.2e}", sizes, flush=True)
    prop = torch.cuda.get_device_properties(0)
    meta = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", "gfx?").split(":")[0], "cus": prop.multi_processor_count,
            "rounds": args.rounds, "iters": args.iters, "warmup": args.warmup}
    with open(args.json, "w") as f:
        json.dump({"meta": meta, "rows": rows}, f)
    print("wrote", args.json)


def phase_profile(args):
    """gp_backward alone at 64 x 64, for the kernel trace"""
    import torch
    size, stride_s = CASES[0]
    _, _, nat, _, _, real = setup(size, stride_s, torch_arm=False)
    grads = {k: torch.zeros_like(p) for k, p in nat.named_parameters()}
    _, _, saved = nat._run(real, save=True, grads=grads, want_fmaps=False)
    h = nat._handle(grads)
    for _ in range(2 + args.profile_calls):
        h.gp_backward(saved, tuple(real.shape), scale=W_GP, accumulate=False)
    torch.cuda.synchronize()
    print("profiled", args.profile_calls, "calls of gp_backward behind 2 warm-up calls")


PHASES = ("clip gradient (head, reverse pass to the clips, L_GP)", "tangent forward", "reverse pass over the pair")


def split_trace(pattern, calls):
    """The kernel trace of --phase profile -> per phase and per kernel family the device time of ONE gp_backward call, in ms (the mean over
    the last ``calls`` calls), or None where no trace is found"""
    paths = sorted(glob.glob(pattern, recursive=True))
    if not paths:
        return None
    ev = []
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("KernelName") or ""
                try:
                    ev.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), name))
                except (KeyError, ValueError):
                    continue
    ev.sort()
    starts = [i for i, e in enumerate(ev) if "d3g_seed_kernel" in e[2]]
    if len(starts) < calls:
        return None
    ev = ev[starts[-calls]:]
    phase, fam = 0, {}
    tot = [0.0, 0.0, 0.0]
    for s, e, name in ev:
        if "d3g_seed_kernel" in name:
            phase = 0
        elif "d3g_tangent_input_kernel" in name:
            phase = 1
        elif "d3g_head_dual_kernel" in name:
            phase = 2
        ms = (e - s) / 1e6 / calls
        tot[phase] += ms
        key = ("GroupNorm of the pair (d3g_gn_*)" if "d3g_gn_" in name else "GroupNorm backward of the clip gradient (d3_gn_*)" if "d3_gn_" in name
               else "conv forward (tc_conv)" if "tc_conv_kernel" in name else "input gradient (tc_dgrad)" if "tc_dgrad_kernel" in name
               else "weight gradient (tc_wgrad)" if "tc_wgrad_kernel" in name else "wgrad finish and projection (tc_finish_*)" if "tc_finish" in name
               else "pool, head, seeds, sums and the rest")
        fam[key] = fam.get(key, 0.0) + ms
    return {"phases": tot, "families": fam, "launches": len(ev) // calls}


def phase_write(args):
    with open(args.json) as f:
        data = json.load(f)
    meta, rows = data["meta"], data["rows"]
    split = split_trace(args.trace, args.profile_calls) if args.trace else None
    med = statistics.median
    lines = ["# Temporal discriminator: the step with the gradient penalty (w_GP = 10)", "",
             f"`python tools/temporal_disc_gp_bench.py --phase time --rounds {meta['rounds']} --iters {meta['iters']} --warmup {meta['warmup']}` on the device the "
             f"runtime names \"{meta['device']}\" ({meta['arch']}, {meta['cus']} compute units); widths [64, 64, 128, 256, 512], {BATCH} fake + {BATCH} real clips of",
             f"{FRAMES} frames; all arms in one process, alternating round by round; each figure is the time of one call in ms (device events around",
             f"{meta['iters']} calls), median and minimum over the rounds.  `native-gp` = TemporalDiscPenaltyTrainer.step; `native-plain` = TemporalDiscTrainer.step",
             "(the step without the penalty, code untouched by this feature); `torch-gp` = the torch-op form of the same network with autograd's double",
             "backward and torch.optim.Adam; `penalty-value` = TemporalDiscTrainer.gradient_penalty (one saved forward and the input-gradient backward that",
             "forms g: the penalty's value alone).  The native arms compute in exact fp32",
             "with fixed summation orders.  A record of what was measured, not a gate: this path has no earlier number.", "",
             "| clips | arm | median | min |", "|---|---|---|---|"]
    for r in rows:
        for k, v in r["times"].items():
            lines.append(f"| 2 x {BATCH} x {FRAMES} x {r['size']} x {r['size']} | {k} | {med(v):.3f} | {min(v):.3f} |")
    lines += ["", "| clips | native-gp / native-plain | expectation | native-gp / torch-gp | saved bytes (one forward) | gp_saved bytes | workspace bytes | gp workspace bytes |",
              "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        t, s = r["times"], r["sizes"]
        lines.append(f"| {r['size']} x {r['size']} | {med(t['native-gp']) / med(t['native-plain']):.2f} | about 2 (6 F -> 12 F of conv work, plus the GroupNorm passes) | "
                     f"{med(t['native-gp']) / med(t['torch-gp']):.2f} | {s['saved']} | {s['gp_saved']} | {s['workspace']} | {s['gp_workspace']} |")
    lines += ["", "What came out:"]
    for r in rows:
        t = r["times"]
        extra = med(t["native-gp"]) - med(t["native-plain"])
        lines.append(f"- {r['size']} x {r['size']}: the penalty adds {extra:.3f} ms to the plain step's {med(t['native-plain']):.3f} ms (ratio "
                     f"{med(t['native-gp']) / med(t['native-plain']):.2f} against the expected 2); the penalty's value alone (a forward and the backward to the clips) takes {med(t['penalty-value']):.3f} ms; the "
                     f"native step takes {med(t['native-gp']) / med(t['torch-gp']):.2f} of the torch-op form's time; the two forms' L_GP differed by {r['agree']:.1e} "
                     "relative before training.")
    lines += ["", f"## Where gp_backward's kernel time goes ({rows[0]['size']} x {rows[0]['size']})", ""]
    if split is None:
        lines.append("Not measured: no kernel trace was given to `--phase write`.")
    else:
        total = sum(split["phases"])
        lines += [f"From `rocprofv3 --kernel-trace --stats -f csv -- python tools/temporal_disc_gp_bench.py --phase profile`, a run of its own: device time of the "
                  f"kernels of one `gp_backward` call (mean over {args.profile_calls} calls, {split['launches']} launches per call), cut at the marker kernels.  Kernel",
                  "time only: the gaps between launches are not in it, so the sum is below the call's end-to-end time.", "",
                  "| part | ms | share |", "|---|---|---|"]
        lines += [f"| {n} | {v:.3f} | {100 * v / total:.1f} % |" for n, v in zip(PHASES, split["phases"])]
        lines += [f"| all kernels of the call | {total:.3f} | 100 % |", "", "| kernel family (all three parts) | ms | share |", "|---|---|---|"]
        lines += [f"| {k} | {v:.3f} | {100 * v / total:.1f} % |" for k, v in sorted(split["families"].items(), key=lambda kv: -kv[1])]
    lines += ["", "The method, the saved layout and what is left out: DESIGN.md section 12.6.1."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=("time", "profile", "write"), default="time")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-calls", type=int, default=3)
    ap.add_argument("--json", default="temporal_disc_gp_timing.json")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_disc_gp_ab.md"))
    args = ap.parse_args()
    if args.phase == "write":
        return phase_write(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("temporal_disc_gp_bench: no HIP device; nothing is measured on a CPU")
    (phase_time if args.phase == "time" else phase_profile)(args)


if __name__ == "__main__":
    main()
