"""Times the spatial discriminator's part of the stage-1 step and writes profiles/patch_disc_ab.md.

Two arms on the same GPU, the same seeded parameters and frames, ndf 64, 20 frames of 64 x 64 and of 128 x 128:
  native   stage1_VAE.modules.patch_disc.NLayerDiscriminator through i2v_train.PatchDiscTrainer: one ``step`` (two forwards, hinge, two
           backwards, fused Adam) and one ``generator_loss``
  torch    the same network from stock torch ops (nn.Conv2d under torch.nn.utils.spectral_norm, ActNorm as the reference writes it,
           autograd, torch.optim.Adam) doing the same two things
The arms alternate, round by round, in ONE process; each timed window is ``--iters`` calls between two device events after ``--warmup``
calls; the table gives the median and the minimum over the rounds, and a sentence per row says which arm was faster.  A window of 20
calls is 20 to 120 ms, short of a second: the rounds' spread (median against minimum) is printed so that it can be judged.  A record, not a
gate.  The whole file is written by this tool; nothing in it is edited by hand.

    python tools/patch_disc_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/patch_disc_ab.md]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image2video-synthesis-using-cinns_amd"))

CFG = {"in_channels": 3, "ndf": 64, "n_layers": 3, "use_actnorm": True, "spectral_norm": True}


class TorchActNorm(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.loc, self.scale = nn.Parameter(torch.zeros(1, c, 1, 1)), nn.Parameter(torch.ones(1, c, 1, 1))
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))
        self.done = False       # (the reference reads the buffer with .item() every forward; the arm is spared that sync)

    def forward(self, x):
        if self.training and not self.done:
            with torch.no_grad():
                flat = x.permute(1, 0, 2, 3).reshape(x.shape[1], -1)
                self.loc.data.copy_(-flat.mean(1).view(1, -1, 1, 1))
                self.scale.data.copy_(1 / (flat.std(1).view(1, -1, 1, 1) + 1e-6))
            self.initialized.fill_(1)
            self.done = True
        return self.scale * (x + self.loc)


def torch_disc(native_module):
    """The torch-op form with the native module's parameters."""
    sn = torch.nn.utils.spectral_norm
    seq, c = [sn(nn.Conv2d(3, 64, 4, 2, 1)), nn.LeakyReLU(0.2, True)], 64
    for cout, stride in ((128, 2), (256, 2), (512, 1)):
        seq += [sn(nn.Conv2d(c, cout, 4, stride, 1)), TorchActNorm(cout), nn.LeakyReLU(0.2, True)]
        c = cout
    seq += [sn(nn.Conv2d(c, 1, 4, 1, 1))]
    net = nn.Module()
    net.main = nn.Sequential(*seq)
    net.load_state_dict(native_module.state_dict())
    net.forward = lambda x: net.main(x)
    return net


def hinge(fake, real):
    return (torch.relu(1.0 - real).mean() + torch.relu(1.0 + fake).mean()) / 2


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "patch_disc_ab.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patch_disc_bench: no HIP device; nothing is measured on a CPU")
    import i2v_train
    from stage1_VAE.modules.patch_disc import NLayerDiscriminator

    rows = []
    for size in (64, 128):
        torch.manual_seed(4300)
        nat = NLayerDiscriminator(dict(CFG)).cuda().train()
        ref = torch_disc(nat).cuda().train()
        g = torch.Generator(device="cuda").manual_seed(4301)
        real = torch.randn(20, 3, size, size, device="cuda", generator=g).clamp(-1, 1)
        fake = (0.5 * torch.randn(20, 3, size, size, device="cuda", generator=g) + 0.3).clamp(-1, 1)
        trainer = i2v_train.PatchDiscTrainer(nat)
        opt = torch.optim.Adam(ref.parameters(), lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5)

        def torch_step():
            loss = hinge(ref(fake), ref(real))
            opt.zero_grad()
            loss.backward()
            opt.step()

        def torch_gen():
            x = fake.detach().requires_grad_(True)
            return torch.autograd.grad(-ref(x).mean(), x)[0]

        arms = {"step": {"native": lambda: trainer.step(fake, real), "torch": torch_step},
                "generator_loss": {"native": lambda: trainer.generator_loss(fake), "torch": torch_gen}}
        for what, pair in arms.items():
            times = {k: [] for k in pair}
            for fn in pair.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for k, fn in pair.items():
                    times[k].append(timed(fn, args.iters))
            rows.append((size, what, times))
            print(size, what, {k: f"{statistics.median(v):.3f} ms" for k, v in times.items()}, flush=True)

    lines = ["# Patch discriminator: native path against the torch-op form", "",
             f"`tools/patch_disc_bench.py --rounds {args.rounds} --iters {args.iters} --warmup {args.warmup}` on the device the runtime names \"{torch.cuda.get_device_name(0)}\""
             f" ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', 'gfx?').split(':')[0]}, {torch.cuda.get_device_properties(0).multi_processor_count} compute units); ndf 64, 20 frames;",
             "both arms in one process, alternating round by round; each figure is the time of one call in ms (device events around",
             f"{args.iters} calls), median and minimum over the rounds.  `step` = two forwards, hinge, two backwards, Adam; `generator_loss` = one forward and the",
             "gradient at the frames.  A record of what was measured, not a gate.", "",
             "| frames | call | native median | native min | torch median | torch min | native / torch (median) |", "|---|---|---|---|---|---|---|"]
    for size, what, t in rows:
        n, r = t["native"], t["torch"]
        lines.append(f"| {size} x {size} | {what} | {statistics.median(n):.3f} | {min(n):.3f} | {statistics.median(r):.3f} | {min(r):.3f} | "
                     f"{statistics.median(n) / statistics.median(r):.2f} |")
    lines += ["", "What came out:"]
    for size, what, t in rows:
        ratio = statistics.median(t["native"]) / statistics.median(t["torch"])
        lines.append(f"- {size} x {size}, `{what}`: the native path takes {ratio:.2f} of the torch-op form's time ({'native' if ratio < 1 else 'torch-op form'} faster).")
    lines += ["", f"Each window is {args.iters} calls ({args.iters * min(min(t['native']) for _, _, t in rows):.0f} ms at the least): short, so read a difference against the",
              "distance between a row's median and minimum.  Where the kernel time goes: DESIGN.md section 12.5."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
