"""Times the temporal discriminator's part of the stage-1 step and writes profiles/temporal_disc_ab.md.

Two arms on the same GPU, the same seeded parameters and clips, the shipped widths [64, 64, 128, 256, 512], 12 frames: B = 10 at 64 x 64
(stride_s [1, 1, 2, 2]) and B = 7 at 128 x 128 (stride_s [1, 2, 2, 2]):
  native   stage1_VAE.modules.resnet3D.Discriminator through i2v_train.TemporalDiscTrainer: one ``step`` (two forwards, hinge, two
           backwards, fused Adam) and one ``generator_loss`` (two forwards, hinge + feature-map loss, the gradient at the generated clips)
  torch    the same network from stock torch ops (nn.Conv3d, plain or under torch.nn.utils.spectral_norm, nn.GroupNorm, nn.MaxPool3d,
           autograd, torch.optim.Adam) doing the same two things
The arms alternate, round by round, in ONE process, back to back; each timed window is ``--iters`` calls between two device events after
``--warmup`` calls (12 calls are 0.25 to 1.9 s); the table gives the median and the minimum over the rounds.  Both arms train while
they are timed, each on its own copy of the parameters: the work per call does not depend on the values.  A record, not a gate: this
path has no earlier number and no ratio is required.  The whole file is written by this tool; nothing in it is edited by hand.

    python tools/temporal_disc_bench.py [--rounds 5] [--iters 12] [--warmup 3] [--out profiles/temporal_disc_ab.md]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image2video-synthesis-using-cinns_amd"))

CASES = ((10, 64, [1, 1, 2, 2]), (7, 128, [1, 2, 2, 2]))


def cfg_of(stride_s):
    return {"res_type_encoder": "resnet18", "use_max_pool": True, "spectral_norm": True, "channels": [64, 64, 128, 256, 512],
            "stride_t": [2, 2, 2, 2], "stride_s": stride_s}


def conv(cin, cout, st, ss, spectral):
    c = nn.Conv3d(cin, cout, 3, (st, ss, ss), 1, bias=False)
    return torch.nn.utils.spectral_norm(c) if spectral else c


class TorchBlock(nn.Module):
    def __init__(self, cin, cout, st, ss, spectral, down):
        super().__init__()
        self.conv1, self.bn1 = conv(cin, cout, st, ss, spectral), nn.GroupNorm(16, cout)
        self.conv2, self.bn2 = conv(cout, cout, 1, 1, spectral), nn.GroupNorm(16, cout)
        if down:
            self.downsample = nn.Sequential(conv(cin, cout, st, ss, True), nn.GroupNorm(16, cout))

    def forward(self, x):
        out = self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x)))))
        return torch.relu(out + (self.downsample(x) if hasattr(self, "downsample") else x))


class TorchDisc(nn.Module):
    """The torch-op form of the network, with the native module's state-dict keys."""

    def __init__(self, cfg):
        super().__init__()
        ch = cfg["channels"]
        self.conv1, self.norm1 = nn.Conv3d(3, ch[0], (3, 7, 7), (1, 2, 2), (1, 3, 3), bias=False), nn.GroupNorm(16, ch[0])
        self.maxpool = nn.MaxPool3d(3, (1, 2, 2), 1)
        layers, cin = [], ch[0]
        for cout, st, ss in zip(ch[1:], cfg["stride_t"], cfg["stride_s"]):
            layers.append(nn.Sequential(TorchBlock(cin, cout, st, ss, cfg["spectral_norm"], ss != 1 or cin != cout or st != 1),
                                        TorchBlock(cout, cout, 1, 1, False, False)))
            cin = cout
        self.layer = nn.Sequential(*layers)
        self.fc = nn.Linear(cin, 1, bias=False)

    def forward(self, x):
        x = self.maxpool(torch.relu(self.norm1(self.conv1(x))))
        fmaps = []
        for lay in self.layer:
            x = lay(x)
            fmaps.append(x)
        return self.fc(x.mean((2, 3, 4))), fmaps


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_disc_ab.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_disc_bench: no HIP device; nothing is measured on a CPU")
    import i2v_train
    from stage1_VAE.modules.resnet3D import Discriminator

    rows = []
    for batch, size, stride_s in CASES:
        cfg = cfg_of(stride_s)
        torch.manual_seed(6300)
        nat = Discriminator(cfg).cuda().train()
        ref = TorchDisc(cfg)
        ref.load_state_dict(nat.state_dict())
        ref = ref.cuda().train()
        g = torch.Generator(device="cuda").manual_seed(6301)
        real = torch.randn(batch, 3, 12, size, size, device="cuda", generator=g).clamp(-1, 1)
        fake = (0.5 * torch.randn(batch, 3, 12, size, size, device="cuda", generator=g) + 0.3).clamp(-1, 1)
        with torch.no_grad():           # the two arms are the same network: one eval-mode forward each, before anything is trained
            nat.eval(), ref.eval()
            agree = float((nat(fake)[0] - ref(fake)[0]).abs().max())
            nat.train(), ref.train()
        trainer = i2v_train.TemporalDiscTrainer(nat)
        opt = torch.optim.Adam(ref.parameters(), lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5)

        def torch_step():
            loss = hinge(ref(fake)[0], ref(real)[0])
            opt.zero_grad()
            loss.backward()
            opt.step()

        def torch_gen():
            x = fake.detach().requires_grad_(True)
            (pf, ff), (_, fr) = ref(x), ref(real)
            loss = -pf.mean() + 10 * sum((a - b).abs().mean() for a, b in zip(ff, fr)) / 4
            return torch.autograd.grad(loss, x)[0]

        arms = {"step": {"native": lambda: trainer.step(fake, real), "torch": torch_step},
                "generator_loss": {"native": lambda: trainer.generator_loss(fake, real), "torch": torch_gen}}
        for what, pair in arms.items():
            times = {k: [] for k in pair}
            for fn in pair.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for k, fn in pair.items():
                    times[k].append(timed(fn, args.iters))
            rows.append((batch, size, what, times, agree))
            print(batch, size, what, {k: f"{statistics.median(v):.3f} ms" for k, v in times.items()}, f"max |pred difference| before training {agree:.2e}", flush=True)

    prop = torch.cuda.get_device_properties(0)
    lines = ["# Temporal discriminator: native path against the torch-op form", "",
             f"`python tools/temporal_disc_bench.py --rounds {args.rounds} --iters {args.iters} --warmup {args.warmup}` on the device the runtime names "
             f"\"{torch.cuda.get_device_name(0)}\" ({getattr(prop, 'gcnArchName', 'gfx?').split(':')[0]}, {prop.multi_processor_count} compute units);",
             "widths [64, 64, 128, 256, 512], clips of 12 frames; both arms in one process, alternating round by round, back to back; each figure",
             f"is the time of one call in ms (device events around {args.iters} calls), median and minimum over the rounds.  `step` = two forwards, hinge,",
             "two backwards, Adam; `generator_loss` = two forwards, hinge + feature-map loss and the gradient at the generated clips.  The native arm",
             "computes in exact fp32 with fixed summation orders; the torch arm uses whatever the framework's convolution library picks.  A record",
             "of what was measured, not a gate: this path has no earlier number.", "",
             "| clips | call | native median | native min | torch median | torch min | native / torch (median) |", "|---|---|---|---|---|---|---|"]
    for batch, size, what, t, _ in rows:
        n, r = t["native"], t["torch"]
        lines.append(f"| {batch} x 12 x {size} x {size} | {what} | {statistics.median(n):.3f} | {min(n):.3f} | {statistics.median(r):.3f} | {min(r):.3f} | "
                     f"{statistics.median(n) / statistics.median(r):.2f} |")
    lines += ["", "What came out:"]
    for batch, size, what, t, agree in rows:
        ratio = statistics.median(t["native"]) / statistics.median(t["torch"])
        lines.append(f"- B = {batch}, {size} x {size}, `{what}`: the native path takes {ratio:.2f} of the torch-op form's time "
                     f"({'native' if ratio < 1 else 'torch-op form'} faster); the two arms' eval-mode logits differed by at most {agree:.1e} before training.")
    lines += ["", "Where the kernel time goes and what is left out: DESIGN.md section 12.6."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
