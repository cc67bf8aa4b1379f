"""Times the training path of one GeneratorBlock (forward + backward) and writes profiles/gblock_train_ab.md.

Two arms on the same GPU, the same seeded parameters and inputs, z = 64, a 64 x 64 start frame, spectral norm on, ``.train()`` mode: the
blocks g_1 (1024 -> 512 at 4 x 16 x 16) and g_3 (256 -> 128 at 16 x 64 x 64) of the BAIR decoder (channel_factor 64):
  native   stage1_VAE.modules.decoder.GeneratorBlock with ``differentiable = True``: the forward with a grad_fn, the loss sum(c out),
           ``backward()`` into x, z and every parameter's ``.grad``
  torch    the same block from stock torch ops (F.conv3d, F.conv2d, F.group_norm, F.instance_norm, F.interpolate, F.linear, the power
           iteration under no_grad, autograd) on copies of the same parameters
Before the timing each arm takes one step and the torch-op form one more in float64: the file states how far each arm's gradients are from
that.  The arms alternate, round by round, in ONE process, back to back; each timed window is ``--iters`` calls between two device events
after ``--warmup`` calls; the table gives the median and the minimum over the rounds.  The native arm is also timed in parts -- the forward
alone and the backward of a frozen module (no weight-gradient launches) -- to say where its time goes.  A record, not a gate: this path
has no earlier number and no ratio is required.  The whole file is written by this tool; nothing in it is edited by hand.

    python tools/gblock_train_bench.py [--rounds 5] [--iters 4] [--warmup 2] [--out profiles/gblock_train_ab.md]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image2video-synthesis-using-cinns_amd"))

#        name  n_in  n_out batch  map
CASES = (("g_1", 1024, 512, 4, (4, 16, 16)), ("g_3", 256, 128, 2, (16, 64, 64)))
Z_DIM, IMG = 64, 64


def torch_forward(p, n_in, n_out, x, z, img):
    """The torch-op form of GeneratorBlock.forward in .train() mode on a dict of the module's state-dict keys."""
    def sn(name):
        w = p[name + ".weight_orig"]
        m = w.reshape(w.shape[0], -1)
        with torch.no_grad():
            u, v = p[name + ".weight_u"], p[name + ".weight_v"]
            v.copy_(F.normalize(m.t() @ u, dim=0, eps=1e-12))
            u.copy_(F.normalize(m @ v, dim=0, eps=1e-12))
        return w / torch.dot(u.clone(), m @ v.clone())

    n_mid = min(n_in, n_out)
    y = F.interpolate(img, size=x.shape[-2:], mode="bilinear", align_corners=True)
    y = F.leaky_relu(F.conv2d(y, p["norm_0.conv.weight"], p["norm_0.conv.bias"], padding=1), 0.2)
    gamma = F.conv2d(y, p["norm_0.conv_gamma.weight"], p["norm_0.conv_gamma.bias"], padding=1).unsqueeze(2)
    beta = F.conv2d(y, p["norm_0.conv_beta.weight"], p["norm_0.conv_beta.bias"], padding=1).unsqueeze(2)
    h = F.leaky_relu(F.group_norm(x, 16) * (1 + gamma) + beta, 0.2)
    h = F.conv3d(h, sn("conv_0"), p["conv_0.bias"], padding=1)
    lin = F.linear(z, p["norm_1.linear.weight"], p["norm_1.linear.bias"])
    h = lin[:, :n_mid, None, None, None] * F.instance_norm(h) + lin[:, n_mid:, None, None, None]
    h = F.conv3d(F.leaky_relu(h, 0.2), sn("conv_1"), p["conv_1.bias"], padding=1)
    xs = F.conv3d(F.group_norm(x, 16, p["norm_s.bn.weight"], p["norm_s.bn.bias"]), sn("conv_s")) if n_in != n_out else x
    return xs + h


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
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gblock_train_ab.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gblock_train_bench: no HIP device; nothing is measured on a CPU")
    from stage1_VAE.modules.decoder import GeneratorBlock

    rows = []
    for name, n_in, n_out, batch, thw in CASES:
        torch.manual_seed(6800)
        nat = GeneratorBlock(n_in, n_out, True, Z_DIM).cuda().train()
        nat.differentiable = True
        frozen = GeneratorBlock(n_in, n_out, True, Z_DIM)
        frozen.load_state_dict(nat.state_dict())
        frozen = frozen.cuda().train().requires_grad_(False)
        frozen.differentiable = True
        start = {k: v.detach().clone() for k, v in nat.state_dict().items()}

        def twin_of(dtype):
            return {k: v.detach().to(dtype).clone().requires_grad_(not k.endswith(("_u", "_v"))) for k, v in start.items()}

        twin = twin_of(torch.float32)
        g = torch.Generator(device="cuda").manual_seed(6801)
        x = torch.randn(batch, n_in, *thw, device="cuda", generator=g).requires_grad_(True)
        z = torch.randn(batch, Z_DIM, device="cuda", generator=g).requires_grad_(True)
        img = torch.rand(batch, 3, IMG, IMG, device="cuda", generator=g) * 2 - 1
        coef = torch.randn(batch, n_out, *thw, device="cuda", generator=g)

        def native_step():
            (nat(x, z, img) * coef).sum().backward()

        def torch_step():
            (torch_forward(twin, n_in, n_out, x, z, img) * coef).sum().backward()

        def native_forward():
            with torch.no_grad():
                nat(x, z, img)

        def frozen_step():
            (frozen(x, z, img) * coef).sum().backward()

        # the two arms are the same block: one step each from the same u and v, and the torch-op form once in float64 as the yardstick
        def grads_of(step, params):
            x.grad = z.grad = None
            step()
            out = {k: t.grad.detach().clone() for k, t in params.items() if t.grad is not None}
            out["x"], out["z"] = x.grad.detach().clone(), z.grad.detach().clone()
            return out

        g_nat = grads_of(native_step, dict(nat.named_parameters()))
        g_tor = grads_of(torch_step, twin)
        twin64 = twin_of(torch.float64)
        x64, z64 = x.detach().double().requires_grad_(True), z.detach().double().requires_grad_(True)
        (torch_forward(twin64, n_in, n_out, x64, z64, img.double()) * coef.double()).sum().backward()
        g64 = {k: t.grad for k, t in twin64.items() if t.grad is not None}
        g64["x"], g64["z"] = x64.grad, z64.grad

        def dist(grads):   # conv_0.bias has a zero gradient (the instance norm removes it): no relative distance exists
            return max((float((grads[k].double() - t).norm() / t.norm().clamp_min(1e-300)), k) for k, t in g64.items() if k != "conv_0.bias")

        worst = {"native": dist(g_nat), "torch": dist(g_tor)}
        del twin64, x64, z64, g64, g_nat, g_tor
        torch.cuda.empty_cache()
        pair = {"native": native_step, "torch": torch_step, "native forward": native_forward, "native frozen": frozen_step}
        times = {k: [] for k in pair}
        for fn in pair.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in pair.items():
                times[k].append(timed(fn, args.iters))
        rows.append((name, n_in, n_out, batch, thw, times, worst))
        print(name, {k: f"{statistics.median(v):.3f} ms" for k, v in times.items()}, "worst rel-L2 of a gradient from float64:", worst, flush=True)
        del nat, frozen, twin, x, z, img, coef
        torch.cuda.empty_cache()

    prop = torch.cuda.get_device_properties(0)
    lines = ["# GeneratorBlock, training path: native against the torch-op form", "",
             f"`python tools/gblock_train_bench.py --rounds {args.rounds} --iters {args.iters} --warmup {args.warmup}` on the device the runtime names "
             f"\"{torch.cuda.get_device_name(0)}\" ({getattr(prop, 'gcnArchName', 'gfx?').split(':')[0]}, {prop.multi_processor_count} compute units);",
             f"z = {Z_DIM}, a {IMG} x {IMG} start frame, spectral norm on, `.train()` mode; all arms in one process, alternating round by round, back to",
             f"back; each figure is the time of one call in ms (device events around {args.iters} calls), median and minimum over the rounds.  One call =",
             "the forward, the loss sum(c out) and the backward into x, z and every parameter gradient (no optimiser step).  The native arm computes in",
             "exact fp32 with fixed summation orders; the torch arm uses whatever the framework's convolution library picks.  A record of what was",
             "measured, not a gate: this path has no earlier number.", "",
             "| block | input | native median | native min | torch median | torch min | native / torch (median) |", "|---|---|---|---|---|---|---|"]
    for name, n_in, n_out, batch, thw, t, _ in rows:
        n, r = t["native"], t["torch"]
        lines.append(f"| {name} {n_in} -> {n_out} | {batch} x {thw[0]} x {thw[1]} x {thw[2]} | {statistics.median(n):.3f} | {min(n):.3f} | "
                     f"{statistics.median(r):.3f} | {min(r):.3f} | {statistics.median(n) / statistics.median(r):.2f} |")
    lines += ["", "Where the native arm's time goes (medians, ms): the forward alone (no `saved`), and forward + backward of a frozen module, which launches",
              "no weight-gradient, bias-gradient or Spade-branch backward kernel; the remainder of the full step is those launches.", "",
              "| block | full step | forward alone | frozen step | frozen backward = frozen - forward | parameter gradients = full - frozen |", "|---|---|---|---|---|---|"]
    for name, n_in, n_out, batch, thw, t, _ in rows:
        full, fwd, fro = (statistics.median(t[k]) for k in ("native", "native forward", "native frozen"))
        lines.append(f"| {name} | {full:.3f} | {fwd:.3f} | {fro:.3f} | {fro - fwd:.3f} | {full - fro:.3f} |")
    lines += ["", "What came out:"]
    for name, n_in, n_out, batch, thw, t, worst in rows:
        ratio = statistics.median(t["native"]) / statistics.median(t["torch"])
        lines.append(f"- {name}: the native path takes {ratio:.2f} of the torch-op form's time ({'native' if ratio < 1 else 'torch-op form'} faster).  "
                     f"Worst rel-L2 of a gradient (x, z or a parameter) from the torch-op form run in float64: native {worst['native'][0]:.1e} "
                     f"(`{worst['native'][1]}`), torch fp32 {worst['torch'][0]:.1e} (`{worst['torch'][1]}`).")
    lines += ["", "The distances from float64 are of one size in both arms: they belong to the problem in fp32 at this size (presumably LeakyReLU decisions",
              "that an fp32 pass takes differently from float64; not examined further), not to one arm.  The tests hold the native path to the",
              "reference's float64 results at 1e-4 on small blocks and its kernels to float64 at derived bounds (profiles/gblock_train_gate.md).",
              "What is left out: DESIGN.md section 12.8.  Per-kernel times were not measured; the split above is by whole calls."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
