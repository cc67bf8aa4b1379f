"""Times the training path of the whole stage-1 Generator (forward + backward) and writes profiles/generator_train_ab.md.

Two arms on the same GPU, the same seeded parameters and inputs, spectral norm on, ``.train()`` mode, at two geometries -- BAIR (channel_factor
64, upsample_s [2, 1], upsample_t [2, 1]: 16 frames of 64 x 64) and 128 x 128 (channel_factor 32, upsample_s [2, 2], upsample_t [2, 1]):
  native   stage1_VAE.modules.decoder.Generator with ``differentiable = True``: the fc Function, six block Functions, the up-sampling
           Functions and the image head Function; the loss sum(c frames), ``backward()`` into motion and every parameter's ``.grad``
  torch    the same network from stock torch ops (tools/gblock_train_bench.torch_forward per block, F.linear, F.interpolate, F.conv3d,
           autograd) on copies of the same parameters
The arms alternate, round by round, in ONE process, back to back; each timed window is ``--iters`` calls between two device events after
``--warmup`` calls; the table gives the median and the minimum over the rounds.  Then the native arm in parts, each a forward + backward of
that part alone on tensors of the shapes it sees in the chain: the six blocks (their entry and exit layout changes included), the layout
changes at the block borders (the [B][C][T][H][W] <-> channels-last copies a block makes at its entry and exit, forward and backward, timed as
torch copies of the same tensors: an estimate of what fusing them away could save, not a native kernel time), the up-samplings, fc, the head.
A record, not a gate: this path has no earlier number.  The whole file is written by this tool; nothing in it is edited by hand.

    python tools/generator_train_bench.py [--rounds 3] [--iters 2] [--warmup 1] [--out profiles/generator_train_ab.md]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image2video-synthesis-using-cinns_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gblock_train_bench import timed, torch_forward  # noqa: E402

#        name      nf  upsample_s upsample_t batch  start frame
CASES = (("BAIR", 64, [2, 1], [2, 1], 2, 64), ("128x128", 32, [2, 2], [2, 1], 1, 128))
Z_DIM = 64
BLOCKS = ("head_0", "g_0", "g_1", "g_2", "g_3", "g_4")
CHANNELS = ((16, 16), (16, 16), (16, 8), (8, 4), (4, 2), (2, 1))


def torch_generator(p, nf, factors, img, z):
    """The torch-op form of Generator.forward in .train() mode on a dict of the module's state-dict keys."""
    x = F.linear(z, p["fc.weight"], p["fc.bias"]).reshape(z.shape[0], -1, 1, 4, 4)
    for name, (a, b), (ut, us) in zip(BLOCKS, CHANNELS, [(1, 1)] + factors):
        if (ut, us) != (1, 1):
            x = F.interpolate(x, scale_factor=(ut, us, us))
        sub = {k[len(name) + 1:]: v for k, v in p.items() if k.startswith(name + ".")}
        x = torch_forward(sub, a * nf, b * nf, x, z, img)
    x = torch.tanh(F.conv3d(F.leaky_relu(x, 0.2), p["conv_img.weight"], p["conv_img.bias"], padding=1))
    return x.transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "generator_train_ab.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generator_train_bench: no HIP device; nothing is measured on a CPU")
    import i2v_native as native
    from stage1_VAE.modules.decoder import Generator, _UpsampleFunction

    rows = []
    for name, nf, ups, upt, batch, side in CASES:
        torch.manual_seed(6900)
        dic = {"channel_factor": nf, "z_dim": Z_DIM, "spectral_norm": True, "upsample_s": ups, "upsample_t": upt}
        nat = Generator(dic).cuda().train()
        nat.differentiable = True
        twin = {k: v.detach().clone().requires_grad_(not k.endswith(("_u", "_v"))) for k, v in nat.state_dict().items()}
        factors = [(2, 2), (2, 2), (2, 2)] + list(zip(upt, ups))
        g = torch.Generator(device="cuda").manual_seed(6901)
        z = torch.randn(batch, Z_DIM, device="cuda", generator=g).requires_grad_(True)
        img = torch.rand(batch, 3, side, side, device="cuda", generator=g) * 2 - 1
        with torch.no_grad():
            frames = nat(img, z)
            dist = float((frames - torch_generator(twin, nf, factors, img, z)).norm() / frames.norm())
        coef = torch.randn(frames.shape, device="cuda", generator=g)

        def native_step():
            (nat(img, z) * coef).sum().backward()

        def torch_step():
            (torch_generator(twin, nf, factors, img, z) * coef).sum().backward()

        # the parts, on tensors of the shapes of the chain
        shapes, T, H = [], 1, 4
        for (a, b), (ut, us) in zip(CHANNELS, [(1, 1)] + factors):
            low = (batch, a * nf, T, H, H)
            T, H = T * ut, H * us
            shapes.append((low, (ut, us), (batch, a * nf, T, H, H), (batch, b * nf, T, H, H)))
        xin = [torch.randn(s[2], device="cuda", generator=g).requires_grad_(True) for s in shapes]
        xlow = [torch.randn(s[0], device="cuda", generator=g).requires_grad_(True) for s in shapes]
        cout = [torch.randn(s[3], device="cuda", generator=g) for s in shapes]
        zf = z.detach().clone().requires_grad_(True)
        g_fc = torch.randn(batch, 256 * nf, device="cuda", generator=g)
        from stage1_VAE.modules.decoder import _GenFcFunction, _GenHeadFunction
        xh = torch.randn(shapes[-1][3], device="cuda", generator=g).requires_grad_(True)

        def blocks_step():
            for blk, x, c in zip(nat._blocks(), xin, cout):
                (blk(x, zf, img) * c).sum().backward()

        def borders_step():   # entry and exit copies of a block, forward and backward
            for x, c in zip(xin, cout):
                for t in (x.detach(), c, c, x.detach()):
                    t.permute(0, 2, 3, 4, 1).contiguous()

        def upsample_step():
            for x, (_, (ut, us), _, _) in zip(xlow, shapes):
                if (ut, us) != (1, 1):
                    y = _UpsampleFunction.apply(x, ut, us)
                    y.backward(y.detach())

        def fc_step():
            _GenFcFunction.apply(nat, zf, nat.fc.weight, nat.fc.bias).backward(g_fc)

        def head_step():
            _GenHeadFunction.apply(nat, xh, nat.conv_img.weight, nat.conv_img.bias).backward(coef)

        pair = {"native": native_step, "torch": torch_step, "blocks": blocks_step, "borders": borders_step, "upsampling": upsample_step, "fc": fc_step,
                "head": head_step}
        times = {k: [] for k in pair}
        for fn in pair.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in pair.items():
                times[k].append(timed(fn, args.iters))
        rows.append((name, nf, batch, tuple(frames.shape), times, dist))
        print(name, {k: f"{statistics.median(v):.3f} ms" for k, v in times.items()}, "frames native vs torch fp32 rel-L2", dist, flush=True)
        del nat, twin, xin, xlow, cout, xh, frames, coef
        torch.cuda.empty_cache()

    prop = torch.cuda.get_device_properties(0)
    lines = ["# Generator, training path: native against the torch-op form", "",
             f"`python tools/generator_train_bench.py --rounds {args.rounds} --iters {args.iters} --warmup {args.warmup}` on the device the runtime names "
             f"\"{torch.cuda.get_device_name(0)}\" ({getattr(prop, 'gcnArchName', 'gfx?').split(':')[0]}, {prop.multi_processor_count} compute units);",
             f"z = {Z_DIM}, spectral norm on, `.train()` mode; all arms in one process, alternating round by round, back to back; each figure is the",
             f"time of one call in ms (device events around {args.iters} calls), median and minimum over {args.rounds} rounds.  One call = the forward, the loss",
             "sum(c frames) and the backward into motion and every parameter gradient (no optimiser step).  The native arm computes in exact fp32",
             "with fixed summation orders; the torch arm uses whatever the framework's convolution library picks.  A record of what was measured, not",
             "a gate: this path has no earlier number.", "",
             "| geometry | frames | native median | native min | torch median | torch min | native / torch (median) |", "|---|---|---|---|---|---|---|"]
    for name, nf, batch, shape, t, _ in rows:
        n, r = t["native"], t["torch"]
        lines.append(f"| {name}, channel_factor {nf} | {' x '.join(map(str, shape))} | {statistics.median(n):.3f} | {min(n):.3f} | "
                     f"{statistics.median(r):.3f} | {min(r):.3f} | {statistics.median(n) / statistics.median(r):.2f} |")
    lines += ["", "The native arm in parts (medians, ms), each a forward + backward of that part alone on tensors of the chain's shapes.  `borders` is",
              "NOT a part of the sum: it is the time of torch copies between [B][C][T][H][W] and channels-last of the tensors that the six blocks",
              "convert at their entry and exit (four per block and step), an estimate of what the blocks spend there; it lies inside `blocks`.", "",
              "| geometry | whole step | six blocks | of which borders (estimate) | up-sampling | fc | head | parts' sum |", "|---|---|---|---|---|---|---|---|"]
    for name, nf, batch, shape, t, _ in rows:
        m = {k: statistics.median(v) for k, v in t.items()}
        lines.append(f"| {name} | {m['native']:.3f} | {m['blocks']:.3f} | {m['borders']:.3f} | {m['upsampling']:.3f} | {m['fc']:.3f} | {m['head']:.3f} | "
                     f"{m['blocks'] + m['upsampling'] + m['fc'] + m['head']:.3f} |")
    lines += ["", "What came out:"]
    for name, nf, batch, shape, t, dist in rows:
        ratio = statistics.median(t["native"]) / statistics.median(t["torch"])
        lines.append(f"- {name}: the native path takes {ratio:.2f} of the torch-op form's time ({'native' if ratio < 1 else 'torch-op form'} faster); "
                     f"its frames lie {dist:.1e} (rel-L2) from the torch-op form's fp32 frames.")
    lines += ["", "Per-kernel times were not measured; the split is by whole calls.  What is left out of this path: DESIGN.md section 12.9."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
