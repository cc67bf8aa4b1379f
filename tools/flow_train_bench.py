#!/usr/bin/env python
"""Step time of cINN training on one GPU: (a) ``FlowTrainer.step`` (HIP forward / backward + fused Adam), (b) the autograd path
(``ConditionalFlow.differentiable`` + ``torch.optim.Adam``), (c) the same flow written with stock torch ops + ``torch.optim.Adam``
(what a user would run without this package's training path).  Full geometry (20 flows, hidden 512, depth 2, E = 64), B = 50 and
64; the variants alternate inside one process and the whole cycle repeats, so the spread between rounds is visible.  Device events
around ``--steps`` steps after ``--warmup``.  Also prints the byte floor of a step computed from the parameter shapes.

    python tools/flow_train_bench.py [--steps 200] [--warmup 20] [--rounds 3] [--only a] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "image2video-synthesis-using-cinns_amd")):
    sys.path.insert(0, p)

import i2v_synth as synth  # noqa: E402
from i2v_train import FlowTrainer  # noqa: E402
from stage2_cINN.modules.flow_blocks import ConditionalFlow  # noqa: E402

COPY_BW = 6.3e12   # bytes / s an MI355X sustains on a device copy
ADAM = dict(lr=1e-5, betas=(0.9, 0.99), weight_decay=0, amsgrad=True)


class StockFlow(torch.nn.Module):
    """ConditionalFlow (conditioning 'none', no control) in plain torch ops over the same state_dict keys."""

    def __init__(self, sd, n_flows=20, depth=2):
        super().__init__()
        self.n_flows, self.depth = n_flows, depth
        self.names = [k for k, v in sd.items() if v.is_floating_point()]
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(sd[k].clone()) for k in self.names])
        self.idx = [sd[f"sub_layers.{fl}.shuffle.forward_shuffle_idx"].cuda() for fl in range(n_flows)]

    def forward(self, x, emb):
        p = dict(zip(self.names, self.ps))
        logdet = torch.zeros(x.shape[0], device=x.device)
        for fl in range(self.n_flows):
            pre = f"sub_layers.{fl}."
            scale = p[pre + "norm_layer.scale"].reshape(1, -1)
            x = scale * (x + p[pre + "norm_layer.loc"].reshape(1, -1))
            logdet = logdet + scale.abs().log().sum()
            x = x * ((x >= 0).to(x) + (x < 0).to(x) * 0.9)
            for i in range(2):
                if i == 1:
                    x = torch.cat(torch.chunk(x, 2, dim=1)[::-1], dim=1)
                keep, apply = torch.chunk(x, 2, dim=1)
                cin = torch.cat((keep, emb), dim=1)
                st = []
                for net in "st":
                    h = cin
                    for li in range(self.depth + 2):
                        h = F.linear(h, p[f"{pre}coupling.{net}.{i}.main.{2 * li}.weight"], p[f"{pre}coupling.{net}.{i}.main.{2 * li}.bias"])
                        if li <= self.depth:
                            h = F.leaky_relu(h, 0.01)
                    st.append(h)
                x = torch.cat((keep, apply * st[0].exp() + st[1]), dim=1)
                logdet = logdet + st[0].sum(1)
            x = x[:, self.idx[fl]]
        return x, logdet


def flow_loss(zt, logdet):
    return (0.5 * zt.reshape(zt.shape[0], -1).pow(2).sum(1)).mean() - logdet.mean()


def make_variant(kind, sd):
    if kind == "c":
        net = StockFlow(sd).cuda()
    else:
        net = ConditionalFlow(64, 64, 512, 2, 20, conditioning_option="None")
        net.load_state_dict(sd)
        net = net.cuda()
    if kind == "a":
        tr = FlowTrainer(net, **ADAM)
        return lambda z, e: tr.step(z, e)
    net.differentiable = True
    opt = torch.optim.Adam(net.parameters(), **ADAM)

    def step(z, e):
        zt, logdet = net(z, e)
        loss = flow_loss(zt, logdet)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--batches", default="50,64")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.flow_state_dict(seed=7, n_flows=20, embedding_dim=64).items()}
    n_params = sum(v.numel() for v in sd.values() if v.is_floating_point())
    floor_ms = 12 * 4 * n_params / COPY_BW * 1e3
    result = {"n_params": n_params, "byte_floor_ms": floor_ms, "steps": args.steps, "runs": {}}
    print(f"{n_params} parameters; a step moves >= 12 x {4 * n_params / 1e6:.1f} MB = {48 * n_params / 1e9:.2f} GB -> floor {floor_ms:.3f} ms at 6.3 TB/s")
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        z, e = torch.randn(B, 64, generator=g).cuda(), torch.randn(B, 64, generator=g).cuda()
        steps = {k: make_variant(k, sd) for k in args.only}
        times = {k: [] for k in args.only}
        for _ in range(args.rounds):
            for k, step in steps.items():
                for _ in range(args.warmup):
                    step(z, e)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                for _ in range(args.steps):
                    step(z, e)
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1) / args.steps)
        for k, v in times.items():
            print(f"B={B} variant {k}: ms/step per round {[round(t, 3) for t in v]}  median {np.median(v):.3f}  "
                  f"spread {(max(v) - min(v)) / np.median(v) * 100:.1f} %  floor share {floor_ms / np.median(v) * 100:.1f} %")
        result["runs"][str(B)] = times
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
