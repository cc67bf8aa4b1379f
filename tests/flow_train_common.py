"""Shared by the flow-training tests: the gradient fixture (written as two files, see tests/golden/make_golden_train.py) and the
autograd reference -- ``oracle/flow_ref.flow_forward`` under torch autograd on the CPU."""
import json
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from oracle import flow_ref

FIXTURE_PARTS = ("flow_grad_ctrl_h128.npz", "flow_grad_ctrl_h128_block1.npz")


def load_grad_fixture():
    arrays = {}
    for name in FIXTURE_PARTS:
        with np.load(os.path.join(GOLDEN, name)) as f:
            arrays.update({k: f[k] for k in f.files})
    meta = json.loads(bytes(arrays.pop("meta")).decode())
    return arrays, meta


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def oracle_grads(sd_np, x, embed, dtype, n_flows, control, d_zt=None, d_logdet=None, depth=2):
    """Autograd through the oracle in ``dtype``.  Cotangents: (d_zt, d_logdet), or the FlowLoss mean(0.5 ||zt||^2) - mean(logdet).
    -> (zt [B,64], logdet [B], loss, {"x", "embed", state_dict keys: gradient})."""
    with torch.enable_grad():
        sd = {}
        for k, v in sd_np.items():
            t = torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v.detach().cpu()
            sd[k] = t.to(dtype).requires_grad_(True) if t.is_floating_point() else t
        x = x.detach().cpu().to(dtype).requires_grad_(True)
        embed = embed.detach().cpu().to(dtype).requires_grad_(True)
        zt, logdet = flow_ref.flow_forward(sd, x, embed, n_flows=n_flows, depth=depth, control=control)
        zt = zt.reshape(zt.shape[0], -1)
        if d_zt is None:
            loss = (0.5 * zt.pow(2).sum(1)).mean() - logdet.mean()
        else:
            loss = (zt * d_zt.cpu().to(dtype)).sum() + (logdet * d_logdet.cpu().to(dtype)).sum()
        loss.backward()
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.grad is not None}
    grads["x"], grads["embed"] = x.grad, embed.grad
    return zt.detach(), logdet.detach(), loss.detach(), grads


def kink_margins(sd_np, x, embed, n_flows, control, depth=2):
    """Per sample, the smallest |input| of any LeakyReLU / InvLeakyRelu of the flow in the float64 oracle, i.e. its distance
    from the nearest kink of the piecewise-smooth function, and the largest |fp32 - fp64| difference of those inputs in the
    oracle's own fp32 run, absolute and relative to the fp64 value (a relative difference of 1 would be a crossed kink).  The oracle is instrumented from outside (its ``F.leaky_relu`` and ``inv_lrelu_forward`` are
    wrapped for the duration of the call), not changed.  -> (margin [B], fp32_error [B], fp32_relative_error [B])"""
    def run(dtype):
        rec = []
        orig_f, orig_inv = flow_ref.F, flow_ref.inv_lrelu_forward

        def lrelu(h, slope):
            rec.append(h.detach())
            return F.leaky_relu(h, slope)

        def inv(h, alpha=0.9):
            rec.append(h.detach())
            return orig_inv(h, alpha)
        flow_ref.F, flow_ref.inv_lrelu_forward = types.SimpleNamespace(linear=F.linear, leaky_relu=lrelu), inv
        try:
            with torch.no_grad():
                sd = {k: torch.as_tensor(np.asarray(v)) for k, v in sd_np.items()}
                sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
                flow_ref.flow_forward(sd, x.to(dtype), embed.to(dtype), n_flows=n_flows, depth=depth, control=control)
        finally:
            flow_ref.F, flow_ref.inv_lrelu_forward = orig_f, orig_inv
        return rec
    r64, r32 = run(torch.float64), run(torch.float32)
    margin = torch.stack([h.abs().min(1).values for h in r64]).min(0).values
    err = torch.stack([(a.double() - b).abs().max(1).values for a, b in zip(r32, r64)]).max(0).values
    crossing = torch.stack([((a.double() - b).abs() / b.abs()).max(1).values for a, b in zip(r32, r64)]).max(0).values
    return margin, err, crossing
