"""LPIPS on the device: own implementation of the reference's ``stage2_cINN/AE/modules/LPIPS.py`` surface (a stripped version of
https://github.com/richzhang/PerceptualSimilarity): a metric and, with frozen weights, a training loss.

``LPIPS`` keeps the reference's ``state_dict`` keys (``scaling_layer.shift/scale``, ``net.slice*``, ``lin{k}.model.1.weight``).  ``forward``
keeps the frames on the device: ScalingLayer and the layout change are one kernel, both images go through the native VGG-16 trunk,
and every layer's normalise / difference / 1x1 conv / spatial mean is ONE reduction in float64 (``i2v_lpips_layer``, csrc/i2v_lpips.hip).  Dropout is the
identity (the metric is evaluated in eval mode).  Weights come from files: ``vgg_path`` (torchvision's vgg16 state_dict) and ``lin_path``
(the ``vgg.pth`` of the LPIPS release: ``lin{k}.model.1.weight``); nothing is downloaded, there is no ``ckpt_util``.

With grad mode on and an argument that requires grad, ``forward`` returns the same bits with a ``grad_fn``: the backward pass (the LPIPS head,
then the trunk's input gradient, ``i2v_lpips_layer_backward`` / ``i2v_vgg_backward``) gives the gradient at ``input`` and / or ``target`` -- the
reference differentiates through ``target`` (stage1_VAE/modules/loss.py).  Once differentiable; VGG-16 and the lin layers stay frozen.

``lpips_score`` is the reference CLI's rule (eval_synthesis_quality.py:80-92)."""
import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

import i2v_native
from stage2_cINN.AE.modules.vgg16 import vgg16, normalize_tensor, spatial_average  # noqa: F401  (the reference's import line)


class LPIPS(nn.Module):
    # Learned perceptual metric
    def __init__(self, use_dropout=True, vgg_path=None, lin_path=None):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = [64, 128, 256, 512, 512]
        self.net = vgg16(pretrained=vgg_path is not None, requires_grad=False, path=vgg_path)
        self.lin0 = NetLinLayer(self.chns[0], use_dropout=use_dropout)
        self.lin1 = NetLinLayer(self.chns[1], use_dropout=use_dropout)
        self.lin2 = NetLinLayer(self.chns[2], use_dropout=use_dropout)
        self.lin3 = NetLinLayer(self.chns[3], use_dropout=use_dropout)
        self.lin4 = NetLinLayer(self.chns[4], use_dropout=use_dropout)
        if lin_path is not None:
            self.load_from_pretrained(lin_path)
        for param in self.parameters():
            param.requires_grad = False

    def load_from_pretrained(self, path):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"LPIPS: the lin-layer checkpoint {path!r} does not exist (vgg.pth of the LPIPS release; this package "
                                    "never downloads it)")
        self.load_state_dict(torch.load(path, map_location=torch.device("cpu")), strict=False)
        print("loaded pretrained LPIPS loss from {}".format(path))

    def _lins(self):
        return [getattr(self, f"lin{k}").model[-1].weight for k in range(5)]

    def forward(self, input, target):
        """input, target [N, 3, H, W] in [-1, 1] on the device -> [N, 1, 1, 1] fp32; differentiable with respect to whichever of the two
        requires grad (the same values, bit for bit, as under ``torch.no_grad()``)."""
        if input.shape != target.shape or input.dim() != 4 or input.shape[1] != 3:
            raise ValueError(f"LPIPS.forward: expected two [N,3,H,W] batches, got {tuple(input.shape)} / {tuple(target.shape)}")
        if not input.is_cuda or not target.is_cuda:
            raise i2v_native.I2VError("LPIPS runs on a HIP device only (csrc/i2v_vgg.hip, csrc/i2v_lpips.hip); this package has no CPU fallback")
        with torch.no_grad():
            self.net._lin = [w.reshape(-1) for w in self._lins()]
            native = self.net.native()
        if torch.is_grad_enabled() and (input.requires_grad or target.requires_grad):
            return _LPIPSFunction.apply(input, target, native)
        with torch.no_grad():
            taps = [native.features(i2v_native.vgg_input_stage(x.float().contiguous(), i2v_native.VGG_INPUT_LPIPS)) for x in (input, target)]
            return native.lpips(*taps).float().view(-1, 1, 1, 1)


class _LPIPSFunction(torch.autograd.Function):
    """LPIPS.forward with a backward pass: the side that needs a gradient keeps its activations (``features(save=True)``)."""

    @staticmethod
    def forward(ctx, input, target, native):
        ctx.native, ctx.dtypes, ctx.saved, taps = native, (input.dtype, target.dtype), [None, None], []
        for i, x in enumerate((input, target)):
            x = i2v_native.vgg_input_stage(x.detach().float().contiguous(), i2v_native.VGG_INPUT_LPIPS)
            if ctx.needs_input_grad[i]:
                t, ctx.saved[i] = native.features(x, save=True)
            else:
                t = native.features(x)
            taps.append(t)
        ctx.taps = taps
        return native.lpips(*taps).float().view(-1, 1, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        need = [s is not None for s in ctx.saved]
        tap_grads = ctx.native.lpips_backward(*ctx.taps, grad.double().reshape(-1).contiguous(), *need)
        out = [ctx.native.backward(g, s, frames=True).to(dt) if s is not None else None for g, s, dt in zip(tap_grads, ctx.saved, ctx.dtypes)]
        return out[0], out[1], None


class ScalingLayer(nn.Module):
    def __init__(self):
        super(ScalingLayer, self).__init__()
        self.register_buffer('shift', torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('scale', torch.Tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, inp):
        return (inp - self.shift) / self.scale


class NetLinLayer(nn.Module):
    """ A single linear layer which does a 1x1 conv """
    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super(NetLinLayer, self).__init__()
        layers = [nn.Dropout(), ] if (use_dropout) else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False), ]
        self.model = nn.Sequential(*layers)


def lpips_score(model, pd_imgs, gt_imgs, batch=10):
    """The reference CLI's rule (eval_synthesis_quality.py:85-89): the mean over floor(n / batch) batch means of ``model(pd, gt)``; the
    ragged tail is dropped, fewer than ``batch`` images are refused (the reference divides by zero there)."""
    n = pd_imgs.size(0)
    if gt_imgs.shape != pd_imgs.shape:
        raise ValueError(f"lpips_score: {tuple(pd_imgs.shape)} generated vs {tuple(gt_imgs.shape)} real images")
    if n < batch:
        raise ValueError(f"lpips_score: {n} images are fewer than one batch of {batch}; the reference's rule averages over floor(n / {batch}) batches")
    total = 0.0
    for i in range(n // batch):
        total += model(pd_imgs[i * batch:(i + 1) * batch], gt_imgs[i * batch:(i + 1) * batch]).mean().cpu().item()
    return total / (n // batch)
