"""VGG-16 feature trunk: own implementation of the reference's ``stage2_cINN/AE/modules/vgg16.py`` surface.

``vgg16`` is a parameter holder with the reference's ``state_dict`` keys (``slice1.0.weight`` ... ``slice5.28.bias``: the ``features`` part
of torchvision's configuration D cut into five slices); ``forward`` runs on the device through ``csrc/i2v_vgg.hip`` (its layer plan: ``csrc/i2v_vgg_plan.h``; thirteen 3x3
convolutions in exact fp32 on the matrix cores, four 2x2 max pools) and returns the reference's namedtuple.  torchvision is not a
dependency: the graph is written out here and the weights come from torchvision's ``vgg16`` state_dict FILE (keys ``features.N.*``;
the classifier keys are ignored).  Nothing is ever downloaded: a missing file raises ``FileNotFoundError`` naming it.

The returned tensors are NCHW-shaped views of channels-last memory (the layout the kernels write).  The weights are frozen:
``requires_grad=True`` (weight gradients) is refused.  The INPUT gradient exists: with grad mode on and ``X.requires_grad`` the five taps
are differentiable with respect to ``X`` (``i2v_vgg_backward``: the input-gradient convolutions on the forward kernel, once differentiable)."""
import os
from collections import namedtuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

import i2v_native

DEFAULT_PATH = './models/vgg16/vgg16-397923af.pth'
# torchvision configuration D up to features.29
_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512)
_SLICES = (range(0, 4), range(4, 9), range(9, 16), range(16, 23), range(23, 30))
VggOutputs = namedtuple("VggOutputs", ['relu1_2', 'relu2_2', 'relu3_3', 'relu4_3', 'relu5_3'])


def _features():
    layers, cin = [], 3
    for v in _CFG:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return layers


def load_torchvision_state_dict(path):
    """{features.N.weight / .bias} of torchvision's vgg16 checkpoint file at ``path``."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"vgg16: the torchvision VGG-16 state_dict file {path!r} does not exist (torchvision's vgg16-397923af.pth; "
                                "this package never downloads it -- pass path=...)")
    sd = torch.load(path, map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    return {k: v for k, v in sd.items() if k.startswith("features.")}


class vgg16(nn.Module):
    def __init__(self, requires_grad=False, pretrained=True, path=None):
        if requires_grad:
            raise NotImplementedError("vgg16(requires_grad=True) is not built: the native trunk has no backward pass (inference only)")
        super().__init__()
        feats = _features()
        self.N_slices = 5
        for k, idx in enumerate(_SLICES):
            s = nn.Sequential()
            for x in idx:
                s.add_module(str(x), feats[x])
            setattr(self, f"slice{k + 1}", s)
        for p in self.parameters():
            p.requires_grad = False
        self._native = None
        self._native_key = None
        self._lin = None     # LPIPS hands its lin weights to the same handle
        if pretrained:
            self.load_torchvision(DEFAULT_PATH if path is None else path)

    def load_torchvision(self, path):
        sd = load_torchvision_state_dict(path)
        own = {}
        for k, idx in enumerate(_SLICES):
            for x in idx:
                for s in ("weight", "bias"):
                    if f"features.{x}.{s}" in sd:
                        own[f"slice{k + 1}.{x}.{s}"] = sd[f"features.{x}.{s}"]
        self.load_state_dict(own, strict=True)

    def torchvision_state_dict(self):
        """The holder's parameters under torchvision's keys (what ``i2v_vgg_load`` takes)."""
        return {"features." + k.split(".", 1)[1]: v for k, v in self.state_dict().items()}

    # ---- native handle: packed from the module's own state, re-packed when the state changes
    def _state_key(self):
        ts = list(self.parameters()) + ([] if self._lin is None else list(self._lin))
        return tuple((t.device, t.data_ptr(), t._version) for t in ts)

    def native(self):
        p = next(self.parameters())
        if not p.is_cuda:
            raise i2v_native.I2VError("vgg16 runs on a HIP device only (csrc/i2v_vgg.hip); this package has no CPU fallback -- move the module "
                                      "and its input to 'cuda'")
        key = self._state_key()
        if self._native is None or self._native_key != key:
            if self._native is None or self._native.device != p.device:
                self._native = i2v_native.NativeVGG(device=p.device)
            sd = self.torchvision_state_dict()
            if self._lin is not None:
                sd.update({f"lin{k}.model.1.weight": w for k, w in enumerate(self._lin)})
            self._native.load(sd)
            self._native_key = key
        return self._native

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._native_key = None

    @torch.no_grad()
    def taps(self, x_cl):
        """Channels-last input [N, H, W, 4] (``i2v_native.vgg_input_stage``) -> the five channels-last taps [N, H', W', C]."""
        return self.native().features(x_cl)

    def forward(self, X):
        """X [N, 3, H, W], already normalised (as the reference's forward takes it) -> VggOutputs of five NCHW-shaped tensors; they carry a
        ``grad_fn`` when grad mode is on and ``X.requires_grad``."""
        if X.dim() != 4 or X.shape[1] != 3:
            raise ValueError(f"vgg16.forward: expected [N,3,H,W], got {tuple(X.shape)}")
        i2v_native._require_gpu(X.detach().float().contiguous())
        if torch.is_grad_enabled() and X.requires_grad:
            return VggOutputs(*_TapsFunction.apply(X, self.native()))
        with torch.no_grad():
            return VggOutputs(*[t.permute(0, 3, 1, 2) for t in self.taps(_pad4(X))])


def _pad4(X):
    """[N, 3, H, W] -> the channels-last input [N, H, W, 4] of the trunk (channel 3 zero)."""
    return torch.cat([X.float().permute(0, 2, 3, 1), X.new_zeros(X.shape[0], X.shape[2], X.shape[3], 1, dtype=torch.float32)], -1).contiguous()


class _TapsFunction(torch.autograd.Function):
    """The five taps as a function of X: forward keeps the activations (``features(save=True)``), backward is ``NativeVGG.backward``."""

    @staticmethod
    def forward(ctx, X, native):
        taps, ctx.saved = native.features(_pad4(X.detach()), save=True)
        ctx.native, ctx.dtype = native, X.dtype
        return tuple(t.permute(0, 3, 1, 2) for t in taps)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        # tap gradients of any stride (NCHW-contiguous ones of a torch graph behind the taps, expanded scalars, ...) -> channels-last
        cl = [g.float().permute(0, 2, 3, 1).contiguous() for g in grads]
        gx = ctx.native.backward(cl, ctx.saved)
        return gx[..., :3].permute(0, 3, 1, 2).to(ctx.dtype), None


def normalize_tensor(x, eps=1e-10):
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
    return x / (norm_factor + eps)


def spatial_average(x, keepdim=True):
    return x.mean([2, 3], keepdim=keepdim)
