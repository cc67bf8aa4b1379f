"""Class-surface mirror of the reference's ``metrics/PyTorch_FVD/I3D.py``: the Kinetics-400 I3D whose logits are the FVD features.

``I3D(num_classes, modality='rgb')`` carries the reference's parameter and buffer names and shapes (``model_rgb.pth`` loads with
``load_state_dict``), and its forward runs on the native handle (csrc/i2v_i3d.hip: exact-fp32 matrix-core convolutions, eval-mode
BatchNorm3d folded at load).  There is no eager forward: on the CPU the module raises.  Only the rgb network is built."""
import torch
import torch.nn as nn

import i2v_native

MIXED = (("mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("mixed_5c", 832, (384, 192, 384, 48, 128, 128)))


def get_padding_shape(filter_dim, stride, mod=0):
    """"TF SAME" padding (front, back) of one dimension; ``mod`` = size % stride, used for the time dimension of strided units."""
    along = max(filter_dim - mod, 0) if mod else max(filter_dim - stride, 0)
    return along // 2, along - along // 2


def _pool_out(size, k, s, mod=0):
    """MaxPool3dTFPadding: zero padding to SAME, then MaxPool3d(ceil_mode=True)."""
    e = size + sum(get_padding_shape(k, s, mod))
    o = -(-(e - k) // s) + 1
    return o - 1 if (o - 1) * s >= e else o


def endpoint_shapes(T, H=224, W=224, num_classes=400, batch=1):
    """{end-point name: [B, C, T, H, W]} of the network for an input of T frames of H x W pixels: the arithmetic csrc/i2v_i3d.hip plans
    its buffers with (the stem's and the stride-2 pools' time padding depends on the parity of T)."""
    shp, out = {}, None

    def put(name, c, t, h, w):
        shp[name] = [batch, c, t, h, w]
        return t, h, w
    conv_s2 = lambda n, m=0: (n + sum(get_padding_shape(7, 2, m)) - 7) // 2 + 1  # noqa: E731
    t, h, w = put("conv3d_1a_7x7", 64, conv_s2(T, T % 2), conv_s2(H), conv_s2(W))
    t, h, w = put("maxPool3d_2a_3x3", 64, t, _pool_out(h, 3, 2), _pool_out(w, 3, 2))
    put("conv3d_2b_1x1", 64, t, h, w)
    put("conv3d_2c_3x3", 192, t, h, w)
    t, h, w = put("maxPool3d_3a_3x3", 192, t, _pool_out(h, 3, 2), _pool_out(w, 3, 2))
    for name, _cin, o in MIXED:
        c = o[0] + o[2] + o[4] + o[5]
        put(name, c, t, h, w)
        if name == "mixed_3c":
            t, h, w = put("maxPool3d_4a_3x3", c, _pool_out(t, 3, 2, t % 2), _pool_out(h, 3, 2), _pool_out(w, 3, 2))
        if name == "mixed_4f":
            t, h, w = put("maxPool3d_5a_2x2", c, _pool_out(t, 2, 2, t % 2), _pool_out(h, 2, 2), _pool_out(w, 2, 2))
    t, h, w = put("avg_pool", 1024, t - 1, h - 6, w - 6)
    put("conv3d_0c_1x1", num_classes, t, h, w)
    return shp


class Unit3Dpy(nn.Module):
    """Parameter holder of one conv unit: ``conv3d`` (+ ``batch3d``, eps 1e-3).  The computation lives in the native handle."""

    def __init__(self, in_channels, out_channels, kernel_size=(1, 1, 1), stride=(1, 1, 1), activation='relu', padding='SAME', use_bias=False,
                 use_bn=True):
        super().__init__()
        self.conv3d = nn.Conv3d(in_channels, out_channels, kernel_size, stride=stride, bias=use_bias)
        if use_bn:
            self.batch3d = nn.BatchNorm3d(out_channels, eps=1e-3)


class Mixed(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        o = out_channels
        self.branch_0 = Unit3Dpy(in_channels, o[0])
        self.branch_1 = nn.Sequential(Unit3Dpy(in_channels, o[1]), Unit3Dpy(o[1], o[2], kernel_size=(3, 3, 3)))
        self.branch_2 = nn.Sequential(Unit3Dpy(in_channels, o[3]), Unit3Dpy(o[3], o[4], kernel_size=(3, 3, 3)))
        self.branch_3 = nn.Sequential(nn.Identity(), Unit3Dpy(in_channels, o[5]))   # index 0 is the (parameter-free) max pool


class I3D(nn.Module):
    def __init__(self, num_classes, modality='rgb', dropout_prob=0, name='inception'):
        super().__init__()
        if modality != 'rgb':
            raise NotImplementedError(f"I3D: only the rgb network is built (modality = {modality!r}); the flow network is out of scope")
        self.name, self.num_classes, self.modality = name, num_classes, modality
        self.conv3d_1a_7x7 = Unit3Dpy(3, 64, kernel_size=(7, 7, 7), stride=(2, 2, 2))
        self.conv3d_2b_1x1 = Unit3Dpy(64, 64)
        self.conv3d_2c_3x3 = Unit3Dpy(64, 192, kernel_size=(3, 3, 3))
        for mname, cin, o in MIXED:
            setattr(self, mname, Mixed(cin, list(o)))
        self.conv3d_0c_1x1 = Unit3Dpy(1024, num_classes, activation=None, use_bias=True, use_bn=False)
        self.softmax = nn.Softmax(1)
        for p in self.parameters():
            p.requires_grad = False
        self._native = None
        self._native_key = None

    # ---- native handle: packed from the module's own state, re-packed when the state changes
    def _state_key(self):
        return tuple((t.device, t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def native(self):
        p = next(self.parameters())
        if not p.is_cuda:
            raise i2v_native.I2VError("I3D runs on a HIP device only (csrc/i2v_i3d.hip); this package has no CPU fallback -- move the "
                                      "module and its input to 'cuda'")
        key = self._state_key()
        if self._native is None or self._native_key != key:
            if self._native is None or self._native.device != p.device:
                self._native = i2v_native.NativeI3D(self.num_classes, 3, device=p.device)
            self._native.load({k: v for k, v in self.state_dict().items() if not k.endswith("num_batches_tracked")})
            self._native_key = key
        return self._native

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._native_key = None

    def forward_frames(self, frames, denorm):
        """The product path: frames [B, T, 3, H, W] fp32 on the device (the decoder's output layout; any H, W -- the resize to 224 x 224
        of ``FVD_logging.preprocess`` is the handle's input stage), ``denorm``: values in [-1, 1] -> logits [B, num_classes]."""
        return self.native().forward(frames, denorm)

    @torch.no_grad()
    def forward(self, inp):
        """Reference signature: ``inp`` [B, 3, T, H, W] -> (softmax, logits).  The values go in as they are (no denorm)."""
        if inp.dim() != 5 or inp.shape[1] != 3:
            raise ValueError(f"I3D.forward: expected [B,3,T,H,W], got {tuple(inp.shape)}")
        logits = self.forward_frames(inp.permute(0, 2, 1, 3, 4).contiguous(), False)
        return self.softmax(logits), logits
