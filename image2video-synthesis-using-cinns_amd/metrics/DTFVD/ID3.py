"""Class-surface mirror of the reference's ``metrics/DTFVD/ID3.py``: the Inception-v1 I3D trained on dynamic textures (DTDB), length 16,
whose pooled 1024-d features DTFVD and the DT-I3D diversity score are computed from.

``InceptionI3D(num_classes, spatial_squeeze, ...)`` carries the reference's parameter and buffer names and shapes
(``I3D_16.pth.tar['state_dict']`` loads with ``load_state_dict(strict=True)``); the computation runs on the native handle
(csrc/i2v_i3d.hip, the dynamic-texture variant: BatchNorm eps 1e-5, SAME padding by ``compute_pad`` in all three dimensions,
``AvgPool3d((2, 7, 7))``).  Only ``get_representation`` is built -- the metric never runs the classifier -- so ``forward`` (logits),
``replace_logits`` and a ``final_endpoint`` other than 'logits' raise ``NotImplementedError``.  There is no eager forward: on the CPU the
module raises ``I2VError``."""
import torch
import torch.nn as nn

import i2v_native

MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))


def compute_pad(kernel, stride, size):
    """``Unit3D.compute_pad`` / ``MaxPool3dSamePadding.compute_pad``: total SAME padding of one dimension, (front, back) = (p // 2, p - p // 2)."""
    p = max(kernel - stride, 0) if size % stride == 0 else max(kernel - size % stride, 0)
    return p // 2, p - p // 2


def _out(size, k, s):
    """Output extent of a SAME-padded conv or (floor-mode) max pool."""
    return (size + sum(compute_pad(k, s, size)) - k) // s + 1


def endpoint_shapes(T, H=224, W=224, batch=1, pool_t=2):
    """{end-point name: [B, C, T, H, W]} up to 'AvgPool_5' for an input of T frames of H x W pixels: the arithmetic csrc/i2v_i3d.hip plans
    its buffers with.  'AvgPool_5' is None where fewer than ``pool_t`` time steps (or not a 7 x 7 map) reach the average pool -- the
    reference raises there, and so does the handle."""
    shp = {}

    def put(name, c, t, h, w):
        shp[name] = [batch, c, t, h, w]
        return t, h, w
    t, h, w = put("Conv3d_1a_7x7", 64, _out(T, 7, 2), _out(H, 7, 2), _out(W, 7, 2))
    t, h, w = put("MaxPool3d_2a_3x3", 64, t, _out(h, 3, 2), _out(w, 3, 2))
    put("Conv3d_2b_1x1", 64, t, h, w)
    put("Conv3d_2c_3x3", 192, t, h, w)
    t, h, w = put("MaxPool3d_3a_3x3", 192, t, _out(h, 3, 2), _out(w, 3, 2))
    for name, _cin, o in MIXED:
        if name == "Mixed_4b":
            t, h, w = put("MaxPool3d_4a_3x3", c, _out(t, 3, 2), _out(h, 3, 2), _out(w, 3, 2))
        if name == "Mixed_5b":
            t, h, w = put("MaxPool3d_5a_2x2", c, _out(t, 2, 2), _out(h, 2, 2), _out(w, 2, 2))
        c = o[0] + o[2] + o[4] + o[5]
        put(name, c, t, h, w)
    shp["AvgPool_5"] = [batch, 1024, t - pool_t + 1, h - 6, w - 6] if t >= pool_t and h >= 7 and w >= 7 else None
    return shp


class Unit3D(nn.Module):
    """Parameter holder of one conv unit: ``conv3d`` (+ ``bn``, torch's default eps 1e-5).  The computation lives in the native handle."""

    def __init__(self, in_channels, output_channels, kernel_size=(1, 1, 1), stride=(1, 1, 1), padding=0, activation_fn='relu',
                 use_batch_norm=True, use_bias=False, name='unit_3d'):
        super().__init__()
        self.name = name
        self.conv3d = nn.Conv3d(in_channels, output_channels, tuple(kernel_size), stride=tuple(stride), padding=0, bias=use_bias)
        if use_batch_norm:
            self.bn = nn.BatchNorm3d(output_channels)


class InceptionModule(nn.Module):
    def __init__(self, in_channels, out_channels, name):
        super().__init__()
        o = out_channels
        self.b0 = Unit3D(in_channels, o[0], name=name + '/Branch_0/Conv3d_0a_1x1')
        self.b1a = Unit3D(in_channels, o[1], name=name + '/Branch_1/Conv3d_0a_1x1')
        self.b1b = Unit3D(o[1], o[2], kernel_size=(3, 3, 3), name=name + '/Branch_1/Conv3d_0b_3x3')
        self.b2a = Unit3D(in_channels, o[3], name=name + '/Branch_2/Conv3d_0a_1x1')
        self.b2b = Unit3D(o[3], o[4], kernel_size=(3, 3, 3), name=name + '/Branch_2/Conv3d_0b_3x3')
        self.b3b = Unit3D(in_channels, o[5], name=name + '/Branch_3/Conv3d_0b_1x1')   # (b3a, the max pool in front, has no parameters)
        self.name = name


class InceptionI3D(nn.Module):
    VALID_ENDPOINTS = ('Conv3d_1a_7x7', 'MaxPool3d_2a_3x3', 'Conv3d_2b_1x1', 'Conv3d_2c_3x3', 'MaxPool3d_3a_3x3', 'Mixed_3b', 'Mixed_3c',
                       'MaxPool3d_4a_3x3', 'Mixed_4b', 'Mixed_4c', 'Mixed_4d', 'Mixed_4e', 'Mixed_4f', 'MaxPool3d_5a_2x2', 'Mixed_5b', 'Mixed_5c',
                       'logits')
    LENGTH = 16      # the clip length the network was trained at; selects the native variant
    POOL_T = 2       # AvgPool3d((POOL_T, 7, 7))
    feature_dim = 1024

    def __init__(self, num_classes=400, spatial_squeeze=True, final_endpoint='logits', name='inception_i3d', in_channels=3,
                 dropout_keep_prob=1.0):
        if final_endpoint not in self.VALID_ENDPOINTS:
            raise ValueError('Unknown final endpoint %s' % final_endpoint)
        if final_endpoint != 'logits':
            raise NotImplementedError(f"InceptionI3D: only the full network (final_endpoint='logits') is built, got {final_endpoint!r}")
        if in_channels != 3:
            raise NotImplementedError(f"InceptionI3D: only the rgb network (3 input channels) is built, got {in_channels}")
        super().__init__()
        self._model_name, self._num_classes, self._spatial_squeeze, self._final_endpoint = name, num_classes, spatial_squeeze, final_endpoint
        self._dropout_rate = 1.0 - dropout_keep_prob
        self.Conv3d_1a_7x7 = Unit3D(in_channels, 64, kernel_size=(7, 7, 7), stride=(2, 2, 2), padding=3, name=name + 'Conv3d_1a_7x7')
        self.Conv3d_2b_1x1 = Unit3D(64, 64, name=name + 'Conv3d_2b_1x1')
        self.Conv3d_2c_3x3 = Unit3D(64, 192, kernel_size=(3, 3, 3), padding=1, name=name + 'Conv3d_2c_3x3')
        for mname, cin, o in MIXED:
            setattr(self, mname, InceptionModule(cin, list(o), name + mname))
        self.logits = Unit3D(1024, num_classes, activation_fn=None, use_batch_norm=False, use_bias=True, name=name + 'logits')
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
            raise i2v_native.I2VError("the dynamic-texture I3D runs on a HIP device only (csrc/i2v_i3d.hip); this package has no CPU fallback -- "
                                      "move the module and its input to 'cuda'")
        key = self._state_key()
        if self._native is None or self._native_key != key:
            if self._native is None or self._native.device != p.device:
                self._native = i2v_native.NativeI3D(self._num_classes, 3, device=p.device, dt_length=self.LENGTH)
            self._native.load({k: v for k, v in self.state_dict().items() if not k.endswith("num_batches_tracked")})
            self._native_key = key
        return self._native

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._native_key = None

    def trainable_params(self):
        return [p for p in self.parameters() if p.requires_grad]

    def features(self, frames, denorm=False, t_out=None):
        """frames [B, T_in, 3, H, W] fp32 on the device, any H, W (the resize to 224 x 224 is the handle's input stage; nothing is
        materialised at 224 x 224) -> [B, 1024, T'].  ``t_out`` frames enter the network, frame t read from source frame t % T_in."""
        return self.native().features(frames.float().contiguous(), denorm, t_out)

    def forward_frames(self, frames, denorm=False, t_out=None):
        """The product path: frames [B, T, 3, H, W] on the device -> [B, 1024].  Requires T' == 1, as the reference's 1024-wide
        ``pred_arr`` does (``get_activations``)."""
        rep = self.features(frames, denorm, t_out)
        if rep.shape[2] != 1:
            raise ValueError(f"InceptionI3D.forward_frames: {frames.shape[1] if t_out is None else t_out} frames leave {rep.shape[2]} time steps "
                             f"behind the average pool; the 1024-wide feature needs exactly one (length {self.LENGTH})")
        return rep[:, :, 0]

    @torch.no_grad()
    def get_representation(self, x):
        """Reference signature: ``x`` [B, 3, T, 224, 224], values as they are -> [B, 1024, T'] (the two ``squeeze(3)`` applied)."""
        if x.dim() != 5 or x.shape[1] != 3:
            raise ValueError(f"InceptionI3D.get_representation: expected [B,3,T,224,224], got {tuple(x.shape)}")
        if tuple(x.shape[3:]) != (224, 224):
            raise ValueError(f"InceptionI3D.get_representation: expected 224 x 224 frames as the reference is fed, got {tuple(x.shape[3:])}; "
                             "forward_frames takes frames of any size and resizes on the device")
        rep = self.features(x.permute(0, 2, 1, 3, 4))
        return rep if self._spatial_squeeze else rep[:, :, :, None, None]

    def forward(self, x):
        raise NotImplementedError("InceptionI3D.forward (the logits) is not built: DTFVD and the diversity score read get_representation, the "
                                  "classifier is never run")

    def replace_logits(self, num_classes, device='cuda:0'):
        raise NotImplementedError("InceptionI3D.replace_logits is not built: training the dynamic-texture I3D is out of scope")
