"""FID Inception-v3: own implementation of the reference's ``metrics/FID/inception.py`` surface (pytorch-fid's ``InceptionV3``).

``InceptionV3`` is a parameter holder under torchvision's ``Inception3`` keys (``Conv2d_1a_3x3.conv.weight`` ... ``Mixed_7c.branch_pool.bn.*``:
94 ``BasicConv2d`` units = Conv2d without bias, BatchNorm2d(eps=0.001), ReLU); ``forward`` runs on the device through
``csrc/i2v_inception.hip`` and returns the list of the requested blocks as NCHW-shaped tensors, block 3 as ``[N, 2048, 1, 1]``.  torchvision
is not a dependency: the graph -- torchvision's with the pytorch-fid patches (the average pools of Mixed_5b-5d, 6b-6e and 7b leave the padding
out of their divisor, Mixed_7c pools with a MAXIMUM) -- is written out in the native code, and the weights come from the FID checkpoint FILE
``pt_inception-2015-12-05-6726825d.pth`` (its 1008-class ``fc`` and any ``AuxLogits`` are ignored).  Nothing is ever downloaded: without
``path=`` the parameters stay unset and the first use raises ``FileNotFoundError`` naming the file.

KEPT QUIRK: the reference builds ``InceptionV3()`` with ``normalize_input=False`` and feeds the pipeline's frames in [-1, 1] as they are --
the range the network expects -- although the docstring speaks of (0, 1).  The default path therefore applies NO range change; only
``normalize_input=True`` maps ``2 x - 1``.

The returned tensors are NCHW-shaped views of channels-last memory (the layout the kernels write).  Inference only."""
import os

import torch
import torch.nn as nn

import i2v_native

FID_WEIGHTS_FILE = 'pt_inception-2015-12-05-6726825d.pth'


def _a(n, cin, pf):
    return [(n + ".branch1x1", cin, 64, (1, 1), 1, (0, 0)), (n + ".branch5x5_1", cin, 48, (1, 1), 1, (0, 0)),
            (n + ".branch5x5_2", 48, 64, (5, 5), 1, (2, 2)), (n + ".branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (n + ".branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)),
            (n + ".branch_pool", cin, pf, (1, 1), 1, (0, 0))]


def _b(n, cin):
    return [(n + ".branch3x3", cin, 384, (3, 3), 2, (0, 0)), (n + ".branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (n + ".branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def _c(n, cin, c7):
    return [(n + ".branch1x1", cin, 192, (1, 1), 1, (0, 0)), (n + ".branch7x7_1", cin, c7, (1, 1), 1, (0, 0)),
            (n + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3)), (n + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0)),
            (n + ".branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), (n + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
            (n + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), (n + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
            (n + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)), (n + ".branch_pool", cin, 192, (1, 1), 1, (0, 0))]


def _d(n, cin):
    return [(n + ".branch3x3_1", cin, 192, (1, 1), 1, (0, 0)), (n + ".branch3x3_2", 192, 320, (3, 3), 2, (0, 0)),
            (n + ".branch7x7x3_1", cin, 192, (1, 1), 1, (0, 0)), (n + ".branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            (n + ".branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), (n + ".branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def _e(n, cin):
    return [(n + ".branch1x1", cin, 320, (1, 1), 1, (0, 0)), (n + ".branch3x3_1", cin, 384, (1, 1), 1, (0, 0)),
            (n + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), (n + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            (n + ".branch3x3dbl_1", cin, 448, (1, 1), 1, (0, 0)), (n + ".branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            (n + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), (n + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            (n + ".branch_pool", cin, 192, (1, 1), 1, (0, 0))]


# (torchvision key, cin, cout, kernel, stride, padding) of every BasicConv2d, in the order of torchvision's state_dict
UNITS = ([("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)), ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
          ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)), ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0))]
         + _a("Mixed_5b", 192, 32) + _a("Mixed_5c", 256, 64) + _a("Mixed_5d", 288, 64) + _b("Mixed_6a", 288)
         + _c("Mixed_6b", 768, 128) + _c("Mixed_6c", 768, 160) + _c("Mixed_6d", 768, 160) + _c("Mixed_6e", 768, 192)
         + _d("Mixed_7a", 768) + _e("Mixed_7b", 1280) + _e("Mixed_7c", 2048))
IGNORED_PREFIXES = ("fc.", "AuxLogits.")


class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)


def load_fid_state_dict(path):
    """The torchvision-keyed state_dict of the FID checkpoint file at ``path`` (``fc.*`` / ``AuxLogits.*`` dropped)."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"InceptionV3: the FID Inception state_dict file {path!r} does not exist (pytorch-fid's {FID_WEIGHTS_FILE}; "
                                "this package never downloads it -- pass path=...)")
    sd = torch.load(path, map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    return {k: v for k, v in sd.items() if not k.startswith(IGNORED_PREFIXES)}


class InceptionV3(nn.Module):
    """Holder of the FID Inception-v3 parameters; ``forward`` returns the requested output blocks from the native trunk."""

    DEFAULT_BLOCK_INDEX = 3                                  # the 2048 features FID is defined on
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}    # channels of a block -> its index: behind the two stem pools, Mixed_6e, the last pool

    def __init__(self, output_blocks=[DEFAULT_BLOCK_INDEX], resize_input=True, normalize_input=False, requires_grad=False, use_fid_inception=True,
                 path=None):
        if requires_grad:
            raise NotImplementedError("InceptionV3(requires_grad=True) is not built: the native trunk has no backward pass (inference only)")
        if not use_fid_inception:
            raise NotImplementedError("InceptionV3(use_fid_inception=False) is not built: only the FID Inception graph (torchvision's with the "
                                      "pytorch-fid patches) exists natively, and torchvision's ImageNet weights are not part of this package")
        blocks = sorted(set(int(b) for b in output_blocks))   # each requested block is returned once, as the reference's walk does
        if not blocks or blocks[0] < 0 or blocks[-1] > 3:
            raise ValueError(f"InceptionV3: output_blocks must name blocks 0..3, got {list(output_blocks)}")
        super().__init__()
        self.resize_input, self.normalize_input = bool(resize_input), bool(normalize_input)
        self.output_blocks, self.last_needed_block = blocks, blocks[-1]
        for key, cin, cout, kernel, stride, padding in UNITS:
            parent, names = self, key.split(".")
            for name in names[:-1]:
                if not hasattr(parent, name):
                    parent.add_module(name, nn.Module())
                parent = getattr(parent, name)
            parent.add_module(names[-1], BasicConv2d(cin, cout, kernel_size=kernel, stride=stride, padding=padding))
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        self._filled = False
        self._native = None
        self._native_key = None
        if path is not None:
            self.load_state_dict(load_fid_state_dict(path))

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """torchvision keys; the checkpoint's ``fc.*`` (1008 classes) and ``AuxLogits.*`` are accepted and ignored.  A missing or mis-shaped
        entry is an error naming the key (``strict``)."""
        own = {k: v for k, v in state_dict.items() if not k.startswith(IGNORED_PREFIXES)}
        out = super().load_state_dict(own, strict=strict, **kwargs)
        self._filled = True
        self._native_key = None
        return out

    # ---- native handle: packed from the module's own state, re-packed when the state changes
    def _state_key(self):
        return tuple((t.device, t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def native(self):
        if not self._filled:
            raise FileNotFoundError(f"InceptionV3: no weights loaded -- pass path=FILE with pytorch-fid's {FID_WEIGHTS_FILE} (this package never "
                                    "downloads it) or call load_state_dict")
        p = next(self.parameters())
        if not p.is_cuda:
            raise i2v_native.I2VError("InceptionV3 runs on a HIP device only (csrc/i2v_inception.hip); this package has no CPU fallback -- move "
                                      "the module and its input to 'cuda'")
        key = self._state_key()
        if self._native is None or self._native_key != key:
            if self._native is None or self._native.device != p.device:
                self._native = i2v_native.NativeInception(device=p.device)
            self._native.load(self.state_dict())
            self._native_key = key
        return self._native

    @torch.no_grad()
    def blocks_cl(self, inp, out=None):
        """inp [N, 3, H, W] on the device -> the requested blocks channels-last ([N, H', W', C]; block 3: [N, 2048])."""
        x = i2v_native.inception_input_stage(inp.float().contiguous(), self.resize_input, self.normalize_input)
        return self.native().features(x, self.output_blocks, out)

    @torch.no_grad()
    def forward(self, inp):
        """inp [B, 3, H, W] on the device (any H, W with ``resize_input``, else at least 75 x 75) -> [block [B, C, H', W'] for each index
        of ``output_blocks``, ascending]."""
        if inp.dim() != 4 or inp.shape[1] != 3:
            raise ValueError(f"InceptionV3.forward: expected [B,3,H,W], got {tuple(inp.shape)}")
        if not inp.is_cuda:
            raise i2v_native.I2VError("InceptionV3.forward takes images on a HIP device (csrc/i2v_inception.hip); this package has no CPU "
                                      "fallback -- move the module and its input to 'cuda'")
        outs = self.blocks_cl(inp)
        return [t.view(t.shape[0], t.shape[1], 1, 1) if b == 3 else t.permute(0, 3, 1, 2) for b, t in zip(self.output_blocks, outs)]


def fid_inception_v3(path=None):
    """The reference's builder name: the holder with all four blocks' parameters, filled from ``path``."""
    return InceptionV3(path=path)
