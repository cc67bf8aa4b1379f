"""The handle lifecycle on the GPU, per handle type with a small state_dict: a forward before load is refused (I2V_E_STATE), a load
with a required key missing is refused (I2V_E_MISSING) and LEAVES THE HANDLE UNLOADED -- its next forward is refused too -- a good
load after it gives the first forward's bits again, and a workspace one byte short is refused (I2V_E_WORKSPACE) without harming the
handle.  Every refusal happens on the host, before any launch.  The embedder, I3D, VGG-16 and Inception handles go through the same
load wrapper and entry scope (csrc/i2v_handle.h); their state_dicts are tens of megabytes and stay out of this file."""
import ctypes

import numpy as np
import pytest
import torch

import i2v_native
import i2v_synth as synth
from i2v_native import I2VError

import encoder_cfgs as ec
import flow_units_common as fu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

E_INVALID, E_MISSING, E_WORKSPACE, E_STATE = -1, -2, -4, -5
NF, ZD = 8, 64   # the decoder's smallest channel_factor


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


_DEC_SD = {}


def _decoder_sd():
    if not _DEC_SD:
        _DEC_SD.update(_t(synth.decoder_state_dict(seed=5, channel_factor=NF, z_dim=ZD)))
    return _DEC_SD


class MLP:
    drop = "main.4.bias"

    def make(self):
        return i2v_native.NativeMLP(8, 16, 1, 8)

    def state_dict(self):
        g = torch.Generator().manual_seed(11)
        return {f"main.{2 * i}.{p}": torch.randn(*s, generator=g) * 0.3
                for i, (o, k) in enumerate(((16, 8), (16, 16), (8, 16))) for p, s in (("weight", (o, k)), ("bias", (o,)))}

    def inputs(self):
        return (_rand(5, 8, seed=1),)

    def forward(self, h, x):
        return h.forward(x)

    def raw(self, h, short, x):
        y = torch.empty(5, 8, device="cuda")
        n = i2v_native.lib().i2v_mlp_workspace_bytes(h._h, 5)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return i2v_native.lib().i2v_mlp_forward(h._h, x.data_ptr(), y.data_ptr(), ws.data_ptr(), n - short, 5, _stream())


class Flow:
    case = min(fu.CASES, key=lambda c: (c["hidden"], c["depth"], c["E"]))   # hidden 64, depth 0, E = 1: the generic chain
    drop = f"sub_layers.{fu.NFL - 1}.coupling.t.1.main.2.bias"

    def make(self):
        c = self.case
        return i2v_native.NativeFlow(64, c["E"], c["hidden"], c["depth"], fu.NFL, control=c["control"])

    def state_dict(self):
        return fu.tensors(fu.state_dict(self.case))

    def inputs(self):
        return _rand(5, 64, seed=2), _rand(5, self.case["E"], seed=3).abs()

    def forward(self, h, x, e):
        return h.inverse(x, e)

    def raw(self, h, short, x, e):
        out = torch.empty_like(x)
        n = i2v_native.lib().i2v_flow_workspace_bytes(h._h, 5)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return i2v_native.lib().i2v_flow_inverse(h._h, x.data_ptr(), e.data_ptr(), out.data_ptr(), ws.data_ptr(), n - short, 5, _stream())


class GBlock:
    drop = "norm_1.linear.bias"   # (behind the convs and SPADE in the packing order: they are repacked before the load fails)
    n_in, n_out = 2 * NF, NF      # g_4 of the smallest decoder: the narrowest block with a learned shortcut
    geom = (1, 4, 8, 8)           # B, T, H, W

    def make(self):
        return i2v_native.NativeGBlock(self.n_in, self.n_out, ZD, mma=1)

    def state_dict(self):
        return {k[len("g_4."):]: v for k, v in _decoder_sd().items() if k.startswith("g_4.")}

    def inputs(self):
        B, T, H, W = self.geom
        return _rand(B, self.n_in, T, H, W, seed=4), _rand(B, ZD, seed=5), _rand(B, 3, 16, 16, seed=6).tanh()

    def forward(self, h, x, z, img):
        return h.forward(x, z, img)

    def raw(self, h, short, x, z, img):
        B, T, H, W = self.geom
        out = torch.empty(B, self.n_out, T, H, W, device="cuda")
        n = i2v_native.lib().i2v_gblock_workspace_bytes(h._h, B, T, H, W)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return i2v_native.lib().i2v_gblock_forward(h._h, x.data_ptr(), z.data_ptr(), img.data_ptr(), 16, 16, out.data_ptr(), ws.data_ptr(), n - short,
                                                   B, T, H, W, _stream())


class Encoder3D:
    case = ec.CASES["c0_16"]      # 16-channel stem, the minimum width everywhere
    drop = "conv_var.bias"
    geom = (1, 16, 64, 64)        # B, T, H, W

    def make(self):
        a = self.case["synth"]
        return i2v_native.NativeEncoder3D(a["z_dim"], a["channels"], a["stride_s"], self.case["stride_t"])

    def state_dict(self):
        return _t(synth.encoder3d_state_dict(**self.case["synth"]))

    def inputs(self):
        B, T, H, W = self.geom
        return (_rand(B, 3, T, H, W, seed=7).tanh(),)

    def forward(self, h, x):
        return torch.cat(h.forward(x)[1:], 1)   # mu | logvar

    def raw(self, h, short, x):
        B, T, H, W = self.geom
        mu, lv = torch.empty(B, ec.Z_DIM, device="cuda"), torch.empty(B, ec.Z_DIM, device="cuda")
        n = i2v_native.lib().i2v_encoder3d_workspace_bytes(h._h, B, T, H, W)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return i2v_native.lib().i2v_encoder3d_forward(h._h, x.data_ptr(), T, H, W, None, None, mu.data_ptr(), lv.data_ptr(), ws.data_ptr(), n - short, B,
                                                      _stream())


class Decoder:
    drop = "conv_img.bias"        # the last key the packer reads: everything else is repacked before the load fails

    def make(self):
        return i2v_native.NativeDecoder(NF, ZD, [2, 1], [2, 1], spectral_norm=True, mma=1)

    def state_dict(self):
        return _decoder_sd()

    def inputs(self):
        return _rand(1, 3, 64, 64, seed=8).tanh(), _rand(1, ZD, seed=9)

    def forward(self, h, img, z):
        return h.forward(img, z)

    def raw(self, h, short, img, z):
        T, H, W = h.out_shape
        out = torch.empty(1, T, 3, H, W, device="cuda")
        n = i2v_native.lib().i2v_dec_workspace_bytes(h._h, 1, 64, 64)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return i2v_native.lib().i2v_dec_forward(h._h, img.data_ptr(), 64, 64, z.data_ptr(), out.data_ptr(), ws.data_ptr(), n - short, 1, _stream())


@pytest.mark.parametrize("kind", [MLP, Flow, GBlock, Encoder3D, Decoder], ids=lambda k: k.__name__)
def test_lifecycle(kind):
    k = kind()
    lib = i2v_native.lib()
    h, sd, x = k.make(), k.state_dict(), k.inputs()
    assert k.drop in sd
    with pytest.raises(I2VError, match=rf"failed \({E_STATE}\)"):     # 1. never loaded
        k.forward(h, *x)
    h.load(sd)                                                         # 2.
    y0 = k.forward(h, *x).clone()
    assert torch.isfinite(y0).all() and float(y0.abs().max()) > 0
    with pytest.raises(I2VError, match=rf"failed \({E_MISSING}\).*{k.drop}"):   # 3. a reload that fails half-way unloads the handle
        h.load({key: v for key, v in sd.items() if key != k.drop})
    with pytest.raises(I2VError, match=rf"failed \({E_STATE}\)"):
        k.forward(h, *x)
    assert k.raw(h, 0, *x) == E_STATE
    h.load(sd)                                                         # 4. the same bits after a good load
    assert torch.equal(k.forward(h, *x), y0)
    assert k.raw(h, 1, *x) == E_WORKSPACE                              # 5. one byte short: refused, and the handle is unharmed
    assert b"workspace" in lib.i2v_last_error()
    assert k.raw(h, 0, *x) == 0
    assert torch.equal(k.forward(h, *x), y0)
    torch.cuda.synchronize()


def test_handle_refuses_another_current_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices: a handle of device 0 called with device 1 current")
    k = MLP()
    with torch.cuda.device(0):
        h = k.make()
        h.load(k.state_dict())
        x = k.inputs()
    with torch.cuda.device(1):
        assert k.raw(h, 0, *x) == E_INVALID
        assert b"lives on HIP device" in i2v_native.lib().i2v_last_error()
