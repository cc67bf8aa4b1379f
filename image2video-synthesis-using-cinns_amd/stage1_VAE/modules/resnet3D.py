"""Mirror of the motion encoder of the reference's ``stage1_VAE/modules/resnet3D.py`` (``Encoder``, lines 138-219; row N3
of the coverage contract): 3D ResNet-18 with GroupNorm(16), ``conv_mu`` / ``conv_var`` heads.  The modules carry the
reference's state_dict keys (``conv1.weight``, ``norm1.*``, ``layer.{L}.{i}.conv{1,2}.weight``, ``.bn{1,2}.*``,
``.downsample.{0.weight,1.*}``, ``conv_mu.*``, ``conv_var.*``); the arithmetic runs in libi2v_hip.so (csrc/i2v_encoder.hip).
The temporal discriminator of the same reference file (``Discriminator``, lines 222-301) follows below the Encoder, on csrc/i2v_disc3d.hip;
below it, the Encoder's opt-in training path (``Encoder.differentiable``) on csrc/i2v_encoder_train.hip."""
import torch
import torch.nn as nn

import i2v_native as native
from i2v_params import AffineParams, ConvParams, NativeBacked, _NoForward


class BasicBlock(_NoForward):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, stride_t=1, downsample=None, spectral=False):
        super().__init__()
        if spectral:
            raise NotImplementedError("the Encoder never enables spectral norm (resnet3D.py:153)")
        self.conv1 = ConvParams(inplanes, planes, 3, 3, bias=False)
        self.bn1 = AffineParams(planes)
        self.conv2 = ConvParams(planes, planes, 3, 3, bias=False)
        self.bn2 = AffineParams(planes)
        if downsample is not None:
            self.downsample = downsample
        self.stride = stride


class _StemConv(_NoForward):
    def __init__(self, cout):
        super().__init__()
        w = torch.empty(cout, 3, 3, 7, 7)
        nn.init.kaiming_normal_(w, mode="fan_out")
        self.weight = nn.Parameter(w)


class Encoder(NativeBacked):
    def __init__(self, dic):
        super().__init__()
        if dic["res_type_encoder"] != "resnet18":
            raise NotImplementedError("Encoder: every shipped config uses res_type_encoder 'resnet18'")
        self.use_max_pool = dic["use_max_pool"]
        if self.use_max_pool:
            raise NotImplementedError("Encoder: use_max_pool is false in every shipped config")
        self.z_dim = dic["z_dim"]
        self.channels = list(dic["channels"])
        self.stride_s = list(dic["stride_s"])
        self.stride_t = list(dic["stride_t"])
        assert len(self.channels) - 1 == len(self.stride_t) == len(self.stride_s) == 4
        self.conv1 = _StemConv(self.channels[0])
        self.norm1 = AffineParams(self.channels[0])
        inplanes = self.channels[0]
        layers = []
        for i, ch in enumerate(self.channels[1:]):
            down = None
            if self.stride_s[i] == 1 and self.stride_t[i] == 2 and inplanes == ch:
                # no downsample branch is built for this layer (next line), so the reference's `out += residual` fails on the
                # halved time extent (resnet3D.py:132); i2v_encoder3d_create refuses the same configuration
                raise ValueError(f"Encoder: layer {i} has stride_t 2 with stride_s 1 and equal widths ({ch}): it has no downsample "
                                 "branch for its half-rate residual")
            if self.stride_s[i] != 1 or inplanes != ch:                      # resnet3D.py:180
                down = nn.Sequential(ConvParams(inplanes, ch, 3, 3, bias=False), AffineParams(ch))
            layers.append(nn.Sequential(BasicBlock(inplanes, ch, self.stride_s[i], self.stride_t[i], down), BasicBlock(ch, ch)))
            inplanes = ch
        self.layer = nn.Sequential(*layers)
        self.conv_mu = ConvParams(self.channels[-1], self.z_dim, 4, 2, bias=True)
        self.conv_var = ConvParams(self.channels[-1], self.z_dim, 4, 2, bias=True)

    def _build_native(self):
        h = native.NativeEncoder3D(self.z_dim, self.channels, self.stride_s, self.stride_t, device=self.module_device())
        h.load(self.state_dict())
        return h

    def forward(self, x):
        """x [B,3,T,H,W] (or [B,T,3,H,W], transposed like the reference when dim 1 > dim 2) -> (sample, mu, logvar);
        sample = eps * exp(0.5 logvar) + mu with eps drawn on the CPU generator (resnet3D.py:199-203)."""
        if x.size(1) > x.size(2):
            x = x.transpose(1, 2)
        x = x.contiguous()
        eps = torch.randn(x.size(0), self.z_dim).to(x.device)
        return self.native().forward(x, eps)


# ---------------------------------------------------------------------------------------------------------------- Discriminator
# The temporal discriminator ``disc_t`` of stage-1 training (reference resnet3D.py:222-301) on csrc/i2v_disc3d.hip (C ABI:
# include/i2v_hip_disc3d.h).  State-dict keys, shapes and dtypes are the reference's, so a ``latest_checkpoint_DISC_t.pth`` loads unchanged:
# ``conv1.weight``, ``norm1.*``, ``layer.L.0.conv{1,2}.{weight_orig,weight_u,weight_v}``, ``layer.L.1.conv{1,2}.weight``,
# ``layer.L.i.bn{1,2}.*``, ``layer.L.0.downsample.0.{weight_orig,weight_u,weight_v}``, ``layer.L.0.downsample.1.*``, ``fc.weight``.
# Semantics kept:
#   * spectral norm covers conv1 / conv2 of block 0 of a layer (``spectral_norm`` of the config) and the downsample conv (always); block
#     1, the stem and ``fc`` are plain.  Training mode does one power iteration per wrapped conv and forward, in place; eval mode uses the
#     stored vectors.  A backward uses the u, v and sigma of ITS forward; ``weight_orig`` and the GroupNorm weights are read when the
#     backward runs, so they must not change between a forward and its backward;
#   * the downsample branch exists when ``stride != 1 or inplanes != planes or stride_t != 1`` (the Encoder's rule lacks the last term);
#   * ``nn.init.orthogonal_`` reaches ``m.weight`` of every Conv3d; on a spectral-normed conv that attribute is ``weight_orig.data`` (what
#     ``spectral_norm`` leaves there until the first forward), so the in-place init lands in ``weight_orig`` as well.  The constructor makes
#     the reference's draws in the reference's order (the default init of every conv and the u, v draws come first and are overwritten);
#   * ``x`` is transposed when ``x.size(1) > x.size(2)``.
# One difference: the reference starts the layers from ``inplanes = 64`` whatever ``channels[0]`` is (so it only runs with a 64-wide stem,
# as in every shipped config); here the first layer takes ``channels[0]`` inputs, which is the same network at 64 and a working one below.
# In grad mode ``forward`` returns tensors with a ``grad_fn`` (once differentiable: ``create_graph=True`` raises; the gradient penalty with
# its gradient is ``forward_with_penalty``, which needs no general double backward);
# the parameters are inputs of the Function; a frozen module skips the weight-gradient launches.  CPU tensors raise ``I2VError``.


class _DiscInside(_NoForward):
    pass


class _DiscConv(_DiscInside):
    """nn.Conv3d(cin, cout, kernel, bias=False) with its default init, optionally as torch.nn.utils.spectral_norm leaves it."""

    def __init__(self, cin, cout, kernel=(3, 3, 3)):
        super().__init__()
        self.weight = nn.Parameter(nn.Conv3d(cin, cout, kernel_size=kernel, bias=False).weight.data)
        self.spectral = False

    def wrap_spectral(self, eps=1e-12):
        w = self.weight
        del self.weight
        self.register_parameter("weight_orig", w)
        with torch.no_grad():
            u = nn.functional.normalize(w.new_empty(w.shape[0]).normal_(0, 1), dim=0, eps=eps)
            v = nn.functional.normalize(w.new_empty(w[0].numel()).normal_(0, 1), dim=0, eps=eps)
        self.register_buffer("weight_u", u)
        self.register_buffer("weight_v", v)
        self.spectral = True
        return self

    def init_orthogonal(self):
        """``m.weight = nn.init.orthogonal_(m.weight)`` (resnet3D.py:259-261): on a wrapped conv ``m.weight`` shares ``weight_orig``'s storage."""
        with torch.no_grad():
            nn.init.orthogonal_(self.weight_orig if self.spectral else self.weight)


class DiscBasicBlock(_DiscInside):
    """BasicBlock as the Discriminator builds it (resnet3D.py:101-117): registration order conv1, bn1, conv2, bn2, downsample."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, stride_t=1, downsample=None, spectral=False):
        super().__init__()
        self.conv1 = _DiscConv(inplanes, planes)
        self.bn1 = AffineParams(planes)
        self.conv2 = _DiscConv(planes, planes)
        self.bn2 = AffineParams(planes)
        if downsample is not None:
            self.downsample = downsample
        self.stride, self.stride_t = stride, stride_t
        if spectral:
            self.conv1.wrap_spectral()
            self.conv2.wrap_spectral()


class _Disc3DFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, *params):
        pred, fmaps, saved = module._run(x, save=True)
        ctx.module, ctx.saved, ctx.shape = module, saved, tuple(x.shape)
        return (pred, *[f.permute(0, 4, 1, 2, 3) for f in fmaps])

    @staticmethod
    def backward(ctx, d_pred, *d_fmaps):
        if torch.is_grad_enabled():   # create_graph=True: a graph through this backward is asked for
            raise NotImplementedError("resnet3D.Discriminator is once differentiable: the double backward (create_graph=True, the gradient "
                                      "penalty's gradient) is not built")
        module = ctx.module
        want = ctx.needs_input_grad[2:]
        grads = native.flat_param_grads(module, ctx.saved.device) if any(want) else None
        h = module._handle(grads)
        cl = [None if g is None else g.permute(0, 2, 3, 4, 1).contiguous().float() for g in d_fmaps]
        dx = h.backward(None if d_pred is None else d_pred.contiguous().float(), cl, ctx.saved, ctx.shape, need_dx=ctx.needs_input_grad[1],
                        param_grads=grads is not None, accumulate=False)
        out = [None] * len(want) if grads is None else [g if w else None for g, w in zip(grads.values(), want)]
        return (None, dx, *out)


class _Disc3DPenaltyFunction(torch.autograd.Function):
    """``forward_with_penalty``: the module's forward plus the penalty of ``mean(pred)`` at ``x`` from the same saved forward.  Backward:
    the existing backward for ``d_pred`` / ``d_fmaps``, plus ``gp_backward`` scaled by the upstream of ``L_GP``, which stays a device
    scalar.  The penalty's value is formed in ``forward`` by the input-gradient backward and ``disc3d_sumsq`` (the bits of
    ``TemporalDiscTrainer.gradient_penalty``); ``gp_backward`` forms the gradient at the clips again, one input-gradient pass in exchange
    for holding no second clip-sized tensor between forward and backward."""

    @staticmethod
    def forward(ctx, module, x, *params):
        pred, fmaps, saved = module._run(x, save=True)
        shape = tuple(x.shape)
        dx = module._handle().backward(module._penalty_seed(pred), None, saved, shape, need_dx=True, param_grads=False)
        l_gp = native.disc3d_sumsq(dx).mean()
        ctx.module, ctx.saved, ctx.shape = module, saved, shape
        ctx.set_materialize_grads(False)
        return (pred, l_gp, *[f.permute(0, 4, 1, 2, 3) for f in fmaps])

    @staticmethod
    def backward(ctx, d_pred, d_lgp, *d_fmaps):
        if torch.is_grad_enabled():   # create_graph=True: a graph through this backward is asked for
            raise NotImplementedError("resnet3D.Discriminator.forward_with_penalty is once differentiable: a general double backward "
                                      "(create_graph=True) is not built")
        module = ctx.module
        want = ctx.needs_input_grad[2:]
        first = d_pred is not None or any(g is not None for g in d_fmaps)
        grads = native.flat_param_grads(module, ctx.saved.device) if any(want) else None
        h = module._handle(grads)
        dx = None
        if first and (grads is not None or ctx.needs_input_grad[1]):
            cl = [None if g is None else g.permute(0, 2, 3, 4, 1).contiguous().float() for g in d_fmaps]
            dx = h.backward(None if d_pred is None else d_pred.contiguous().float(), cl, ctx.saved, ctx.shape, need_dx=ctx.needs_input_grad[1],
                            param_grads=grads is not None, accumulate=False)
        elif grads is not None:
            for g in grads.values():
                g.zero_()
        if d_lgp is not None and grads is not None:   # (the penalty has no gradient at the clips: the reference's seq_real is data)
            h.gp_backward(ctx.saved, ctx.shape, scale=1.0, scale_dev=d_lgp.detach().to(torch.float32).reshape(1).contiguous(), accumulate=True)
        out = [None] * len(want) if grads is None else [g if w else None for g, w in zip(grads.values(), want)]
        return (None, dx, *out)


class Discriminator(nn.Module):
    """resnet3D.Discriminator(dic) (reference resnet3D.py:222-301): ``forward(x) -> (pred [B, 1], [fmap0 .. fmap3])``."""

    def __init__(self, dic):
        super().__init__()
        if dic["res_type_encoder"] != "resnet18":
            raise NotImplementedError(f"Discriminator: res_type_encoder {dic['res_type_encoder']!r} is not built (every shipped config uses 'resnet18')")
        self.use_spectral_norm = bool(dic["spectral_norm"])
        self.use_max_pool = bool(dic["use_max_pool"])
        channels, stride_s, stride_t = list(dic["channels"]), list(dic["stride_s"]), list(dic["stride_t"])
        assert len(channels) - 1 == len(stride_t)
        assert len(channels) - 1 == len(stride_s)
        if len(channels) != 5 or any(c <= 0 or c % 16 for c in channels) or any(s not in (1, 2) for s in stride_s + stride_t):
            raise native.I2VError(f"Discriminator: channels {channels} (five multiples of 16) or strides {stride_s} / {stride_t} (1 or 2) are not built")
        self.cfg = dict(channels=channels, stride_s=stride_s, stride_t=stride_t, use_max_pool=self.use_max_pool, spectral_norm=self.use_spectral_norm)

        self.conv1 = _DiscConv(3, channels[0], (3, 7, 7))
        self.norm1 = AffineParams(channels[0])
        self.inplanes = channels[0]
        layers = []
        for i, ch in enumerate(channels[1:]):
            layers.append(self._make_layer(ch, 2, stride=stride_s[i], stride_t=stride_t[i]))
        self.layer = nn.Sequential(*layers)
        self.fc = _DiscInside()
        self.fc.weight = nn.Parameter(nn.Linear(channels[-1], 1, bias=False).weight.data)
        for m in self.modules():
            if isinstance(m, _DiscConv):
                m.init_orthogonal()
        object.__setattr__(self, "_native", None)

    def _make_layer(self, planes, blocks, stride=1, stride_t=1):
        downsample = None
        if stride != 1 or self.inplanes != planes or stride_t != 1:
            downsample = nn.Sequential(_DiscConv(self.inplanes, planes).wrap_spectral(), AffineParams(planes))
        layers = [DiscBasicBlock(self.inplanes, planes, stride, stride_t, downsample, self.use_spectral_norm)]
        self.inplanes = planes
        for _ in range(1, blocks):
            layers.append(DiscBasicBlock(self.inplanes, planes))
        return nn.Sequential(*layers)

    def __getstate__(self):
        state = dict(super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__)
        state["_native"] = None
        return state

    # ---- native side
    def _tensors(self):
        return {k: t for k, t in list(self.named_parameters()) + list(self.named_buffers()) if t.dtype == torch.float32}

    def _handle(self, grads=None):
        """The handle, bound to the storage of the parameters as it is now and, when ``grads`` ({parameter name: tensor}) is given, to
        those gradient tensors; the two bindings are kept apart."""
        tensors = self._tensors()
        for t in tensors.values():
            if not t.is_cuda:
                raise native.I2VError("Discriminator runs on a HIP device only: move the module to 'cuda' (this package has no CPU fallback)")
        h = self._native
        dev = next(iter(tensors.values())).device
        if h is None or h.device != dev:
            h = native.NativeDisc3D(device=dev, **self.cfg)
            object.__setattr__(self, "_native", h)
        return native.bind_in_place(h, tensors, grads)

    def _run(self, x, save, grads=None, want_fmaps=True):
        """x [B, 3, T, H, W] -> (pred, channels-last feature maps or None, saved or None); training mode iterates the spectral norm."""
        if not x.is_cuda:
            raise native.I2VError("Discriminator got a CPU tensor: its kernels run on a HIP device only (this package has no CPU fallback)")
        if x.size(1) > x.size(2):
            x = x.transpose(1, 2)
        with torch.no_grad():
            return self._handle(grads).forward(x.detach().float().contiguous(), iterate=self.training, save=save, want_fmaps=want_fmaps)

    def forward(self, x):
        if x.dim() == 5 and x.size(1) > x.size(2):
            x = x.transpose(1, 2)
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            pred, *fmaps = _Disc3DFunction.apply(self, x, *params)
            return pred, list(fmaps)
        pred, fmaps, _ = self._run(x, save=False)
        return pred, [f.permute(0, 4, 1, 2, 3) for f in fmaps]

    @staticmethod
    def _penalty_seed(pred):
        """d mean(pred) / d pred"""
        return torch.full((pred.shape[0], 1), 1.0 / pred.shape[0], dtype=torch.float32, device=pred.device)

    def forward_with_penalty(self, x):
        """-> (pred [B, 1], [fmap0 .. fmap3], L_GP): ``forward(x)`` plus ``gradient_penalty(pred, x)`` of the reference (loss.py:35-43) from
        the SAME forward, so one power iteration as in the reference.  In grad mode all three carry the ``grad_fn`` of one Function, so
        loss.py:98-108 reads ``(hinge_loss(pred_f, pred_r, 'disc') + w_GP * L_GP).backward()`` and any optimiser steps the module.  Once
        differentiable; a frozen module returns the values and launches no weight-gradient kernel; ``x.grad`` receives the ``pred`` /
        ``fmaps`` part only (the penalty's gradient at the clips is not formed: the reference's ``seq_real`` is data)."""
        if x.dim() == 5 and x.size(1) > x.size(2):
            x = x.transpose(1, 2)
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            pred, l_gp, *fmaps = _Disc3DPenaltyFunction.apply(self, x, *params)
            return pred, list(fmaps), l_gp
        with torch.no_grad():
            pred, fmaps, saved = self._run(x, save=True)
            dx = self._handle().backward(self._penalty_seed(pred), None, saved, tuple(x.shape), need_dx=True, param_grads=False)
        return pred, [f.permute(0, 4, 1, 2, 3) for f in fmaps], native.disc3d_sumsq(dx).mean()


# ---------------------------------------------------------------------------------------------------------------- Encoder, training path
# ``Encoder`` as the package exports it: the class above (the packed, forward-only handle of csrc/i2v_encoder.hip) plus the opt-in
# training path on csrc/i2v_encoder_train.hip (C ABI: include/i2v_hip_enc3d_train.h).  ``differentiable`` is a plain attribute, default
# False, not a constructor argument (as ``ConditionalFlow.differentiable``): while it is False every call runs the inference handle
# exactly as before, in grad mode too.  With ``differentiable = True`` every forward runs on the training handle, which reads the
# parameters in place (an optimiser step is seen by the next call, no refresh); in grad mode it returns ``(sample, mu, logvar)`` with a
# ``grad_fn`` from a Function that takes the parameters as inputs; a frozen module skips the weight-gradient launches;
# ``create_graph=True`` raises.  Setting it back to False calls ``refresh_native()``, so the packed handle is rebuilt from the current
# parameters.  ``eps`` is drawn as above (``torch.randn(B, z)`` on the CPU generator) unless the caller passes ``eps=``.

_PackedEncoder = Encoder


class _Enc3DTrainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, eps, *params):
        sample, mu, logvar, saved = module._train_handle().forward(x, eps, save=True)
        ctx.module, ctx.saved, ctx.shape = module, saved, tuple(x.shape)
        ctx.set_materialize_grads(False)   # an output that the loss does not use arrives as None, not as zeros
        return sample, mu, logvar

    @staticmethod
    def backward(ctx, d_sample, d_mu, d_logvar):
        if torch.is_grad_enabled():   # create_graph=True: a graph through this backward is asked for
            raise NotImplementedError("resnet3D.Encoder is once differentiable: the double backward (create_graph=True) is not built")
        module = ctx.module
        want = ctx.needs_input_grad[3:]
        ups = [None if g is None else g.contiguous().float() for g in (d_sample, d_mu, d_logvar)]
        if all(g is None for g in ups):
            return (None,) * (3 + len(want))
        grads = native.flat_param_grads(module, ctx.saved.device) if any(want) else None
        h = module._train_handle(grads)
        dx = h.backward(*ups, ctx.saved, ctx.shape, need_dx=ctx.needs_input_grad[1] or grads is None, param_grads=grads is not None, accumulate=False)
        out = [None] * len(want) if grads is None else [g if w else None for g, w in zip(grads.values(), want)]
        return (None, dx if ctx.needs_input_grad[1] else None, None, *out)


class Encoder(_PackedEncoder):
    def __init__(self, dic):
        super().__init__(dic)
        object.__setattr__(self, "_train_native", None)
        object.__setattr__(self, "_differentiable", False)

    @property
    def differentiable(self):
        return self.__dict__.get("_differentiable", False)

    @differentiable.setter
    def differentiable(self, value):
        value = bool(value)
        if not value and self.differentiable:
            self.refresh_native()
        object.__setattr__(self, "_differentiable", value)

    def _drop_native(self):
        super()._drop_native()
        object.__setattr__(self, "_train_native", None)

    def __getstate__(self):
        state = dict(super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__)
        state["_native"] = state["_train_native"] = None
        return state

    def _train_handle(self, grads=None):
        """The training handle, bound to the storage of the parameters as it is now and, when ``grads`` ({parameter name: tensor}) is
        given, to those gradient tensors."""
        tensors = dict(self.named_parameters())
        for t in tensors.values():
            if not t.is_cuda:
                raise native.I2VError("Encoder runs on a HIP device only: move the module to 'cuda' (this package has no CPU fallback)")
        h = self.__dict__.get("_train_native")
        dev = next(iter(tensors.values())).device
        if h is None or h.device != dev:
            h = native.NativeEnc3DTrain(self.z_dim, self.channels, self.stride_s, self.stride_t, device=dev)
            object.__setattr__(self, "_train_native", h)
        return native.bind_in_place(h, tensors, grads)

    def forward(self, x, eps=None):
        """As the inference forward; ``eps`` [B, z]: the reparameterisation's draw, when the caller supplies it."""
        if not self.differentiable and eps is None:
            return super().forward(x)
        if x.size(1) > x.size(2):
            x = x.transpose(1, 2)
        if not x.is_cuda:
            raise native.I2VError("Encoder got a CPU tensor: its kernels run on a HIP device only (this package has no CPU fallback)")
        if eps is None:
            eps = torch.randn(x.size(0), self.z_dim)
        eps = eps.detach().to(x.device, torch.float32).contiguous()
        if not self.differentiable:
            return self.native().forward(x.detach().float().contiguous(), eps)
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _Enc3DTrainFunction.apply(self, x.float().contiguous(), eps, *params)
        with torch.no_grad():
            return self._train_handle().forward(x.detach().float().contiguous(), eps)[:3]
