"""Mirror of the reference's ``stage1_VAE/modules/patch_disc.py``: ``weights_init``, ``ActNorm`` and ``NLayerDiscriminator(config)``, the
spatial discriminator ``disc_s`` of stage-1 training, on csrc/i2v_patchdisc.hip (C ABI: include/i2v_hip_disc.h).

State-dict keys, shapes and dtypes are the reference's (``main.{0,2,5,8,11}.{bias,weight_orig,weight_u,weight_v}``,
``main.{3,6,9}.{loc,scale,initialized}`` at n_layers 3), so a ``latest_checkpoint_DISC_s.pth`` loads unchanged.  Semantics kept:
  * spectral norm in training mode does one power iteration per conv and forward, in place on ``weight_u`` / ``weight_v``; eval mode uses
    the stored vectors.  A backward uses the u, v and sigma of ITS forward (they are part of that forward's saved state).  That covers
    those three and the normalised weights only: ``weight_orig``, ``loc`` and ``scale`` are read when the backward runs, so a parameter
    changed between a forward and its backward (stock autograd would raise a version error) gives an inconsistent gradient silently;
  * ActNorm's first training forward sets ``loc = -mean`` and ``scale = 1 / (std + 1e-6)`` per channel from that conv's output;
  * ``weights_init(self.main)`` is called on the Sequential, whose class name matches neither branch: the convs keep nn.Conv2d's
    default init (the reference's behaviour, kept), and every conv has a bias.
``use_actnorm: False`` (BatchNorm2d) is refused: not built.  CPU tensors raise ``I2VError``: there is no fallback.

In grad mode ``forward`` returns a tensor with a ``grad_fn`` (once differentiable; the parameters are inputs of the Function, so ``.grad``,
``zero_grad`` and detached inputs behave as with stock modules); a frozen module skips the weight-gradient launches and an input that
does not require grad the first layer's input gradient."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import i2v_native as native


def weights_init(m):
    classname = m.__class__.__name__
    if classname.find('Conv') != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find('BatchNorm') != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class _Inside(nn.Module):
    """A layer of ``NLayerDiscriminator.main``: it holds parameters under the reference's keys; the network's forward is one native call."""

    def forward(self, *args, **kwargs):
        raise native.I2VError(f"{type(self).__name__} holds parameters of NLayerDiscriminator, whose forward runs all layers natively; "
                              "it has no forward of its own (this package has no eager fallback)")


class ActNorm(_Inside):
    def __init__(self, num_features, logdet=False, affine=True, allow_reverse_init=False):
        assert affine
        super().__init__()
        if logdet:
            raise NotImplementedError("ActNorm(logdet=True) is not built: the patch discriminator never uses it")
        self.logdet = logdet
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.allow_reverse_init = allow_reverse_init
        self.register_buffer('initialized', torch.tensor(0, dtype=torch.uint8))

    def reverse(self, output):
        raise NotImplementedError("ActNorm.reverse is not built: the patch discriminator never uses it")


class _Conv4x4(_Inside):
    """nn.Conv2d(cin, cout, 4, stride, 1) with its default init, optionally as torch.nn.utils.spectral_norm leaves it: ``weight_orig``
    with the buffers ``weight_u`` / ``weight_v`` (drawn in the order and with the calls of SpectralNorm.apply)."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        conv = nn.Conv2d(cin, cout, kernel_size=4, stride=stride, padding=1)
        self.in_channels, self.out_channels, self.stride, self.spectral = cin, cout, stride, False
        self.weight = nn.Parameter(conv.weight.data)
        self.bias = nn.Parameter(conv.bias.data)

    def wrap_spectral(self, eps=1e-12):
        w = self.weight
        del self.weight
        self.register_parameter("weight_orig", w)
        with torch.no_grad():
            u = F.normalize(w.new_empty(w.shape[0]).normal_(0, 1), dim=0, eps=eps)
            v = F.normalize(w.new_empty(w[0].numel()).normal_(0, 1), dim=0, eps=eps)
        self.register_buffer("weight_u", u)
        self.register_buffer("weight_v", v)
        self.spectral = True


class _PatchDiscFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, *params):
        pred, saved = module._run(x, save=True)
        ctx.module, ctx.saved, ctx.shape = module, saved, tuple(x.shape)
        return pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_pred):
        module = ctx.module
        want = ctx.needs_input_grad[2:]
        grads = native.flat_param_grads(module, d_pred.device) if any(want) else None
        h = module._handle(grads)
        dx = h.backward(d_pred.contiguous(), ctx.saved, ctx.shape, need_dx=ctx.needs_input_grad[1], param_grads=grads is not None, accumulate=False)
        out = [None] * len(want) if grads is None else [g if w else None for g, w in zip(grads.values(), want)]
        return (None, dx, *out)


def _forget_init(module, incompatible):
    module.forget_init()


class NLayerDiscriminator(nn.Module):
    """Defines a PatchGAN discriminator as in Pix2Pix (reference patch_disc.py:101-165)."""

    def __init__(self, config):
        super().__init__()
        input_nc, ndf, n_layers = config["in_channels"], config["ndf"], config["n_layers"]
        use_actnorm, use_spectral = config["use_actnorm"], config["spectral_norm"]
        if not use_actnorm:
            raise NotImplementedError("NLayerDiscriminator: use_actnorm False (BatchNorm2d) is not built; every shipped stage-1 config uses ActNorm")
        self.cfg = dict(in_channels=int(input_nc), ndf=int(ndf), n_layers=int(n_layers), use_actnorm=True, spectral_norm=bool(use_spectral))
        if input_nc != 3 or ndf % 16 != 0 or not 1 <= n_layers <= 6:
            raise native.I2VError(f"NLayerDiscriminator: in_channels {input_nc} (3), ndf {ndf} (a multiple of 16) or n_layers {n_layers} (1..6) is not built")
        sequence = [_Conv4x4(input_nc, ndf, 2), nn.LeakyReLU(0.2, True)]
        nf_mult = 1
        for n in range(1, n_layers):
            nf_mult_prev, nf_mult = nf_mult, min(2 ** n, 8)
            sequence += [_Conv4x4(ndf * nf_mult_prev, ndf * nf_mult, 2), ActNorm(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        nf_mult_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        sequence += [_Conv4x4(ndf * nf_mult_prev, ndf * nf_mult, 1), ActNorm(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        sequence += [_Conv4x4(ndf * nf_mult, 1, 1)]
        if use_spectral:
            for lay in sequence:
                if isinstance(lay, _Conv4x4):
                    lay.wrap_spectral()
        self.main = nn.Sequential(*sequence)
        weights_init(self.main)   # the Sequential itself: neither branch matches, nothing is re-initialised (kept quirk)
        # Host-side state, not part of the module's value: the native handle and the remembered answer of "is ActNorm initialised".
        # Both are dropped by copy.deepcopy / pickling (__getstate__) and rebuilt on the next forward.  ``_init_done`` follows
        # load_state_dict; code that writes an ``initialized`` buffer directly must call ``forget_init()``.
        object.__setattr__(self, "_native", None)
        object.__setattr__(self, "_init_done", None)
        self.register_load_state_dict_post_hook(_forget_init)

    def __getstate__(self):
        state = dict(super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__)
        state["_native"], state["_init_done"] = None, None
        return state

    def forget_init(self):
        """Read the ActNorm ``initialized`` buffers again at the next training forward."""
        object.__setattr__(self, "_init_done", None)

    # ---- native side
    def _tensors(self):
        return {k: t for k, t in list(self.named_parameters()) + list(self.named_buffers()) if t.dtype == torch.float32}

    def _handle(self, grads=None):
        """The handle, bound to the storage of the parameters as it is now and, when ``grads`` ({parameter name: tensor}) is given, to
        those gradient tensors; the two bindings are kept apart, so a forward never re-binds because of a backward's gradient buffer."""
        tensors = self._tensors()
        for t in tensors.values():
            if not t.is_cuda:
                raise native.I2VError("NLayerDiscriminator runs on a HIP device only: move the module to 'cuda' (this package has no CPU fallback)")
        h = self._native
        dev = next(iter(tensors.values())).device
        if h is None or h.device != dev:
            h = native.NativePatchDisc(device=dev, **self.cfg)
            object.__setattr__(self, "_native", h)
        return native.bind_in_place(h, tensors, grads)

    def _needs_init(self):
        """Training mode with ActNorm not initialised yet (the buffers are read once, then the answer is remembered on the host)."""
        if not self.training:
            return False
        if self._init_done is None:
            flags = [int(m.initialized.item()) for m in self.main if isinstance(m, ActNorm)]
            if len(set(flags)) > 1:
                raise native.I2VError("NLayerDiscriminator: some ActNorm layers are initialised and some are not; that state is not built")
            object.__setattr__(self, "_init_done", bool(flags[0]) if flags else True)
        return not self._init_done

    def _run(self, x, save, grads=None):
        if not x.is_cuda:
            raise native.I2VError("NLayerDiscriminator got a CPU tensor: its kernels run on a HIP device only (this package has no CPU fallback)")
        init = self._needs_init()
        with torch.no_grad():
            out = self._handle(grads).forward(x.detach().float().contiguous(), iterate=self.training and self.cfg["spectral_norm"], init_actnorm=init,
                                              save=save)
            if init:
                for m in self.main:
                    if isinstance(m, ActNorm):
                        m.initialized.fill_(1)
                object.__setattr__(self, "_init_done", True)
        return out

    def forward(self, input):
        """Standard forward."""
        params = list(self.parameters())
        if torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in params)):
            return _PatchDiscFunction.apply(self, input, *params)
        return self._run(input, save=False)
