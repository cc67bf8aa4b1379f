"""Mirror of the reference's ``stage1_VAE/modules/decoder.py`` class surface (GeneratorBlock, Generator).

``Generator.forward(img, motion)`` is ONE call into libi2v_hip.so (``i2v_dec_forward``, csrc/i2v_dec.hip): all
activations stay channels-last in HBM, spectral-norm is folded at load time, the 3x3x3 convolutions run on the
gfx950 matrix cores.  The sub-modules carry the reference's state_dict keys (``g_k.conv_0.weight_orig`` ...) so
released ``.pth`` files load unchanged."""
import torch
import torch.nn as nn

import i2v_native as native
from i2v_params import ConvParams, LinearParams, NativeBacked
from stage1_VAE.modules.normalization_layer import ADAIN, Norm3D, Spade


class _GBlockTrainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, cond1, cond2, *params):
        out, saved = module._train_handle().forward(x, cond1, cond2, train=module.training, save=True)
        ctx.module, ctx.saved, ctx.z, ctx.shape, ctx.img_shape = module, saved, cond1, tuple(x.shape), tuple(cond2.shape)
        return out

    @staticmethod
    def backward(ctx, g_out):
        if torch.is_grad_enabled():   # create_graph=True: a graph through this backward is asked for
            raise NotImplementedError("GeneratorBlock is once differentiable: the double backward (create_graph=True) is not built")
        module = ctx.module
        want = ctx.needs_input_grad[4:]
        grads = native.flat_param_grads(module, ctx.saved.device) if any(want) else None
        h = module._train_handle(grads)
        need_dx, need_dz = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx, dz = h.backward(g_out.contiguous().float(), ctx.z, ctx.saved, ctx.shape, ctx.img_shape, need_dx=need_dx or (grads is None and not need_dz),
                            need_dz=need_dz, param_grads=grads is not None, accumulate=False)
        out = [None] * len(want) if grads is None else [g if w else None for g, w in zip(grads.values(), want)]
        return (None, dx if need_dx else None, dz, None, *out)


class GeneratorBlock(NativeBacked):
    """out = shortcut(x) + conv_1(lrelu(ADAIN(conv_0(lrelu(Spade(x, img))), z)))   (reference decoder.py:7-52).

    ``differentiable`` (a plain attribute, default False; not a reference argument): while it is False every call runs the packed inference
    handle (csrc/i2v_gblock.hip), in grad mode too.  With ``differentiable = True`` every forward runs on the training handle
    (csrc/i2v_gblock_train.hip, exact fp32), which reads the parameters in place and, in ``.train()`` mode, iterates ``weight_u`` /
    ``weight_v`` in place as torch's spectral norm does; in grad mode it returns a tensor with a ``grad_fn`` from a Function whose inputs
    are ``x``, ``cond1`` and the parameters.  A frozen module skips the weight-gradient launches; ``create_graph=True`` raises, and so does
    a ``cond2`` that requires grad (no gradient is formed at the start frame).  Setting it back to False rebuilds the packed handle from
    the current parameters."""

    def __init__(self, n_in, n_out, use_spectral, z_dim, mma=None):
        super().__init__()
        self.mma = mma   # not a reference argument: the native block's matrix-core mode (None: I2V_DEC_MMA / default; 0, 1 or "fp16")
        self.learned_shortcut = (n_in != n_out)
        n_middle = min(n_in, n_out)
        self.n_in, self.n_out, self.z_dim, self.use_spectral = n_in, n_out, z_dim, bool(use_spectral)
        self.conv_0 = ConvParams(n_in, n_middle, 3, 3, bias=True, spectral=use_spectral)
        self.conv_1 = ConvParams(n_middle, n_out, 3, 3, bias=True, spectral=use_spectral)
        if self.learned_shortcut:
            self.conv_s = ConvParams(n_in, n_out, 1, 3, bias=False, spectral=use_spectral)
        self.norm_0 = Spade(n_in)
        self.norm_1 = ADAIN(n_middle, z_dim)
        if self.learned_shortcut:
            self.norm_s = Norm3D(n_in)
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

    def _build_native(self):
        h = native.NativeGBlock(self.n_in, self.n_out, self.z_dim, self.use_spectral, mma=self.mma, device=self.module_device())
        h.load(self.state_dict())
        return h

    def _train_handle(self, grads=None):
        """The training handle, bound to the storage of the parameters and spectral-norm buffers as it is now and, when ``grads``
        ({parameter name: tensor}) is given, to those gradient tensors."""
        tensors = {k: t for k, t in list(self.named_parameters()) + list(self.named_buffers()) if t.dtype == torch.float32}
        for t in tensors.values():
            if not t.is_cuda:
                raise native.I2VError("GeneratorBlock runs on a HIP device only: move the module to 'cuda' (this package has no CPU fallback)")
        h = self.__dict__.get("_train_native")
        dev = next(iter(tensors.values())).device
        if h is None or h.device != dev:
            h = native.NativeGBlockTrain(self.n_in, self.n_out, self.z_dim, self.use_spectral, device=dev)
            object.__setattr__(self, "_train_native", h)
        return native.bind_in_place(h, tensors, grads)

    def forward(self, x, cond1, cond2):
        if not self.differentiable:
            return self.native().forward(x.contiguous(), cond1.contiguous(), cond2.contiguous())
        if not (x.is_cuda and cond1.is_cuda and cond2.is_cuda):
            raise native.I2VError("GeneratorBlock got a CPU tensor: its kernels run on a HIP device only (this package has no CPU fallback)")
        params = list(self.parameters())
        if torch.is_grad_enabled():
            if cond2.requires_grad:
                raise NotImplementedError("GeneratorBlock forms no gradient at the start frame (cond2): the reference never asks for one")
            if x.requires_grad or cond1.requires_grad or any(p.requires_grad for p in params):
                return _GBlockTrainFunction.apply(self, x.float().contiguous(), cond1.float().contiguous(), cond2.detach().float().contiguous(), *params)
        with torch.no_grad():
            return self._train_handle().forward(x.detach().float().contiguous(), cond1.detach().float().contiguous(),
                                                cond2.detach().float().contiguous(), train=self.training)[0]


def _once_differentiable(what):
    if torch.is_grad_enabled():   # create_graph=True: a graph through this backward is asked for
        raise NotImplementedError(f"{what} is once differentiable: the double backward (create_graph=True) is not built")


class _GenFcFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, z, weight, bias):
        ctx.module, ctx.z = module, z
        return module._train_handle().fc_forward(z)

    @staticmethod
    def backward(ctx, g_out):
        _once_differentiable("Generator")
        need_dz, want = ctx.needs_input_grad[1], ctx.needs_input_grad[2:]
        if not (need_dz or any(want)):
            return None, None, None, None
        grads = ctx.module._glue_grads(g_out.device) if any(want) else None
        dz = ctx.module._train_handle(grads).fc_backward(g_out.contiguous().float(), ctx.z, need_dz=need_dz, param_grads=grads is not None)
        return None, dz, grads["fc.weight"] if want[0] else None, grads["fc.bias"] if want[1] else None


class _UpsampleFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ut, us):
        ctx.factors = (ut, us)
        return native.gen_train_upsample(x, ut, us)

    @staticmethod
    def backward(ctx, g_out):
        _once_differentiable("Generator")
        return native.gen_train_upsample_backward(g_out.contiguous().float(), *ctx.factors), None, None


class _GenHeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, weight, bias):
        out, saved = module._train_handle().head_forward(x, save=True)
        ctx.module, ctx.saved, ctx.shape = module, saved, tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g_out):
        _once_differentiable("Generator")
        need_dx, want = ctx.needs_input_grad[1], ctx.needs_input_grad[2:]
        if not (need_dx or any(want)):
            return None, None, None, None
        grads = ctx.module._glue_grads(g_out.device) if any(want) else None
        dx = ctx.module._train_handle(grads).head_backward(g_out.contiguous().float(), ctx.saved, ctx.shape, need_dx=need_dx,
                                                           param_grads=grads is not None)
        return None, dx, grads["conv_img.weight"] if want[0] else None, grads["conv_img.bias"] if want[1] else None


class Generator(NativeBacked):
    """fc -> head_0 -> (x2, g_0) -> (x2, g_1) -> (x2, g_2) -> (up, g_3) -> (up, g_4) -> lrelu -> conv_img -> tanh
    (reference decoder.py:55-120).  Returns ``[B, 16, 3, H, W]`` (contiguous; the reference returns a transposed
    view of a [B,3,16,H,W] buffer).

    ``differentiable`` (a plain attribute, default False; not a reference argument): while it is False every call is the packed inference
    handle, in grad mode too.  Setting it True sets every block's ``differentiable`` and ``forward(img, motion)`` then runs the chain in
    exact fp32 with the parameters read in place: the ``fc`` Function, ``head_0``, five (up-sampling Function, block) pairs and the image
    head Function (csrc/i2v_gen_train.hip around the six block Functions of csrc/i2v_gblock_train.hip).  In grad mode the frames carry a
    ``grad_fn``; ``motion.grad`` is the sum of fc's and the six blocks' contributions; no gradient is formed at ``img``.  ``.train()``
    iterates every block's ``weight_u`` / ``weight_v`` once per forward.  ``out=``, ``realizations != 1`` and ``prepare()`` are the inference
    handle's and raise here.  Setting it back to False resets the blocks and rebuilds the packed decoder from the current parameters."""

    def __init__(self, dic):
        super().__init__()
        nf = dic["channel_factor"]
        self.z_dim = dic["z_dim"]
        self.fmap_start = 16 * nf
        use_spectral = dic["spectral_norm"]
        self.upsample_s = list(dic["upsample_s"])
        self.upsample_t = list(dic["upsample_t"])
        self.channel_factor = nf
        self.use_spectral = bool(use_spectral)
        self.fc = LinearParams(self.z_dim, 4 * 4 * 16 * nf)
        self.head_0 = GeneratorBlock(16 * nf, 16 * nf, use_spectral, self.z_dim)
        self.g_0 = GeneratorBlock(16 * nf, 16 * nf, use_spectral, self.z_dim)
        self.g_1 = GeneratorBlock(16 * nf, 8 * nf, use_spectral, self.z_dim)
        self.g_2 = GeneratorBlock(8 * nf, 4 * nf, use_spectral, self.z_dim)
        self.g_3 = GeneratorBlock(4 * nf, 2 * nf, use_spectral, self.z_dim)
        self.g_4 = GeneratorBlock(2 * nf, 1 * nf, use_spectral, self.z_dim)
        self.conv_img = ConvParams(nf, 3, 3, 3, bias=True, spectral=False)
        # matrix-core mode of the 3x3x3 convolutions: 0 = exact fp32 MFMA, 1 = split-fp16 (3 fp16 MFMAs per product,
        # fp32-class accuracy, ~5x the rate).  Not a reference key: taken from dic["mma"] or the I2V_DEC_MMA env var.
        mma = dic.get("mma", None) if hasattr(dic, "get") else None
        self.mma = native.default_mma() if mma is None else native.parse_mma(mma)   # 0, 1, 2 or "auto" (= 2)
        object.__setattr__(self, "_train_native", None)
        object.__setattr__(self, "_differentiable", False)

    def _blocks(self):
        return (self.head_0, self.g_0, self.g_1, self.g_2, self.g_3, self.g_4)

    @property
    def differentiable(self):
        return self.__dict__.get("_differentiable", False)

    @differentiable.setter
    def differentiable(self, value):
        value = bool(value)
        was = self.differentiable
        object.__setattr__(self, "_differentiable", value)
        for blk in self._blocks():
            blk.differentiable = value
        if was and not value:
            self.refresh_native()

    def _drop_native(self):
        super()._drop_native()
        object.__setattr__(self, "_train_native", None)

    def __getstate__(self):
        state = dict(super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__)
        state["_native"] = state["_train_native"] = None
        return state

    _GLUE_KEYS = ("fc.weight", "fc.bias", "conv_img.weight", "conv_img.bias")

    def _glue_params(self):
        return {"fc.weight": self.fc.weight, "fc.bias": self.fc.bias, "conv_img.weight": self.conv_img.weight, "conv_img.bias": self.conv_img.bias}

    def _glue_grads(self, device):
        """{key: gradient tensor} of fc and conv_img: views of one flat fp32 allocation, each starting on a multiple of 4 floats."""
        params = self._glue_params()
        sizes = [(p.numel() + 3) // 4 * 4 for p in params.values()]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=device)
        return {k: v[:p.numel()].view(p.shape) for (k, p), v in zip(params.items(), flat.split(sizes))}

    def _train_handle(self, grads=None):
        """The training handle of fc and the image head, bound to the storage of their parameters as it is now and, when ``grads`` is
        given, to those gradient tensors."""
        tensors = self._glue_params()
        for t in tensors.values():
            if not t.is_cuda:
                raise native.I2VError("Generator runs on a HIP device only: move the module to 'cuda' (this package has no CPU fallback)")
        h = self.__dict__.get("_train_native")
        dev = tensors["fc.weight"].device
        if h is None or h.device != dev:
            h = native.NativeGenTrain(self.channel_factor, self.z_dim, device=dev)
            object.__setattr__(self, "_train_native", h)
        return native.bind_in_place(h, tensors, grads)

    def _forward_differentiable(self, img, motion):
        if not (img.is_cuda and motion.is_cuda):
            raise native.I2VError("Generator got a CPU tensor: its kernels run on a HIP device only (this package has no CPU fallback)")
        if motion.dim() != 2 or motion.shape[1] != self.z_dim or img.dim() != 4 or img.shape[0] != motion.shape[0] or img.shape[1] != 3:
            raise native.I2VError(f"Generator: expected img [B,3,h,w] and motion [B,{self.z_dim}], got {tuple(img.shape)}, {tuple(motion.shape)}")
        grad = torch.is_grad_enabled()
        if grad and img.requires_grad:
            raise NotImplementedError("Generator forms no gradient at the start frame (img): the reference never asks for one")
        img, z = img.detach().float().contiguous(), motion.float().contiguous()
        B, up = z.shape[0], native.gen_train_upsample
        factors = [(2, 2), (2, 2), (2, 2)] + [(int(t), int(s)) for t, s in zip(self.upsample_t, self.upsample_s)]
        fc = (self.fc.weight, self.fc.bias)
        if grad and (z.requires_grad or any(p.requires_grad for p in fc)):
            x = _GenFcFunction.apply(self, z, *fc)
        else:
            with torch.no_grad():
                x = self._train_handle().fc_forward(z.detach())
        x = self.head_0(x.view(B, 16 * self.channel_factor, 1, 4, 4), z, img)
        for blk, (ut, us) in zip(self._blocks()[1:], factors):
            if (ut, us) != (1, 1):
                x = _UpsampleFunction.apply(x, ut, us) if grad and x.requires_grad else up(x.detach(), ut, us)
            x = blk(x, z, img)
        head = (self.conv_img.weight, self.conv_img.bias)
        if grad and (x.requires_grad or any(p.requires_grad for p in head)):
            return _GenHeadFunction.apply(self, x.contiguous(), *head)
        with torch.no_grad():
            return self._train_handle().head_forward(x.detach().contiguous())[0]

    def _build_native(self):
        h = native.NativeDecoder(self.channel_factor, self.z_dim, self.upsample_s, self.upsample_t, self.use_spectral,
                                 mma=self.mma, device=self.module_device())
        h.load(self.state_dict())
        if getattr(self, "_shared_side", None) is not None and self._shared_side.device == h.device:
            h.set_side_stream(self._shared_side)
        return h

    def forward(self, img, motion, out=None, realizations=1):
        """decoder.py:97-120.  ``out`` (not a reference argument): a float32 view [B,16,3,H,W] with contiguous sample blocks to
        decode into; ``img`` may be a sample-strided view such as ``seq[:, -1]`` -- together they let the autoregressive loop of
        ``Model.forward`` (get_model.py:68-73) run without ``torch.cat`` / ``.contiguous()`` copies.
        ``realizations`` (not a reference argument) = K: ``img`` holds F start frames and ``motion`` F*K latents; sample f*K + k is
        realization k of frame f.  Same bits as ``forward(img.repeat_interleave(K, 0), motion)``; the SPADE branches run once per frame."""
        if self.differentiable:
            if out is not None or realizations != 1:
                raise NotImplementedError("Generator.differentiable is True: out= and realizations != 1 belong to the inference handle "
                                          "(set differentiable = False)")
            return self._forward_differentiable(img, motion)
        K = native.check_realizations(img, motion, self.z_dim, realizations)
        if K == 1:
            return self.native().forward(img, motion, out=out)
        return self.native().forward(img, motion, out=out, realizations=K)

    def decode_sequence(self, x_0, z, vid_length, realizations=1):
        """get_model.py:68-73 -- ``seq = G(x_0, z); while T < vid_length: seq = cat(seq, G(seq[:, -1], z))`` -- into ONE
        pre-allocated [B, 16*ceil(vid_length/16), 3, H, W] buffer: pass k writes frames [16k, 16k+16) in place and pass k+1 reads
        its start frames from the strided view seq[:, 16k+15] (i2v_dec_forward_strided).  Same kernels, same bits as the loop.
        ``realizations`` = K: ``x_0`` holds F start frames, ``z`` F*K latents; pass 0 shares each frame's SPADE branches between its K
        samples, the later passes start from each sample's own last frame (F*K distinct frames, the strided path)."""
        K = native.check_realizations(x_0, z, self.z_dim, realizations)
        T, H, W = self.native().out_shape
        n = max(1, -(-int(vid_length) // T))
        if K > 1:
            if n == 1:
                return self.forward(x_0, z, realizations=K)
            seq = torch.empty(x_0.shape[0] * K, n * T, 3, H, W, dtype=torch.float32, device=x_0.device)
            self.forward(x_0, z, out=seq[:, :T], realizations=K)
            for k in range(1, n):
                self.forward(seq[:, k * T - 1], z, out=seq[:, k * T:(k + 1) * T])
            return seq
        if n == 1:
            return self.forward(x_0, z)
        seq = torch.empty(x_0.shape[0], n * T, 3, H, W, dtype=torch.float32, device=x_0.device)
        self.forward(x_0, z, out=seq[:, :T])
        for k in range(1, n):
            self.forward(seq[:, k * T - 1], z, out=seq[:, k * T:(k + 1) * T])
        return seq

    def share_side_stream(self, stream):
        """Not a reference method: run the decoder's side work (SPADE branches, learned shortcuts, ``prepare``) on ``stream`` -- the
        stream the caller's cINN prefetch runs on (``i2v_pipeline.LatentPrefetcher.stream``) -- instead of a stream the native handle
        creates: one side stream per job (``None``: the handle's own again).  Survives a rebuild of the native handle."""
        object.__setattr__(self, "_shared_side", stream)
        self.native().set_side_stream(stream)

    def prepare(self, img, realizations=1):
        """Not a reference method: enqueue the SPADE branches of all blocks for the start frames ``img`` (they do not depend on
        the motion latent) on the native handle's side stream, behind what is already on the current stream.  The next
        ``forward(img, z)`` with the SAME contiguous tensor waits for them level by level instead of computing them
        (i2v_dec_prepare); ``get_model.Model.synthesize`` uses it to fill the time the cINN pass takes.  ``realizations`` = K: for
        ``forward(img, z, realizations=K)`` (the branches of the F frames, once each)."""
        if self.differentiable:
            raise NotImplementedError("Generator.differentiable is True: prepare() belongs to the inference handle (set differentiable = False)")
        K = native.check_realizations(None, None, None, realizations)
        if K == 1:
            self.native().prepare(img.contiguous())
        else:
            self.native().prepare(img.contiguous(), realizations=K)
