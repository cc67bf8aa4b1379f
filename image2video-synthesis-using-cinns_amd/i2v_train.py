"""Training natively: ``FusedAdam`` (``torch.optim.Adam`` semantics in one multi-tensor HIP launch, ``i2v_adam_step``),
``FlowTrainer`` (forward, loss gradient, backward and optimiser step of the stage-2 trainer, reference
stage2_cINN/main.py:22-46, without autograd in between), ``PatchDiscTrainer`` (the spatial-discriminator lines of the stage-1
step, reference stage1_VAE/modules/loss.py:111-125), ``TemporalDiscTrainer`` (the temporal-discriminator lines 94-109 without the
gradient penalty, 127-135) and ``TemporalDiscPenaltyTrainer`` (lines 94-109 complete, ``w_GP`` included).  No CPU fallback: parameters and gradients live on a HIP device."""
import ctypes

import numpy as np
import torch

import i2v_native as native


def _adam_plan(rows, device):
    """rows: [(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq or None)] -> (device table of AdamTensor rows, chunk list)."""
    chunk = int(native.lib().i2v_adam_chunk())
    tab = np.zeros((len(rows), 6), dtype=np.int64)
    chunks = []
    for i, r in enumerate(rows):
        tab[i, :5] = [0 if t is None else t.data_ptr() for t in r]
        tab[i, 5] = r[0].numel()
        starts = np.arange(0, r[0].numel(), chunk, dtype=np.int32)
        chunks.append(np.stack([np.full_like(starts, i), starts], axis=1))
    assert ctypes.sizeof(native.AdamTensor) == 48
    table = torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(device)
    return table, torch.from_numpy(np.concatenate(chunks, axis=0)).to(device)


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` with the update of every tensor in ONE launch.  Same constructor arguments, same ``state_dict()``
    layout (``step``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``), so a checkpoint of one loads into the other and the
    ``torch.optim.lr_scheduler`` classes work on it.  Parameters without ``.grad`` are skipped like torch skips them."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"FusedAdam: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        # the key set of torch's own Adam (whatever this torch version keeps in a param_group), so state dicts interchange
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad).defaults)
        super().__init__(params, defaults)
        self._plans = {}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}

    def _rows(self, group):
        rows, steps = [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse or not p.is_cuda or p.dtype != torch.float32:
                raise native.I2VError("FusedAdam: dense float32 parameters on a HIP device only (this package has no CPU fallback)")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if group["amsgrad"] and "max_exp_avg_sq" not in st:
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            rows.append((p.data if p.is_contiguous() else None, g, st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq")))
            if rows[-1][0] is None:
                raise native.I2VError("FusedAdam: parameters must be contiguous")
            steps.append(st["step"])
        return rows, steps

    def _launch(self, gi, group, rows, steps, check=True):
        """One launch per distinct step count of the group (normally one)."""
        torch._foreach_add_(steps, 1)
        counts = [int(s) for s in steps] if check else [int(steps[0])] * len(steps)
        for count in sorted(set(counts)):
            sel = [r for r, c in zip(rows, counts) if c == count]
            key = (gi, count if len(set(counts)) > 1 else 0)
            ptrs = tuple(t.data_ptr() for r in sel for t in r[:2]) if check else None
            plan = self._plans.get(key)
            if plan is None or (check and plan[0] != ptrs):
                plan = (ptrs,) + _adam_plan(sel, sel[0][0].device) + (sel,)
                self._plans[key] = plan
            b1, b2 = group["betas"]
            native.adam_step(plan[1], plan[2], float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], group["amsgrad"], count)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if group.get("maximize") or group.get("decoupled_weight_decay"):
                raise native.I2VError("FusedAdam: maximize / decoupled_weight_decay are not implemented")
            rows, steps = self._rows(group)
            if rows:
                self._launch(gi, group, rows, steps)
        return loss


class FlowTrainer:
    """The stage-2 training step without autograd: ``step(z, cond_or_embed)`` runs forward (training handle), the FlowLoss
    gradient ``d_zt = zt / B``, ``d_logdet = -1 / B``, backward into one flat gradient buffer this object owns, and the fused
    Adam step -- all enqueued on the current stream, no host synchronisation.  ``network``: a ``SupervisedTransformer`` or a
    ``ConditionalFlow``.  ``.grad`` of every flow parameter is a view of the flat buffer; ``optimizer`` is a ``FusedAdam`` over
    them (``torch.optim.lr_scheduler`` works on it)."""

    def __init__(self, network, lr=1e-5, betas=(0.9, 0.99), weight_decay=0, amsgrad=True, eps=1e-8):
        self.network = network
        self.flow = getattr(network, "flow", network)
        self.optimizer = FusedAdam(self.flow.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        self._handle, self._bound, self._flat, self._rows, self._const = None, None, None, None, {}

    def _prepare(self):
        h = self.flow._train_native()
        if h is not self._handle or self._bound != h.bound_ptrs:
            self._handle, self._bound = h, h.bound_ptrs
            dev = self.flow.module_device()
            self._flat = torch.zeros(h.flat_numel, dtype=torch.float32, device=dev)
            for (name, shape), p in zip(self.flow._train_names, self.flow._train_params):
                off, n = h.flat_slices[name]
                p.grad = self._flat[off:off + n].view(shape)
            self._rows = self.optimizer._rows(self.optimizer.param_groups[0])
            self.optimizer._plans = {}
        return h

    def step(self, z, cond_or_embed):
        """One optimisation step on the batch; returns the four FlowLoss numbers as 0-d device tensors."""
        flow = self.flow
        with torch.no_grad():
            z2 = z.reshape(z.shape[0], -1).contiguous()
            if self.network is not flow:
                if isinstance(cond_or_embed, (list, tuple)):
                    e2 = self.network._embed(z2, cond_or_embed, None)
                elif self.network.control and cond_or_embed.shape[1] != flow.cond_channels:
                    raise native.I2VError("FlowTrainer.step: with control, pass cond = [x0, pos] or the full-width embedding")
                else:
                    e2 = cond_or_embed
            else:
                e2 = cond_or_embed
            e2 = e2.reshape(e2.shape[0], -1).contiguous()
            flow._check_init(z2, e2)
            h = self._prepare()
            flow._invalidate_inference()
            B = z2.shape[0]
            zt, logdet, saved = h.forward(z2, e2)
            d_ld = self._const.get(B)
            if d_ld is None:
                d_ld = self._const[B] = torch.full((B,), -1.0 / B, dtype=torch.float32, device=z2.device)
            h.backward(zt / B, d_ld, saved, self._flat, accumulate=False)
            rows, steps = self._rows
            self.optimizer._launch(0, self.optimizer.param_groups[0], rows, steps, check=False)
            nll_loss = 0.5 * zt.pow(2).sum(1).mean()
            nlogdet_loss = -logdet.mean()
            reference_nll_loss = 0.5 * torch.randn_like(zt).pow(2).sum(1).mean()
        return {"Loss": nll_loss + nlogdet_loss, "reference_nll_loss": reference_nll_loss, "nlogdet_loss": nlogdet_loss,
                "nll_loss": nll_loss}


class PatchDiscTrainer:
    """The spatial-discriminator part of the stage-1 step without autograd.  ``step(data_fake, data_real)`` is loss.py:112-118: two
    forwards (each with its own power iteration; the first one initialises ActNorm), the hinge loss, two backwards that accumulate
    into ``.grad``, and the fused Adam step.  ``generator_loss(data_fake)`` is loss.py:122-123: a third forward and the gradient of
    ``-mean(pred)`` at the frames, with no weight-gradient launch.  Everything is enqueued on the current stream; nothing
    synchronises.  Defaults: stage1_VAE/main.py:103 and the shipped configs."""

    def __init__(self, disc, lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5, eps=1e-8):
        self.disc = disc
        self.optimizer = FusedAdam(disc.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    def _grads(self):
        for p in self.disc.parameters():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        return {k: p.grad for k, p in self.disc.named_parameters()}

    @torch.no_grad()
    def step(self, data_fake, data_real):
        """-> (L_d_s, mean real logit, mean fake logit) as float64 0-d device tensors."""
        disc, grads = self.disc, self._grads()
        pred_f, saved_f = disc._run(data_fake, save=True, grads=grads)
        pred_r, saved_r = disc._run(data_real, save=True, grads=grads)
        out, d_f, d_r = native.patchdisc_hinge(pred_f, pred_r, "disc")
        h = disc._handle(grads)
        h.backward(d_f, saved_f, tuple(data_fake.shape), need_dx=False, param_grads=True, accumulate=False)
        h.backward(d_r, saved_r, tuple(data_real.shape), need_dx=False, param_grads=True, accumulate=True)
        self.optimizer.step()
        return out[0], out[1], out[2]

    @torch.no_grad()
    def generator_loss(self, data_fake):
        """-> (loss_gen_s as a float64 0-d device tensor, its gradient at ``data_fake`` [N, 3, H, W]); ``.grad`` is left untouched."""
        pred, saved = self.disc._run(data_fake, save=True)
        out, d_f, _ = native.patchdisc_hinge(pred, None, "gen")
        dx = self.disc._handle().backward(d_f, saved, tuple(data_fake.shape), need_dx=True, param_grads=False)   # (the gradient binding of step() stays)
        return out[0], dx


class TemporalDiscTrainer:
    """The temporal-discriminator part of the stage-1 step without autograd, on ``resnet3D.Discriminator``.  Clips are [B, T, 3, H, W] as
    the step holds them (or [B, 3, T, H, W]; the module transposes as the reference does).  Everything is enqueued on the current
    stream; no method synchronises the host.  Defaults: stage1_VAE/main.py and the shipped configs.

    ``w_GP != 0`` is refused here: this class has no double backward.  ``TemporalDiscPenaltyTrainer`` below is the step with the penalty
    (the penalty's gradient as a tangent forward and one reverse pass over the pair, csrc/i2v_res3d_gp.h).  ``gradient_penalty`` returns
    the penalty's VALUE, which is a first-order quantity."""

    def __init__(self, disc, lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5, w_GP=0, eps=1e-8, optimizer=None):
        """``optimizer``: an optimiser over ``disc.parameters()`` to step instead of the fused Adam (the tests step plain SGD)."""
        if w_GP:
            raise NotImplementedError(f"TemporalDiscTrainer: w_GP = {w_GP} needs the gradient of the gradient penalty, which this class does not "
                                      "form (it has no double backward of resnet3D.Discriminator; gradient_penalty() gives the penalty's value "
                                      "only): use i2v_train.TemporalDiscPenaltyTrainer, the same step with the penalty's gradient")
        self.disc = disc
        self.optimizer = optimizer or FusedAdam(disc.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._ones = {}

    def _grads(self):
        for p in self.disc.parameters():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        return {k: p.grad for k, p in self.disc.named_parameters()}

    @staticmethod
    def _shape(seq):
        n, a, b, h, w = seq.shape
        return (n, b, a, h, w) if a > b else (n, a, b, h, w)

    @torch.no_grad()
    def step(self, seq_fake, seq_real):
        """loss.py:98-109 without the penalty: two forwards (each with its own power iteration), the hinge loss, two backwards that
        accumulate into ``.grad``, the fused Adam step.  -> (L_d_t, mean real logit, mean fake logit) as float64 0-d device tensors."""
        disc, grads = self.disc, self._grads()
        pred_f, _, saved_f = disc._run(seq_fake, save=True, grads=grads, want_fmaps=False)
        pred_r, _, saved_r = disc._run(seq_real, save=True, grads=grads, want_fmaps=False)
        out, d_f, d_r = native.patchdisc_hinge(pred_f, pred_r, "disc")
        h = disc._handle(grads)
        h.backward(d_f, None, saved_f, self._shape(seq_fake), need_dx=False, param_grads=True, accumulate=False)
        h.backward(d_r, None, saved_r, self._shape(seq_real), need_dx=False, param_grads=True, accumulate=True)
        self.optimizer.step()
        return out[0], out[1], out[2]

    @torch.no_grad()
    def generator_loss(self, seq_fake, seq_real, w_coup_t=1, w_fmap_t=10):
        """loss.py:127-135: both forwards iterate the spectral norm, as the reference's do.  -> ((coup_t, L_fmap_t, L_temp) as float64 0-d
        device tensors, the gradient of L_temp at ``seq_fake`` [B, 3, T, H, W]); ``.grad`` is left untouched."""
        disc = self.disc
        pred_f, fmap_f, saved = disc._run(seq_fake, save=True)
        _, fmap_r, _ = disc._run(seq_real, save=False)
        hinge, d_pred, _ = native.patchdisc_hinge(pred_f, None, "gen")
        fm, d_fmaps = native.disc3d_fmap_loss(fmap_f, fmap_r, "L1", need_grads=True, grad_scale=float(w_fmap_t))
        if w_coup_t != 1:
            d_pred = d_pred * float(w_coup_t)
        dx = disc._handle().backward(d_pred, d_fmaps, saved, self._shape(seq_fake), need_dx=True, param_grads=False)
        return (hinge[0], fm[0], w_coup_t * hinge[0] + w_fmap_t * fm[0]), dx

    @torch.no_grad()
    def gradient_penalty(self, seq_real):
        """The value of ``gradient_penalty(pred, x)`` (loss.py:35-43): the mean over the samples of the squared norm of the gradient of
        ``mean(pred)`` at the clips, from one saved forward (it iterates in training mode, as a forward of the step does) and one
        input-gradient backward.  -> float64 0-d device tensor."""
        pred, _, saved = self.disc._run(seq_real, save=True, want_fmaps=False)
        n = pred.shape[0]
        d_pred = self._ones.get((n, pred.device))
        if d_pred is None:
            d_pred = self._ones[(n, pred.device)] = torch.full((n, 1), 1.0 / n, dtype=torch.float32, device=pred.device)
        dx = self.disc._handle().backward(d_pred, None, saved, self._shape(seq_real), need_dx=True, param_grads=False)
        return native.disc3d_sumsq(dx).mean()


class TemporalDiscPenaltyTrainer(TemporalDiscTrainer):
    """``TemporalDiscTrainer`` with the gradient penalty's gradient: ``step`` is loss.py:95-109 complete,
    ``(L_d_t + w_GP * L_GP).backward()`` and the optimiser step.  The penalty's gradient is no general double backward: a tangent forward
    along ``(2 w_GP / n) grad_x mean(pred)`` and one reverse pass over the pair (``NativeDisc3D.gp_backward``, csrc/i2v_res3d_gp.h), from
    the SAME saved forward on the real clips that the hinge loss uses, so each step iterates the spectral norm twice, as the reference's
    does.  ``generator_loss`` and ``gradient_penalty`` are inherited.  No method synchronises the host."""

    def __init__(self, disc, lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5, w_GP=10, eps=1e-8, optimizer=None):
        super().__init__(disc, lr=lr, betas=betas, weight_decay=weight_decay, w_GP=0, eps=eps, optimizer=optimizer)
        self.w_GP = float(w_GP)
        self._gp_saved = None

    @torch.no_grad()
    def step(self, seq_fake, seq_real):
        """-> (L_d_t, mean real logit, mean fake logit, L_GP) as float64 0-d device tensors; ``w_GP = 0`` runs the parent's step and
        returns ``L_GP = 0``."""
        if not self.w_GP:
            out = super().step(seq_fake, seq_real)
            return out[0], out[1], out[2], torch.zeros((), dtype=torch.float64, device=out[0].device)
        disc, grads = self.disc, self._grads()
        pred_f, _, saved_f = disc._run(seq_fake, save=True, grads=grads, want_fmaps=False)
        pred_r, _, saved_r = disc._run(seq_real, save=True, grads=grads, want_fmaps=False)
        out, d_f, d_r = native.patchdisc_hinge(pred_f, pred_r, "disc")
        h = disc._handle(grads)
        shape_r = self._shape(seq_real)
        # the real clips first, the penalty onto them, then the fake clips: the sum autograd forms for
        # (hinge_loss(pred_f, pred_r, 'disc') + w_GP * L_GP).backward() over forward() and forward_with_penalty(), bit for bit
        h.backward(d_r, None, saved_r, shape_r, need_dx=False, param_grads=True, accumulate=False)
        need = h.gp_saved_bytes(shape_r[0], *shape_r[2:])
        if self._gp_saved is None or self._gp_saved.numel() < need or self._gp_saved.device != saved_r.device:
            self._gp_saved = torch.empty(need, dtype=torch.uint8, device=saved_r.device)
        l_gp, _ = h.gp_backward(saved_r, shape_r, scale=self.w_GP, accumulate=True, gp_saved=self._gp_saved)
        h.backward(d_f, None, saved_f, self._shape(seq_fake), need_dx=False, param_grads=True, accumulate=True)
        self.optimizer.step()
        return out[0], out[1], out[2], l_gp
