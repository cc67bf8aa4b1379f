"""Stage-1 losses and validation metrics, mirror of the reference's ``stage1_VAE/modules/loss.py``: ``KL``, ``fmap_loss``, ``hinge_loss`` and
``gradient_penalty`` and ``Backward`` with the reference's ``eval`` (loss.py:183-216).  The training step ``Backward.forward`` is not built:
every backward pass it needs exists (the Generator, the motion encoder through ``resnet3D.Encoder.differentiable``, ``KL`` and LPIPS with
gradients, both discriminators, and the gradient penalty's gradient without a general double backward), so only its composition remains, the
one open piece of stage-1 training.  Its spatial-discriminator lines (loss.py:111-125) are ``i2v_train.PatchDiscTrainer`` on
``patch_disc.NLayerDiscriminator``, its temporal-discriminator lines ``i2v_train.TemporalDiscTrainer`` (loss.py:94-109 without the penalty,
127-135) and ``i2v_train.TemporalDiscPenaltyTrainer`` (94-109 complete, ``w_GP`` included) on ``resnet3D.Discriminator``.
``fmap_loss`` and ``hinge_loss`` here are the reference's functions on torch tensors (they differentiate through the discriminators'
autograd Functions); the trainers use the kernel forms ``i2v_native.disc3d_fmap_loss`` and ``i2v_native.patchdisc_hinge``.

The reference takes ``psnr`` and ``ssim`` from ``pytorch_lightning.metrics.functional`` (1.2.7).  Here they are two kernel entries of
csrc/i2v_recon.hip over frames that stay on the device: one range pass and one pass that forms the L1 error, the MSE and the SSIM map in
float64 (DESIGN §12.4 states the formulas; the row is pinned to them, not to the library).  Argument order as the library's and as the
reference calls them, ``psnr(seq_orig, seq_gen)``: ``pred`` is the real clip and ``target`` the generated one -- with ``data_range=None``
only ``target`` sets the range of the PSNR (the 1.2.x rule, kept).

Differences of ``Backward`` from the reference, all of the surface and none of the numbers: no ``wandb.log``; the two returned sequences
stay on the device; ``lpips`` is an ``LPIPS`` instance the caller builds from files (``LPIPS(vgg_path=..., lin_path=...)``: nothing is
downloaded), and with ``lpips=None`` the key ``LPIPS`` is left out; the five values reach the host in ONE copy."""
import math

import torch
import torch.nn as nn

import i2v_native


class _KLFunction(torch.autograd.Function):
    """``i2v_kl_normal`` with the kernel gradient ``i2v_enc3d_kl_backward``: mu / n and (e^logvar - 1) / (2 n), fp32 [B, z]."""

    @staticmethod
    def forward(ctx, mu, logvar):
        ctx.save_for_backward(mu, logvar)
        return i2v_native.kl_normal(mu, logvar)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        d_mu, d_lv = i2v_native.enc3d_kl_backward(mu, logvar, 1.0)
        g = g.to(torch.float32)
        return (d_mu * g if ctx.needs_input_grad[0] else None), (d_lv * g if ctx.needs_input_grad[1] else None)


def KL(mu, logvar):
    """KL divergence between N(mu, exp(logvar)) and the unit Gaussian (loss.py:10-12).  On a HIP device: ``i2v_kl_normal`` (one
    workgroup, float64, fixed order) -> float64 0-d device tensor.  CPU tensors are refused (no CPU fallback).  In grad mode, with an
    argument that requires grad, the same value carries a ``grad_fn`` (the kernel gradient of ``i2v_enc3d_kl_backward``)."""
    mu, logvar = mu.reshape(mu.size(0), -1), logvar.reshape(logvar.size(0), -1)
    mu, logvar = mu.float().contiguous(), logvar.float().contiguous()
    if torch.is_grad_enabled() and (mu.requires_grad or logvar.requires_grad):
        return _KLFunction.apply(mu, logvar)
    return i2v_native.kl_normal(mu, logvar)


def fmap_loss(fmap1, fmap2, metric):
    """Feature-map loss over two lists of discriminator maps (loss.py:14-21)."""
    recp_loss = 0
    for a, b in zip(fmap1, fmap2):
        recp_loss = recp_loss + (torch.mean(torch.abs(a - b)) if metric == "L1" else torch.mean((a - b) ** 2) if metric == "L2" else 0)
    return recp_loss / len(fmap1)


def hinge_loss(fake_data, orig_data, update):
    """Hinge loss for the discriminator (``update='disc'``) or the generator (``'gen'``) (loss.py:24-32)."""
    if update == "disc":
        return (torch.mean(torch.relu(1.0 - orig_data)) + torch.mean(torch.relu(1.0 + fake_data))) / 2
    elif update == "gen":
        return -torch.mean(fake_data)


def gradient_penalty(disc, x):
    """The reference's ``gradient_penalty(pred, x)`` (loss.py:35-43): the mean over the samples of the squared norm of the gradient of
    ``mean(pred)`` at ``x``.  -> ``(pred, fmaps, L_GP)`` of ``disc.forward_with_penalty(x)``.

    The signature differs from the reference's ``(pred, x)``: there ``pred`` carries an autograd graph from which
    ``torch.autograd.grad(..., create_graph=True)`` builds the double backward.  Here the network is one autograd Function over HIP kernels
    with no graph inside to differentiate twice, so the penalty has to come out of the SAME forward call that makes ``pred`` -- the module
    and the clips go in, and ``pred`` comes out next to ``L_GP``.  In grad mode ``L_GP`` carries a ``grad_fn`` whose backward is the tangent
    forward and the reverse pass over the pair (csrc/i2v_res3d_gp.h); loss.py:98-108 is then
    ``pred_r, _, L_GP = gradient_penalty(disc_t, seq_real); (hinge_loss(pred_f, pred_r, 'disc') + w_GP * L_GP).backward()``."""
    return disc.forward_with_penalty(x)


def recon_metrics(pred, target, data_range=None, per_image=False):
    """PSNR, SSIM, L1 and MSE of two frame tensors [B, T, C, H, W] (or [N, C, H, W]) on a HIP device -> dict of float64 0-d device tensors
    ``l1, mse, psnr, ssim``; nothing synchronises.  ``data_range=None`` is the reference's behaviour (ranges taken from the data: PSNR from
    ``target`` alone, SSIM from the wider of the two); ``data_range=2.0`` is the fixed-range form for frames in [-1, 1].
    ``per_image=True`` adds ``psnr_per_image`` and ``ssim_per_image`` [B, T] (the per-frame curves of the prediction literature; the
    per-image PSNR uses the same R).  A strided view such as ``seq[:, 1:]`` is read in place."""
    scalars, rows, rng = i2v_native.recon_stats(pred, target, data_range)
    out = {"l1": scalars[0], "mse": scalars[1], "psnr": scalars[2], "ssim": scalars[3]}
    if per_image:
        lead = tuple(pred.shape[:2]) if pred.dim() == 5 else (pred.shape[0],)
        c, h, w = pred.shape[-3:]
        r = torch.full((), float(data_range), dtype=torch.float64, device=rows.device) if data_range is not None else rng[3] - rng[2]
        out["psnr_per_image"] = ((2 * torch.log(r) - torch.log(rows[:, 1] / (c * h * w))) * (10.0 / math.log(10.0))).view(lead)
        out["ssim_per_image"] = (rows[:, 2] / (c * (h - 10) * (w - 10))).view(lead)
    return out


def psnr(pred, target, data_range=None):
    """``pytorch_lightning.metrics.functional.psnr(pred, target, data_range)`` at its defaults (base 10, mean over all elements)."""
    return recon_metrics(pred, target, data_range)["psnr"]


def ssim(pred, target, data_range=None):
    """``pytorch_lightning.metrics.functional.ssim(pred, target, data_range=data_range)`` at its defaults (11 x 11 window, sigma 1.5,
    k1 = 0.01, k2 = 0.03, mean)."""
    return recon_metrics(pred, target, data_range)["ssim"]


def _section(opt, name):
    sec = None if opt is None else (opt.get(name) if isinstance(opt, dict) else getattr(opt, name, None))
    return sec if sec is not None else {}


class Backward(nn.Module):
    """Losses of stage 1 (loss.py:47-216).  ``eval`` is built; of ``forward`` (the training step) only the composition is missing."""

    def __init__(self, opt, lpips=None):
        super().__init__()
        self.dic = opt
        training, data = _section(opt, "Training"), _section(opt, "Data")
        for attr, key in (("w_kl", "w_kl"), ("gan_loss", "GAN_Loss"), ("w_coup_t", "w_coup_t"), ("w_fmap_t", "w_fmap_t"), ("w_coup_s", "w_coup_s"),
                          ("subsample_length", "subsample_length"), ("w_mse", "w_recon"), ("w_GP", "w_GP"), ("w_percep", "w_percep"),
                          ("pretrain", "pretrain")):
            setattr(self, attr, training.get(key))
        self.seq_length = data.get("sequence_length")
        self.lpips = lpips            # the reference builds LPIPS().cuda() here, which downloads its weights
        self.data_range = None        # None: the reference's data-dependent ranges
        self.per_image = False        # True: eval() also appends the [B, T] PSNR / SSIM curves (device tensors) to self.curves
        self.curves = []

    def forward(self, decoder, encoder, disc_t, disc_s, seq_o, optimizers, epoch, logger):
        raise NotImplementedError("Backward.forward (the stage-1 training step, loss.py:64-180) is not built: only its composition remains.  "
                                  "All of the backward passes it needs are built: the Generator (the decoder), the two discriminators "
                                  "(patch_disc.NLayerDiscriminator with i2v_train.PatchDiscTrainer: loss.py:111-125; resnet3D.Discriminator with "
                                  "i2v_train.TemporalDiscTrainer / TemporalDiscPenaltyTrainer: loss.py:94-109, 127-135), the gradient penalty's "
                                  "gradient (w_GP; a tangent forward and one reverse pass, no general double backward: "
                                  "Discriminator.forward_with_penalty, loss.gradient_penalty), the LPIPS gradient, and the motion-encoder "
                                  "backward with the KL gradient (resnet3D.Encoder.differentiable = True; KL returns a grad_fn); "
                                  "Backward.eval is built")

    @torch.no_grad()
    def eval(self, decoder, encoder, seq_o, logger):
        """loss.py:183-216: encode ``seq_o[:, 1:]``, decode from ``seq_o[:, 0]``, log Loss_L1, LPIPS, L_KL, PSNR, SSIM of the reconstruction.
        Returns ``[seq_gen, seq_orig]`` on the device."""
        seq_orig = seq_o[:, 1:]
        motion, mu, covar = encoder(seq_orig.transpose(1, 2))
        seq_gen = decoder(seq_o[:, 0], motion)

        m = recon_metrics(seq_orig, seq_gen, self.data_range, per_image=self.per_image)   # psnr(seq_orig, seq_gen), ssim(seq_orig, seq_gen)
        values = {"Loss_L1": m["l1"]}
        if self.lpips is not None:
            values["LPIPS"] = self.lpips(seq_orig.reshape(-1, *seq_orig.shape[2:]), seq_gen.reshape(-1, *seq_gen.shape[2:])).mean().double()
        values.update({"L_KL": KL(mu, covar), "PSNR": m["psnr"], "SSIM": m["ssim"]})
        if self.per_image:
            self.curves.append((m["psnr_per_image"], m["ssim_per_image"]))

        host = torch.stack(list(values.values())).cpu().tolist()   # the one device-to-host copy
        loss_dic = dict(zip(values, host))
        logger.append(loss_dic)
        return [seq_gen.detach(), seq_orig]
