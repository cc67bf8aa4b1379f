"""Mirror of the reference's ``stage2_cINN/modules/loss.py``: the negative log-likelihood of the flow under a standard normal
prior.  Plain torch ops on ``[B, 64]`` tensors: the loss is not a hot path (its gradient, ``d_zt = zt / B`` and
``d_logdet = -1 / B``, enters the HIP backward of csrc/i2v_flow_train.hip through autograd)."""
import torch
import torch.nn as nn

try:  # optional: logged to only when it is installed
    import wandb
except ImportError:
    wandb = None


def nll(sample):
    """0.5 * ||sample||^2 per batch entry of a [B, C, H, W] tensor (loss.py:28-29)."""
    return 0.5 * sample.pow(2).sum(dim=[1, 2, 3])


class LossLogger:
    """Smallest logger ``FlowLoss`` can write to: ``reset()`` and ``append(dict)``; ``mean(key)`` over what was appended."""

    def __init__(self):
        self.entries = []

    def reset(self):
        self.entries = []

    def append(self, dic):
        self.entries.append(dict(dic))

    def mean(self, key):
        return sum(e[key] for e in self.entries) / max(1, len(self.entries))


class FlowLoss(nn.Module):
    """loss = mean(nll(sample)) - mean(logdet) (loss.py:9-26).  ``logger.append`` receives the keys ``Loss``,
    ``reference_nll_loss``, ``nlogdet_loss``, ``nll_loss`` as Python floats; ``reference_nll_loss`` is the nll of a fresh
    ``randn_like(sample)`` draw, which consumes the RNG stream exactly like the reference does (seeded runs line up)."""

    def forward(self, sample, logdet, logger, mode="eval"):
        assert len(logdet.shape) == 1
        nll_loss = nll(sample).mean()
        nlogdet_loss = -logdet.mean()
        loss = nll_loss + nlogdet_loss
        reference_nll_loss = nll(torch.randn_like(sample)).mean()
        loss_dic = {"Loss": loss.item(), "reference_nll_loss": reference_nll_loss.item(),
                    "nlogdet_loss": nlogdet_loss.item(), "nll_loss": nll_loss.item()}
        logger.append(loss_dic)
        if wandb is not None and getattr(wandb, "run", None) is not None:
            wandb.log({f"{mode}_{k}": v for k, v in loss_dic.items()})
        return loss
