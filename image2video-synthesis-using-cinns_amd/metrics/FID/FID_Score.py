"""FID on the device: own implementation of the reference's ``metrics/FID/FID_Score.py`` surface (pytorch-fid's ``fid_score.py``).

The reference keeps a ``[n, 2048]`` float64 array on the host and calls ``scipy.linalg.sqrtm``.  Here images and features stay on the
device until the set is done, the features come from the native Inception trunk (``metrics.FID.inception.InceptionV3``) and the Frechet distance is the float64 ``eigh``
formulation of ``metrics/PyTorch_FVD/FVD_logging.py`` (imported, not copied; no scipy, no imageio).

Two quirks of the reference are KEPT in ``get_activations`` and documented: ``n // batch_size`` batches are run and the ragged rest is
silently dropped, and a ``batch_size`` above ``n`` is clipped to ``n``.  ``FIDAccumulator`` is the streaming form; it uses EVERY image it
is given, so for a set size that is no multiple of the batch its value differs from ``calculate_FID``'s."""
import numpy as np
import torch

import i2v_native
from metrics.PyTorch_FVD.FVD_logging import StatsAccumulator, calculate_frechet_distance  # noqa: F401  (the eigh formulation)


def _pooled(pred):
    """[B, C, H, W] -> [B, C]: the model's block, globally averaged when it is not 1 x 1 (``dims`` other than 2048)."""
    if pred.shape[2] == 1 and pred.shape[3] == 1:
        return pred.reshape(pred.shape[0], -1)
    if pred.is_cuda:
        return i2v_native.inception_global_avg(pred.permute(0, 2, 3, 1).float().contiguous())
    return pred.mean((2, 3))


@torch.no_grad()
def get_activations(data, model, batch_size=50, dims=2048, cuda=False, verbose=False):
    """Features of the images ``data`` [N, 3, H, W] as a float64 array [n_used, dims].  They are collected in ONE device tensor and cross
    to the host once, at the end (the reference fills a host array with a synchronising copy per batch).

    KEPT QUIRKS: a ``batch_size`` above N is clipped to N, and only the ``N // batch_size`` whole batches are run -- the ragged rest is
    silently dropped.  ``cuda``: move each batch to the device first (a host-resident set never sits on the device as a whole)."""
    model.eval()
    total = data.size(0)
    step = min(batch_size, total)
    whole = total // step
    feats = None
    for k in range(whole):
        chunk = data[k * step:(k + 1) * step]
        f = _pooled(model(chunk.cuda() if cuda else chunk)[0])
        if feats is None:
            feats = torch.empty(whole * step, dims, dtype=torch.float32, device=f.device)
        feats[k * step:(k + 1) * step] = f
    if verbose:
        print(f"FID features: {whole} batches of {step} images, {total - whole * step} images left out")
    return feats.cpu().numpy().astype(np.float64)


def calculate_activation_statistics(data, model, batch_size=50, dims=2048, cuda=True, verbose=False):
    """(mean [dims], covariance [dims, dims] with n - 1 as ``np.cov``) of the features of ``data``, float64."""
    act = get_activations(data, model, batch_size, dims, cuda, verbose)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def calculate_FID(inception, seq_gen, seq_orig, batch_size, dims):
    """FID of two image tensors [N, 3, H, W] (on the device, or moved there batch by batch) -> (FID, N); the reference's signature."""
    if not torch.cuda.is_available():
        raise i2v_native.I2VError("FID needs a HIP device (torch.cuda.is_available() is False); this package has no CPU fallback")
    net = inception.cuda()
    stats = [calculate_activation_statistics(images, net, batch_size, dims, True) for images in (seq_gen, seq_orig)]
    return calculate_frechet_distance(*stats[0], *stats[1]), seq_gen.size(0)


class FIDAccumulator(StatsAccumulator):
    """Streaming FID: ``update(images, which)`` for images [B, 3, H, W] on the device, ``compute()`` at the end (``StatsAccumulator`` over the
    ``dims`` features of ``model``'s first output block, 2048 for the default ``InceptionV3``).  Every image counts."""

    def __init__(self, model, dims=2048):
        self.model = model
        super().__init__(dims)

    @torch.no_grad()
    def update(self, images, which):
        self._check_update(images, which)
        feats = _pooled(self.model(images.float().contiguous())[0]).contiguous()
        if feats.shape[1] != self.dim:
            raise ValueError(f"FIDAccumulator.update: the model returned {feats.shape[1]} features, the accumulator holds {self.dim}")
        self.update_features(feats, which)
        return feats
