"""Diversity on the device: own implementation of the reference's ``metrics/Diversity/I3D.py`` surface.

The diversity score of a stochastic video model is the mean squared distance between the features of several samples of ONE start frame:
for embeddings ``embed`` [N instances, R realizations, D] the mean over all ordered pairs i != j of
``((embed[:, i] - embed[:, j]) ** 2).mean()``.  ``compute_DTI3D_diversity`` measures it in the 1024-d features of the dynamic-texture
I3D (metrics/DTFVD); it takes the videos where ``Model.sample`` left them -- [N, R, T, 3, H, W] on the device -- embeds them with the
native I3D (``embedding_I3D``'s input rule: the first 16 frames, values as they are; length 32: exactly 32 frames) and reduces the pairs
on the device in float64 (``i2v_diversity_update``).  No frame and no embedding goes to the host; two scalars do.

Differences from the reference, on purpose:
  * the reference's pair loop hard-codes 5 realizations (``range(5)``); here the loop runs over R, the size of dimension 1;
  * the printed figure keeps the reference's ``x 1000``; the function also RETURNS the unscaled mean (the reference returns nothing).
Kept: the batches of 20 per realization with ``get_activations``' ragged-batch drop -- with more than ``batch_size`` instances only
``N // batch_size * batch_size`` of them count.  ``DiversityAccumulator`` is the streaming form for sets that do not fit: every instance
it is given counts.

``compute_I3D_diversity`` (Kinetics I3D through TF-hub) and ``compute_vgg_diversity`` (torchvision VGG) are not built."""
import torch

import i2v_native
from metrics.DTFVD import DTFVD_Score


class DiversityAccumulator:
    """Streaming pair diversity: ``update(frames [F, R, T, 3, H, W])`` for videos on the device, ``compute()`` at the end.

    Keeps (sum over instances and ordered pairs of the mean squared feature distance, number of such terms) as two float64 on the device;
    ``compute()`` is their quotient -- the reference's ``np.mean(div)`` whenever every pair has the same number of instances, which is
    always the case here.  One workgroup owns the sums and adds in a fixed order: two runs give the same bits."""

    def __init__(self, model, batch_size=20):
        self.model = model
        self.batch_size = int(batch_size)
        self._acc = None

    def reset(self):
        self._acc = None

    @torch.no_grad()
    def embed(self, frames):
        """[F, R, T, 3, H, W] -> [F, R, 1024] fp32 on the device, ``batch_size`` clips per forward."""
        if frames.dim() != 6 or frames.shape[3] != 3:
            raise ValueError(f"DiversityAccumulator: expected videos [F,R,T,3,H,W], got {tuple(frames.shape)}")
        if not frames.is_cuda:
            raise i2v_native.I2VError("DiversityAccumulator takes videos on a HIP device (no frame goes through the host); this package has "
                                      "no CPU fallback")
        F, R, T = frames.shape[:3]
        if self.model.LENGTH == 32:
            if T != 32:
                raise ValueError(f"DiversityAccumulator: the length-32 network takes clips of exactly 32 frames, got {T}")
            t_out = None
        else:
            t_out = min(T, 16)
        flat = frames.reshape(F * R, *frames.shape[2:])
        out = torch.empty(F * R, self.model.feature_dim, dtype=torch.float32, device=frames.device)
        for i in range(0, F * R, self.batch_size):
            out[i:i + self.batch_size] = self.model.forward_frames(flat[i:i + self.batch_size], False, t_out)
        return out.view(F, R, -1)

    def update(self, frames):
        emb = self.embed(frames)
        self.update_embeddings(emb)
        return emb

    def update_embeddings(self, emb):
        if emb.shape[1] < 2:
            raise ValueError(f"DiversityAccumulator: at least 2 realizations per instance are needed, got {emb.shape[1]}")
        if self._acc is None:
            self._acc = torch.zeros(2, dtype=torch.float64, device=emb.device)
        i2v_native.diversity_update(emb.contiguous(), self._acc)

    def state(self):
        """Host copy (sum, count) as a float64 array [2]."""
        if self._acc is None:
            raise ValueError("DiversityAccumulator: no update yet")
        return self._acc.cpu().numpy().copy()

    def compute(self):
        s, n = self.state()
        return float(s / n)


def compute_DTI3D_diversity(seq1, I3D=None, batch_size=20):
    """Diversity of ``seq1`` [N, R, T, 3, H, W] (on the device, in [-1, 1]; e.g. straight from ``Model.sample``) in the features of the
    dynamic-texture I3D.  ``I3D``: a loaded ``metrics.DTFVD`` network (None: ``load_model`` of the length the clips ask for, as the
    reference does).  Prints the reference's line (the figure x 1000) and returns the unscaled mean."""
    if seq1.dim() != 6:
        raise ValueError(f"compute_DTI3D_diversity: expected videos [N,R,T,3,H,W], got {tuple(seq1.shape)}")
    if not seq1.is_cuda:
        raise i2v_native.I2VError("compute_DTI3D_diversity takes videos on a HIP device; this package has no CPU fallback")
    if I3D is None:
        I3D = DTFVD_Score.load_model(length=32 if seq1.size(2) > 16 else 16).cuda()
    n = seq1.size(0)
    n_used = n if n < batch_size else n // batch_size * batch_size   # get_activations' ragged-batch drop, per realization
    acc = DiversityAccumulator(I3D, batch_size)
    for i in range(0, n_used, batch_size):
        acc.update(seq1[i:min(i + batch_size, n_used)])
    value = acc.compute()
    print(f'Diversity score of {value * 1000} using I3D backbone pretrained on dynamic textures')
    return value


def compute_I3D_diversity(seq1, n_samples):
    raise NotImplementedError("compute_I3D_diversity is not built: it embeds with the Kinetics I3D of the TensorFlow FVD "
                              "(metrics/FVD/evaluate_FVD.get_embeddings, a TF-hub module), and neither TensorFlow nor that module is part of "
                              "this package; compute_DTI3D_diversity is")
