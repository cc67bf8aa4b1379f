"""FVD on the device: own implementation of the reference's ``metrics/PyTorch_FVD/FVD_logging.py`` surface.

The reference takes every generated frame to the host, resizes the whole set to 224 x 224 on the CPU and feeds it back to the GPU in
batches.  Here frames stay where the decoder wrote them: the resize and the de-normalisation are the input stage of the native I3D
(csrc/i2v_i3d.hip), and the activation statistics are accumulated on the device (``i2v_fvd_stats_update``).  Only the (n, sum, gram)
triple of a set reaches the host, where the Frechet distance is evaluated in float64 with numpy (no scipy).

Two quirks of the reference are KEPT in the functions that carry its names, and documented:
  * ``get_activations`` silently drops the ragged last batch (``n // batch_size`` batches);
  * ``preprocess`` de-normalises a set by ``(x + 1) / 2`` only when its global minimum is negative (one device reduction here).
``FVDAccumulator`` is the streaming form the evaluation hook uses; it has neither quirk's cost: it uses every clip it is given and
takes the de-normalisation decision as an argument."""
import numpy as np
import torch
import torch.nn.functional as F

import i2v_native
from metrics.PyTorch_FVD.I3D import I3D


# ---------------------------------------------------------------------------------------------- Frechet distance (host, float64)
def _sqrt_psd(m):
    w, v = np.linalg.eigh((m + m.T) * 0.5)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = ||mu1 - mu2||^2 + tr(S1) + tr(S2) - 2 tr sqrt(S1 S2) in float64.

    tr sqrt(S1 S2) is the sum of the square roots of the eigenvalues of S1^(1/2) S2 S1^(1/2) (symmetric positive semi-definite, the same
    spectrum as S1 S2; ``numpy.linalg.eigh``, negatives clamped to 0) where the reference calls ``scipy.linalg.sqrtm`` on S1 S2.  A
    rank-deficient product needs no special case in this formulation; ``eps`` is accepted for the reference's signature and unused."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    diff = mu1 - mu2
    root1 = _sqrt_psd(sigma1)
    m = root1 @ sigma2 @ root1
    ev = np.linalg.eigvalsh((m + m.T) * 0.5)
    tr_covmean = np.sqrt(np.clip(ev, 0.0, None)).sum()
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2.0 * tr_covmean)


def stats_from_sums(n, total, gram):
    """(n, sum [D], gram [D, D]) -> (mean, covariance with n - 1 as ``np.cov``), float64."""
    total, gram = np.asarray(total, dtype=np.float64), np.asarray(gram, dtype=np.float64)
    if n < 2:
        raise ValueError(f"FVD statistics need at least 2 clips per set (got {n})")
    mu = total / n
    return mu, (gram - n * np.outer(mu, mu)) / (n - 1)


# ---------------------------------------------------------------------------------------------- the reference's function names
def load_model(path='./models/PI3D/model_rgb.pth'):
    model = I3D(400, 'rgb')
    model.load_state_dict(torch.load(path, map_location="cpu"))
    model.eval()
    return model


def denorm(x):
    return (x + 1.0) / 2.0


def _needs_denorm(data):
    """The reference's ``if data.min() < 0``: one device reduction, one scalar to the host.  The reference tests the RESIZED set; here the
    set is never materialised at 224 x 224, so the test is taken on the frames as they are.  A bilinear resize is a convex combination, so
    the two agree for every set whose negative values are more than isolated pixels outweighed by their neighbours -- in particular for
    [-1, 1] and for [0, 1] data, the two ranges the pipeline produces."""
    return bool(data.min() < 0)


def preprocess(data_gen, data_orig):
    """The reference's preprocess as a function of its own: [N, T, 3, H, W] sets resized to 224 x 224 (bilinear, align_corners=True) and
    de-normalised when their global minimum is negative.  The product path (``get_activations``) does NOT call it -- there the native
    input stage does the same per batch without materialising the resized set; this function is for inspection."""
    out = []
    for d in (data_gen, data_orig):
        r = F.interpolate(d.reshape(-1, *d.shape[2:]), mode='bilinear', size=(224, 224), align_corners=True).reshape(*d.shape[:2], 3, 224, 224)
        out.append(denorm(r) if _needs_denorm(r) else r)
    return out[0], out[1]


def _device_set(data, cuda):
    if not cuda and not data.is_cuda:
        raise i2v_native.I2VError("FVD runs on a HIP device only (native I3D); this package has no CPU fallback -- pass cuda=True")
    if not torch.cuda.is_available():
        raise i2v_native.I2VError("FVD needs a HIP device (torch.cuda.is_available() is False); this package has no CPU fallback")
    return data if data.is_cuda else data.cuda()


@torch.no_grad()
def get_activations(data, model, batch_size=50, cuda=False, verbose=False, denorm_input=None):
    """Logits of the clips ``data`` [N, T, 3, H, W] (any H, W), batch by batch, as a float64 array [n_used, num_classes].

    KEPT QUIRK: like the reference, ``n // batch_size`` batches are run and the ragged rest is silently dropped.  ``denorm_input``:
    whether the values are in [-1, 1] (None = the reference's rule, decided once for the whole set by ``preprocess``'s test)."""
    model.eval()
    data = _device_set(data, cuda)
    n = data.size(0)
    batch_size = min(batch_size, n)
    n_batches = n // batch_size
    if denorm_input is None:
        denorm_input = _needs_denorm(data)
    out = torch.empty(n_batches * batch_size, model.num_classes, dtype=torch.float32, device=data.device)
    for i in range(n_batches):
        out[i * batch_size:(i + 1) * batch_size] = model.forward_frames(data[i * batch_size:(i + 1) * batch_size].float().contiguous(),
                                                                        denorm_input)
    return out.cpu().numpy().astype(np.float64)


def calculate_activation_statistics(data, model, batch_size=50, cuda=True, verbose=False):
    act = get_activations(data, model, batch_size, cuda, verbose)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def calculate_FVD(model, data_gen, data_orig, batch_size, cuda=True):
    """FVD of two sets of clips [N, T, 3, H, W] (on the device, or moved there as a whole); the reference's signature and quirks."""
    m1, s1 = calculate_activation_statistics(data_gen, model, batch_size, cuda)
    m2, s2 = calculate_activation_statistics(data_orig, model, batch_size, cuda)
    return calculate_frechet_distance(m1, s1, m2, s2)


def compute_activations(model, data_gen, data_orig, batch_size, cuda=True):
    return get_activations(data_orig, model, batch_size, cuda), get_activations(data_gen, model, batch_size, cuda)


# ---------------------------------------------------------------------------------------------- streaming form
class StatsAccumulator:
    """Streaming Frechet statistics of two sets of D-dimensional features: the part that ``FVDAccumulator``, ``DTFVDAccumulator`` and
    ``metrics.FID.FID_Score.FIDAccumulator`` share.  Per set ('gen' / 'orig') it keeps n, sum [D] and gram [D, D] in float64 ON THE DEVICE
    (``i2v_fvd_stats_update``: one owner per element, rows in order, no atomics -- two runs give the same bits); ``compute()`` brings the
    two triples to the host and evaluates the Frechet distance there.  ``state()`` / ``load_state()`` save and restore the triples, so the
    statistics of the real set can be computed once and reused across epochs (the reference recomputes them every epoch).  A subclass
    adds ``update``: its network's features of a batch, handed to ``update_features``."""

    SETS = ("gen", "orig")

    def __init__(self, dim):
        self.dim = dim
        self._n, self._sum, self._gram = {}, {}, {}
        self.reset()

    def reset(self, which=None):
        for k in (self.SETS if which is None else (which,)):
            self._n[k], self._sum[k], self._gram[k] = 0, None, None

    def _check_update(self, frames, which):
        name = type(self).__name__
        if which not in self.SETS:
            raise ValueError(f"{name}.update: which must be one of {self.SETS}, got {which!r}")
        if not frames.is_cuda:
            raise i2v_native.I2VError(f"{name}.update takes frames on a HIP device (no frame goes through the host); this package has "
                                      "no CPU fallback")

    def update_features(self, feats, which):
        if self._sum[which] is None:
            self._sum[which] = torch.zeros(self.dim, dtype=torch.float64, device=feats.device)
            self._gram[which] = torch.zeros(self.dim, self.dim, dtype=torch.float64, device=feats.device)
        i2v_native.fvd_stats_update(feats, self._sum[which], self._gram[which])
        self._n[which] += feats.shape[0]

    def state(self, which=None):
        """Host copy {set: {"n", "sum", "gram"}} of one set or of both."""
        out = {}
        for k in (self.SETS if which is None else (which,)):
            if self._sum[k] is not None:
                out[k] = {"n": self._n[k], "sum": self._sum[k].cpu().numpy().copy(), "gram": self._gram[k].cpu().numpy().copy()}
        return out

    def load_state(self, state, device=None):
        for k, s in state.items():
            if k not in self.SETS:
                raise ValueError(f"{type(self).__name__}.load_state: unknown set {k!r}")
            total, gram = np.asarray(s["sum"], dtype=np.float64), np.asarray(s["gram"], dtype=np.float64)
            if total.shape != (self.dim,) or gram.shape != (self.dim, self.dim):
                raise ValueError(f"{type(self).__name__}.load_state: set {k!r} has shapes {total.shape}, {gram.shape} for {self.dim} features")
            self._n[k] = int(s["n"])
            dev = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
            self._sum[k], self._gram[k] = torch.from_numpy(total.copy()).to(dev), torch.from_numpy(gram.copy()).to(dev)

    def compute(self):
        st = self.state()
        if set(st) != set(self.SETS):
            raise ValueError(f"{type(self).__name__}.compute: both sets need at least one update")
        m1, s1 = stats_from_sums(st["gen"]["n"], st["gen"]["sum"], st["gen"]["gram"])
        m2, s2 = stats_from_sums(st["orig"]["n"], st["orig"]["sum"], st["orig"]["gram"])
        return calculate_frechet_distance(m1, s1, m2, s2)


class FVDAccumulator(StatsAccumulator):
    """Streaming FVD: ``update(frames, which)`` for frames on the device, ``compute()`` at the end (``StatsAccumulator`` over the logits of
    the Kinetics I3D).  Unlike ``get_activations`` it uses EVERY clip it is given (there is no ragged-batch drop), so with a set size that
    is not a multiple of the batch its value differs from the reference's, which ignores the rest."""

    def __init__(self, model):
        self.model = model
        super().__init__(model.num_classes)

    @torch.no_grad()
    def update(self, frames, which, denorm_input=True):
        """frames [B, T, 3, H, W] fp32 on the device, ``denorm_input``: the values are in [-1, 1] (the decoder's and the loaders' range)."""
        self._check_update(frames, which)
        feats = self.model.forward_frames(frames.float().contiguous(), denorm_input)
        self.update_features(feats, which)
        return feats
