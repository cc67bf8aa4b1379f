"""DTFVD on the device: own implementation of the reference's ``metrics/DTFVD/DTFVD_Score.py`` surface -- the Frechet distance of the
1024-d pooled features of the dynamic-texture I3D, the metric the texture checkpoints (Landscape, DTDB) are selected and compared by.

The reference resizes the whole set to 224 x 224 on the host and feeds it to the GPU in batches.  Here the clips stay on the device at
their own size: the resize and the time rule are the input stage of the native I3D (csrc/i2v_i3d.hip, ``i2v_i3d_features``); nothing is
materialised at 224 x 224.  The Frechet distance is the package's float64 eigenvalue formulation
(``metrics.PyTorch_FVD.FVD_logging.calculate_frechet_distance``; no scipy, no kornia).

Quirks of the reference that are KEPT in the functions that carry its names:
  * NO de-normalisation: the network sees the values as they are, [-1, 1] from the decoder and the loaders (the Kinetics FVD maps to
    [0, 1] first; this metric does not);
  * ``calculate_FVD`` tiles a clip three times in time and keeps the first 16 frames (``.repeat(1, 3, 1, 1, 1)[:, :16]``): frame t is
    source frame t % T, and a clip longer than 16 frames is cut to its first 16;
  * ``embedding_I3D`` only cuts (``[:, :16]``), it does not tile;
  * ``get_activations`` silently drops the ragged last batch (``n // batch_size`` batches).
One quirk is NOT kept: the reference's ``assert data_orig.size(1) == 32 & data_gen.size(1) == 32`` parses as a chained comparison around
``32 & data_gen.size(1)`` and lets other lengths through; ``calculate_FVD32`` here requires both sets to have exactly 32 frames.
``DTFVDAccumulator`` is the streaming form the evaluation hooks use: every clip counts, statistics stay on the device."""
import numpy as np
import torch

from metrics.DTFVD import ID3, ID3_32
from metrics.PyTorch_FVD.FVD_logging import FVDAccumulator, _device_set, calculate_frechet_distance  # noqa: F401  (the eigh formulation)


@torch.no_grad()
def get_activations(data, model, batch_size=50, cuda=False, verbose=False, t_out=None):
    """Pooled features of the clips ``data`` [N, T, 3, H, W] (any H, W; values as they are), batch by batch, as a float64 array
    [n_used, 1024].  KEPT QUIRK: ``n // batch_size`` batches are run and the ragged rest is silently dropped.  ``t_out``: frames per clip
    that enter the network (frame t = source frame t % T); None = all of them."""
    model.eval()
    data = _device_set(data, cuda)
    n = data.size(0)
    batch_size = min(batch_size, n)
    n_batches = n // batch_size
    out = torch.empty(n_batches * batch_size, model.feature_dim, dtype=torch.float32, device=data.device)
    for i in range(n_batches):
        out[i * batch_size:(i + 1) * batch_size] = model.forward_frames(data[i * batch_size:(i + 1) * batch_size], False, t_out)
    return out.cpu().numpy().astype(np.float64)


def calculate_activation_statistics(data, model, batch_size=50, cuda=True, verbose=False, t_out=None):
    act = get_activations(data, model, batch_size, cuda, verbose, t_out)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def calculate_FVD(model, data_gen, data_orig, batch_size, cuda=True):
    """DTFVD of two sets of clips [N, T, 3, H, W] with the length-16 network; the reference's signature and quirks (tile x 3, first 16)."""
    m1, s1 = calculate_activation_statistics(data_gen, model, batch_size, cuda, t_out=16)
    m2, s2 = calculate_activation_statistics(data_orig, model, batch_size, cuda, t_out=16)
    return calculate_frechet_distance(m1, s1, m2, s2)


def _require_32(name, *sets):
    for d in sets:
        if d.size(1) != 32:
            raise ValueError(f"{name}: the length-32 network takes clips of exactly 32 frames, got {d.size(1)}")


def calculate_FVD32(model, data_gen, data_orig, batch_size, cuda=True):
    """DTFVD with the length-32 network.  Both sets must have exactly 32 frames (the reference's assert is weaker, see the module text)."""
    _require_32("calculate_FVD32", data_gen, data_orig)
    m1, s1 = calculate_activation_statistics(data_gen, model, batch_size, cuda)
    m2, s2 = calculate_activation_statistics(data_orig, model, batch_size, cuda)
    return calculate_frechet_distance(m1, s1, m2, s2)


def embedding_I3D(model, data, batch_size, cuda=True):
    """Features [n_used, 1024] of the first 16 frames of ``data`` [N, T, 3, H, W] (cut, not tiled)."""
    return get_activations(data, model, batch_size, cuda, t_out=min(int(data.size(1)), 16))


def embedding_I3D_32(model, data, batch_size, cuda=True):
    _require_32("embedding_I3D_32", data)
    return get_activations(data, model, batch_size, cuda)


def load_model(length, path=None):
    """``InceptionI3D(18, 1)`` of the given length (32, else 16) filled from ``path`` (default: the reference's ``./models/DTI3D/...``)."""
    if length == 32:
        model = ID3_32.InceptionI3D(18, 1)
        model_path = './models/DTI3D/length32/I3D_32.pth.tar'
    else:
        model = ID3.InceptionI3D(18, 1)
        model_path = './models/DTI3D/length16/I3D_16.pth.tar'
    model.load_state_dict(torch.load(path or model_path, map_location="cpu")['state_dict'])
    _ = model.eval()
    return model


class DTFVDAccumulator(FVDAccumulator):
    """``FVDAccumulator`` over the 1024-d features of a dynamic-texture ``InceptionI3D``: same ``update`` / ``update_features`` /
    ``state`` / ``load_state`` / ``compute``, statistics in float64 on the device.  ``update`` applies ``calculate_FVD``'s input rule for
    the length-16 network (frame t = source frame t % T, 16 frames) and ``calculate_FVD32``'s for the length-32 one (exactly 32 frames),
    and takes ``denorm_input=False``: the reference does not de-normalise for this metric."""

    def __init__(self, model):
        if not isinstance(model, ID3.InceptionI3D):
            raise TypeError(f"DTFVDAccumulator takes a metrics.DTFVD InceptionI3D, got {type(model).__name__}")
        self.model = model
        self.dim = model.feature_dim   # (the base class reads model.num_classes, the width of the Kinetics logits)
        self._n, self._sum, self._gram = {}, {}, {}
        self.reset()

    @torch.no_grad()
    def update(self, frames, which, denorm_input=False):
        """frames [B, T, 3, H, W] fp32 on the device, values as they are."""
        import i2v_native
        if which not in self.SETS:
            raise ValueError(f"DTFVDAccumulator.update: which must be one of {self.SETS}, got {which!r}")
        if not frames.is_cuda:
            raise i2v_native.I2VError("DTFVDAccumulator.update takes frames on a HIP device (no frame goes through the host); this package "
                                      "has no CPU fallback")
        if self.model.LENGTH == 32:
            _require_32("DTFVDAccumulator.update", frames)
            feats = self.model.forward_frames(frames, denorm_input)
        else:
            feats = self.model.forward_frames(frames, denorm_input, t_out=16)
        self.update_features(feats.contiguous(), which)
        return feats
