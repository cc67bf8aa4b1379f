"""Class-surface mirror of the reference's ``metrics/DTFVD/ID3_32.py``: the dynamic-texture I3D trained on 32-frame clips.  The reference
file is ``ID3.py`` with one line changed -- ``AvgPool3d((4, 7, 7))`` in place of ``((2, 7, 7))`` -- and so is this one: the same keys
(``I3D_32.pth.tar['state_dict']`` loads with ``strict=True``), the native handle created with length 32.  At least 25 frames are needed;
the 1024-wide feature (one time step behind the pool) takes 25 to 32, and ``DTFVD_Score.calculate_FVD32`` asks for exactly 32."""
from metrics.DTFVD import ID3
from metrics.DTFVD.ID3 import MIXED, Unit3D, InceptionModule, compute_pad  # noqa: F401


def endpoint_shapes(T, H=224, W=224, batch=1):
    return ID3.endpoint_shapes(T, H, W, batch, pool_t=4)


class InceptionI3D(ID3.InceptionI3D):
    LENGTH = 32
    POOL_T = 4
