"""The motion-encoder configuration cases shared by tests/golden/make_golden.py (``encoder3d_cfgs``), test_host_encoder_configs.py and
test_gpu_encoder_configs.py, and a pure-Python restatement of the kernel choice of ``i2v_encoder3d_load`` / ``_forward``
(csrc/i2v_encoder.hip).  No torch import: make_golden.py loads this file by path."""

# name, channels, stride_s, stride_t, frame size, frames, batch.  Cases 1-9 have the reference's 64-channel stem and are pinned to the
# reference module's outputs (tests/golden/enc3d_cfgs.npz); the reference hard-codes ``self.inplanes = 64`` (resnet3D.py:141) and cannot
# build the last two, which are pinned to the float64 oracle only.
REF_CASES = (
    ("dtdb",       (64, 64, 128, 256, 512),  (2, 2, 2, 2), (1, 2, 2, 2), 128, 16, 1),   # shipped DTDB config: s2d with equal widths
    ("nodown_l0",  (64, 64, 32, 48, 80),     (1, 2, 2, 2), (1, 2, 2, 2), 64, 16, 3),    # first block without downsample; widths 48, 80
    ("t8",         (64, 32, 32, 48, 64),     (1, 2, 2, 2), (1, 2, 2, 2), 64, 8, 3),     # last layer at T == 1: *_s2d_t1
    ("t7_128",     (64, 32, 32, 48, 64),     (2, 2, 2, 2), (1, 2, 2, 2), 128, 7, 1),    # the same at 128^2, odd frame count
    ("t3",         (64, 32, 32, 48, 64),     (1, 2, 2, 2), (1, 2, 2, 2), 64, 3, 5),     # stem T = 2, two single-frame strided layers
    ("st2_ss1",    (64, 32, 32, 48, 64),     (1, 2, 2, 2), (2, 2, 2, 1), 64, 15, 2),    # fp32 conv_forward with temporal stride only
    ("st2_ss1_t1", (64, 32, 48, 64, 64),     (2, 2, 1, 2), (2, 2, 2, 2), 64, 4, 2),     # the same path at T == 1 (st_eff = 1)
    ("st1122",     (64, 32, 48, 64, 32),     (2, 2, 2, 1), (1, 1, 2, 2), 64, 8, 2),     # spatial stride 1 in the last layer
    ("wide1024",   (64, 64, 128, 512, 1024), (1, 2, 2, 2), (1, 2, 2, 2), 64, 16, 1),    # 1024-channel sums / coef buffers, head 16384 -> 128
)
ORACLE_ONLY_CASES = (
    ("c0_16",      (16, 16, 32, 48, 80),     (1, 2, 2, 2), (1, 2, 2, 2), 64, 16, 3),    # minimum width everywhere
    ("c0_80",      (80, 48, 48, 64, 64),     (1, 2, 2, 2), (1, 2, 2, 2), 64, 15, 1),    # widest stem the LDS check admits
)
Z_DIM = 64


def _case(k, row):
    name, channels, stride_s, stride_t, size, frames, batch = row
    return dict(name=name, synth=dict(seed=30 + k, z_dim=Z_DIM, channels=list(channels), stride_s=list(stride_s)),
                stride_t=list(stride_t), x_seed=100 + k, x_shape=[batch, 3, frames, size, size])


CASES = {row[0]: _case(k, row) for k, row in enumerate(REF_CASES + ORACLE_ONLY_CASES, start=1)}
REF_NAMES = tuple(r[0] for r in REF_CASES)
ALL_NAMES = tuple(CASES)

MEMBERS = ("c1_16", "s2d", "s2d_t1", "fp32_strided", "fp32_t1")


def encoder_paths(channels, stride_s, stride_t, frames):
    """[(member, has_down)] for the first block of each of the four layers: which packed weight set / kernel
    ``i2v_encoder3d_forward`` runs its strided conv1 (and downsample conv) on for a clip of ``frames`` frames.

    ``c1_16``: stride-1 split-fp16 conv; ``s2d``: space-to-depth split-fp16 conv; ``s2d_t1``: its single-frame weight set
    (temporal stride 2 on one frame runs as stride 1); ``fp32_strided``: exact-fp32 conv_forward with a temporal stride only;
    ``fp32_t1``: that conv on a single frame, run with stride 1.  Raises ValueError where ``i2v_encoder3d_create`` refuses."""
    t = (frames - 1) // 2 + 1            # stem: kernel 3, stride 2, pad 1
    out, inplanes = [], channels[0]
    for ss, st, planes in zip(stride_s, stride_t, channels[1:]):
        has_down = ss != 1 or inplanes != planes
        if ss == 1 and st == 2 and not has_down:
            raise ValueError("stride_t 2 with stride_s 1 and equal widths: no downsample branch for the half-rate residual")
        st_eff = 1 if t == 1 else st
        if ss == 1 and st == 1:
            member = "c1_16"
        elif ss == 2:
            member = "s2d" if st_eff == st else "s2d_t1"
        else:
            member = "fp32_strided" if st_eff == st else "fp32_t1"
        out.append((member, has_down))
        t = (t + 1) // 2 if st == 2 else t
        inplanes = planes
    return out
