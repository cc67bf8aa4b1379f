"""Output side of the sampling path: the on-disk tiling of generated sequences and the prior-sampling
loop that the reference's evaluation runs over a data loader.

Own implementations of the reference behaviour (``utils/auxiliaries.py:15-22`` GIF tiling, ``:53-55`` denormalisation,
``:87-101`` the sampling loop of ``evaluate_FVD_prior``) and the FVD evaluation hooks ``evaluate_FVD_prior`` /
``evaluate_FVD_posterior`` on the device (metrics/PyTorch_FVD, and with ``mode='DTFVD'`` metrics/DTFVD); wandb logging and video
writers of the reference are not rebuilt."""
import numpy as np
import torch


def denorm(x):
    """[-1, 1] -> [0, 1], clipped (reference semantics; the input is left untouched)."""
    return torch.clamp(x * 0.5 + 0.5, 0.0, 1.0)


def convert_seq2gif(sequence):
    """``[N, T, 3, H, W]`` in [-1, 1] -> float array ``[T, H, N*W, 3]``: the N clips side by side along the width, scaled
    so that the brightest value of the whole strip is 255 (the reference divides by the strip's own maximum, not by 1)."""
    n, t, c, h, w = sequence.shape
    strip = denorm(sequence.detach().float().cpu())          # [N, T, C, H, W]
    strip = strip.permute(1, 3, 0, 4, 2).reshape(t, h, n * w, c).numpy()
    peak = float(strip.max())
    return strip * (255.0 / peak)


def convert_grid2gif(videos):
    """``[N, K, T, 3, H, W]`` in [-1, 1] (K realizations of N start frames) -> float array ``[T, K*H, N*W, 3]``: row k is the strip
    ``convert_seq2gif`` lays out for realization k (the N clips side by side), and ONE normalisation over the whole grid scales its
    brightest value to 255 (so that the rows stay comparable).  K = 1 is ``convert_seq2gif(videos[:, 0])``."""
    n, k, t, c, h, w = videos.shape
    grid = denorm(videos.detach().float().cpu())             # [N, K, T, C, H, W]
    grid = grid.permute(2, 1, 4, 0, 5, 3).reshape(t, k * h, n * w, c).numpy()
    peak = float(grid.max())
    return grid * (255.0 / peak)


def convert_seq2gif_u8(sequence):
    """The bytes of ``convert_seq2gif(sequence).astype(np.uint8)``: ``[N, T, 3, H, W]`` -> uint8 ``[T, H, N*W, 3]``.  A CUDA tensor is
    converted on the device (csrc/i2v_frames.hip: one peak reduction, one interleaving kernel; no host round trip) and a uint8 DEVICE
    tensor comes back; a CPU tensor takes the numpy path and a numpy array comes back."""
    if sequence.dim() != 5:
        raise ValueError(f"convert_seq2gif_u8: expected [N,T,3,H,W], got {tuple(sequence.shape)}")
    if not sequence.is_cuda:
        return convert_seq2gif(sequence).astype(np.uint8)
    import i2v_native
    return i2v_native.frames_to_u8(sequence.detach(), mode="peak", layout="strip")


def convert_grid2gif_u8(videos):
    """The bytes of ``convert_grid2gif(videos).astype(np.uint8)``: ``[N, K, T, 3, H, W]`` -> uint8 ``[T, K*H, N*W, 3]``; device in, device
    out, as ``convert_seq2gif_u8``."""
    if videos.dim() != 6:
        raise ValueError(f"convert_grid2gif_u8: expected [N,K,T,3,H,W], got {tuple(videos.shape)}")
    if not videos.is_cuda:
        return convert_grid2gif(videos).astype(np.uint8)
    import i2v_native
    return i2v_native.frames_to_u8(videos.detach(), mode="peak", layout="strip")


def to_uint8_clips(sequence):
    """``[N, T, 3, H, W]`` (or ``[F, K, T, 3, H, W]``) in [-1, 1] -> uint8 ``[N, T, H, W, 3]`` (``[F, K, T, H, W, 3]``): what an encoder or a
    metric takes.  Fixed scale, rounded as ``tile_images`` rounds: ``denorm(x) * 255 + 0.5``, clamped to [0, 255], truncated.  A CUDA tensor
    is converted by the device kernel, a CPU tensor by the torch expression; both return a torch tensor on the input's device."""
    if sequence.dim() not in (5, 6):
        raise ValueError(f"to_uint8_clips: expected [N,T,3,H,W] or [F,K,T,3,H,W], got {tuple(sequence.shape)}")
    if sequence.is_cuda:
        import i2v_native
        return i2v_native.frames_to_u8(sequence.detach(), mode="unit", layout="clips")
    x = denorm(sequence.detach().float()).mul(255).add_(0.5).clamp_(0, 255)
    return x.movedim(-3, -1).to(torch.uint8).contiguous()


def tile_images(images, nrow=8, padding=2):
    """``torchvision.utils.save_image(images, ..., normalize=True)``'s picture as a uint8 array ``[H', W', 3]``: ``images`` [B, 3, H, W]
    min-max normalised over the whole tensor, tiled ``nrow`` per row with ``padding`` zero pixels around every tile (one image: no
    padding), rounded as save_image rounds (x * 255 + 0.5, clamped)."""
    x = images.detach().float().cpu().clone()
    lo, hi = float(x.min()), float(x.max())
    x = x.clamp(lo, hi).sub(lo).div(max(hi - lo, 1e-5))
    b, c, h, w = x.shape
    if b == 1:
        grid = x[0]
    else:
        xm = min(nrow, b)
        ym = -(-b // xm)
        grid = torch.zeros(c, ym * (h + padding) + padding, xm * (w + padding) + padding)
        for i in range(b):
            y, xx = divmod(i, xm)
            grid[:, y * (h + padding) + padding:y * (h + padding) + padding + h, xx * (w + padding) + padding:xx * (w + padding) + padding + w] = x[i]
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()


def _prior_batches(dloader, cINN, decoder, z_dim, control=False, generator=None):
    """The loop body shared by ``sample_prior`` and ``evaluate_FVD_prior``: yields (generated [B, 16, 3, H, W], original seq[:, 1:]) of
    every batch ON THE DEVICE."""
    for file in dloader:
        seq = file["seq"].float().cuda()
        b = seq.size(0)
        res = torch.randn(b, z_dim, generator=generator).cuda()
        x_0 = seq[:, 0].contiguous()
        cond = [x_0, file["cond"]] if control else [x_0]
        z = cINN(res, cond, reverse=True).view(b, -1)
        yield decoder(x_0, z), seq[:, 1:]


def _check_decoder_range(decoder, who):
    if hasattr(decoder, "native") and decoder.native().status():   # range guard of the split-fp16 operands (call after a synchronisation)
        raise RuntimeError(f"{who}: the decoder's activations left the fp16 range of the split-fp16 conv operands "
                           "(use mma = 0 for this checkpoint)")


@torch.no_grad()
def sample_prior(dloader, cINN, decoder, z_dim, control=False, generator=None):
    """The sampling loop of the reference's ``evaluate_FVD_prior`` (second caller of cINN^-1 + decoder): for every batch
    ``file`` of ``dloader`` (a dict with ``"seq"`` ``[B, T+1, 3, H, W]`` and, with ``control``, ``"cond"`` ``[B, 3]``) draw
    ``res ~ N(0, 1)`` on the CPU generator, invert the cINN conditioned on the first frame, decode, and collect
    ``(generated [N, 16, 3, H, W], original seq[:, 1:])`` on the CPU.  ``cINN`` is a ``SupervisedTransformer``-like callable
    ``cINN(res, cond, reverse=True)``, ``decoder`` a ``Generator``-like callable ``decoder(x_0, z)``."""
    gen, orig = [], []
    for g, o in _prior_batches(dloader, cINN, decoder, z_dim, control, generator):
        gen.append(g.cpu())
        _check_decoder_range(decoder, "sample_prior")   # (.cpu() synchronised)
        orig.append(o.cpu())
    return torch.cat(gen, dim=0), torch.cat(orig, dim=0)


def _fvd_accumulator(I3D, mode, who):
    """'FVD' with the Kinetics-400 I3D (metrics/PyTorch_FVD) or 'DTFVD' with a dynamic-texture InceptionI3D (metrics/DTFVD)."""
    if mode == 'DTFVD':
        from metrics.DTFVD.DTFVD_Score import DTFVDAccumulator
        from metrics.DTFVD.ID3 import InceptionI3D
        if not isinstance(I3D, InceptionI3D):
            raise NotImplementedError(f"{who}: mode 'DTFVD' needs the dynamic-texture network (metrics.DTFVD.DTFVD_Score.load_model), got "
                                      f"{type(I3D).__name__}; DTFVD on any other network is not built")
        return DTFVDAccumulator(I3D)
    if mode != 'FVD':
        raise NotImplementedError(f"{who}: mode {mode!r} -- only 'FVD' (the Kinetics-400 I3D of metrics/PyTorch_FVD) and 'DTFVD' (the "
                                  "dynamic-texture I3D of metrics/DTFVD) are built")
    from metrics.PyTorch_FVD.FVD_logging import FVDAccumulator
    return FVDAccumulator(I3D)


@torch.no_grad()
def evaluate_FVD_prior(dloader, cINN, decoder, I3D, z_dim, opt, epoch, mode, control):
    """PFVD, the reference's checkpoint-selection metric (``utils/auxiliaries.py:83-110``, argument list kept): sample one video per start
    frame of ``dloader`` from the prior (the ``sample_prior`` loop) and return the FVD between the generated clips and ``seq[:, 1:]``.

    No frame goes to the host: every batch is fed to a ``FVDAccumulator`` on the device as it is decoded.  All clips count (the reference's
    ``calculate_FVD(.., 20)`` drops the ragged last batch of 20).  The reference's side effects -- the GIF of ten random samples
    (``plot_vid``) and ``wandb.log`` -- are left out; ``opt`` and ``epoch`` only served them and are unused."""
    acc = _fvd_accumulator(I3D, mode, "evaluate_FVD_prior")   # (mode 'DTFVD': the accumulator's default is no de-normalisation)
    for g, o in _prior_batches(dloader, cINN, decoder, z_dim, control):
        acc.update(g, "gen")
        acc.update(o, "orig")
    value = acc.compute()   # (synchronises)
    _check_decoder_range(decoder, "evaluate_FVD_prior")
    return value


@torch.no_grad()
def evaluate_FVD_posterior(dloader, model, encoder, I3D, mode):
    """FVD of the stage-1 reconstructions (``utils/auxiliaries.py:65-81``, argument list kept): ``model(seq[:, 0], encoder(seq[:, 1:])[0])``
    against ``seq[:, 1:]``, accumulated on the device like ``evaluate_FVD_prior`` (all clips, no host copy of a frame)."""
    acc = _fvd_accumulator(I3D, mode, "evaluate_FVD_posterior")
    for file in dloader:
        seq = file["seq"].float().cuda()
        motion, *_ = encoder(seq[:, 1:].transpose(1, 2))
        acc.update(model(seq[:, 0].contiguous(), motion), "gen")
        acc.update(seq[:, 1:], "orig")
    return acc.compute()
