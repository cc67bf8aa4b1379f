"""VGG diversity on the device: own implementation of the reference's ``metrics/Diversity/VGG.py`` surface.

``compute_vgg_diversity(videos, vgg)`` runs the reference's loop on ``videos`` [N, R, T, 3, H, W] (on the device, in [-1, 1]): every frame
is de-normalised, normalised with the ImageNet constants and THEN resized to 224 x 224 (the reference's order), goes through the
VGG-16 trunk, and for every video the mean squared difference of the five feature maps is taken over all ordered pairs of realizations.
One group of R images (one video, one time step) is processed at a time -- the 224 x 224 taps of all R x T images are never alive at
once -- and the pairs are reduced on the device in float64 (``i2v_vgg_pairdiff_update``); two scalars go to the host.

kornia is not a dependency.  Its ``Resize(size=(224, 224))`` is fixed here as
``F.interpolate(..., size=(224, 224), mode='bilinear', align_corners=False)``; ``align_corners=True`` is an argument.
Kept: the range checks, the square frames (``img_res = videos.size(-1)``), the printed line.  The function also RETURNS the mean over
the N R (R - 1) 5 terms (the reference returns nothing).  Without a loaded ``vgg`` it raises as before: there are no weights to fall
back to."""
import torch

import i2v_native


def compute_vgg_diversity(videos, vgg=None, align_corners=False):
    """
    Computes diversity based on VGG backbone trained on ImageNet

    Input: PyTorch tensor of shape (BatchSize, NumberSamples, Time, Channel, H, W)
        Important input needs to be in range [-1, 1] !
    ``vgg``: a loaded ``stage2_cINN.AE.modules.vgg16.vgg16`` on the device.
    """
    if vgg is None:
        raise NotImplementedError("compute_vgg_diversity is not built without weights: it needs torchvision's VGG-16 ImageNet weights, which are "
                                  "not part of this package -- pass vgg=vgg16(path=<torchvision vgg16 state_dict file>).cuda(); "
                                  "metrics.Diversity.I3D.compute_DTI3D_diversity needs none")
    if videos.dim() != 6 or videos.shape[3] != 3:
        raise ValueError(f"compute_vgg_diversity: expected videos [N,R,T,3,H,W], got {tuple(videos.shape)}")
    if not videos.is_cuda:
        raise i2v_native.I2VError("compute_vgg_diversity takes videos on a HIP device; this package has no CPU fallback")
    print('Evaluate Diversity score based on VGG trained on ImageNet')
    n_samples = videos.size(1)
    if n_samples < 2:
        raise ValueError(f"compute_vgg_diversity: at least 2 realizations per instance are needed, got {n_samples}")

    ## check if videos are in correct range
    assert videos.min() < 0
    assert videos.max() <= 1
    img_res = videos.size(-1)
    seq_length = videos.size(2)
    if videos.size(-2) != img_res:
        raise ValueError(f"compute_vgg_diversity: square frames are expected (the reference reshapes to img_res x img_res), got {tuple(videos.shape[-2:])}")

    native = vgg.native()
    acc = torch.zeros(2, dtype=torch.float64, device=videos.device)
    taps = None
    with torch.no_grad():
        for video in videos.float():
            for t in range(seq_length):
                x = i2v_native.vgg_input_stage(video[:, t].contiguous(), i2v_native.VGG_INPUT_DIVERSITY, (224, 224), align_corners)
                taps = native.features(x, taps)
                for fmap in taps:
                    i2v_native.vgg_pairdiff_update(fmap, acc)
    # every term of the reference is a mean over (T, C, H, W): the T groups of one video share its R (R - 1) 5 terms
    s, cnt = acc.cpu().tolist()
    value = s / cnt
    print(f'Diversity score of {value} using VGG backbone')
    return value
