#!/usr/bin/env python
"""Diversity CLI, mirror of the reference's ``eval_diversity.py``:

    python eval_diversity.py -gpu 0 -dataset DTDB -texture fire -ckpt_path DIR/ -clips_npy real.npy -DTI3D True [-n_realiz 5] [-seq_length 16]

``-n_realiz`` videos are sampled per start frame and the mean squared distance between their features is reported.  Built: ``-DTI3D``
(the features of the dynamic-texture I3D, metrics/Diversity/I3D.py ``compute_DTI3D_diversity``, on the device; the length-32 network
when ``-seq_length > 16``); it prints the reference's line.  ``-I3D`` (Kinetics I3D through TF-hub) exits with a "not built" message.

The reference's data package is out of scope, so the start frames come from ``-clips_npy FILE``: ``[N, T, 3, H, W]`` (frame 0 of every
clip is used, as the reference uses ``seq[:, 0]``) or ``[N, 3, H, W]``, float in [-1, 1].  The reference runs ``-n_realiz`` passes over
the loader; here the realizations of a batch come from ONE ``Model.sample(x_0, n_realiz)`` call (the start-frame work is done once) and
stay on the device as [F, R, T, 3, H, W], so the residuals are drawn frame-major instead of pass-major: the same distribution, other
draws.  ``-VGG True -vgg_path FILE`` (torchvision's vgg16 state_dict file; nothing is downloaded) runs ``compute_vgg_diversity`` on the same
videos with the native VGG-16 trunk; without ``-vgg_path`` it exits with the "not built" message.  ``-i3d_path`` overrides the I3D checkpoint, ``-seed`` the reference's fixed 249; ``-embed_npy`` / ``-embed_seed`` / ``-dec_mma`` as
in ``generate_samples.py``."""
import argparse
import os
import sys

NOT_BUILT = {"I3D": "the Kinetics-I3D diversity embeds with the TensorFlow FVD's TF-hub module (metrics/FVD), which is not built"}
NEEDS_PATHS = {"VGG": (("vgg_path",), "the VGG diversity needs torchvision's VGG-16 ImageNet weights, which are not part of this package: pass "
                                      "-vgg_path FILE (torchvision's vgg16 state_dict, vgg16-397923af.pth)")}


def parse(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument('-gpu', type=str, required=True, help="Define GPU on which to run")
    parser.add_argument('-dataset', type=str, required=True, help='Specify dataset')
    parser.add_argument('-texture', type=str, help='Specify texture when using DTDB')
    parser.add_argument('-ckpt_path', type=str, required=False)
    parser.add_argument('-data_path', type=str, required=False, help="(reference flag; the data package is not built, use -clips_npy)")
    parser.add_argument('-seq_length', type=int, default=16, help='Number of frames to predict')
    parser.add_argument('-n_realiz', type=int, default=5, help='How many samples should be generated for each test instance')
    parser.add_argument('-bs', type=int, default=6, help='Batchsize')
    parser.add_argument('-I3D', type=bool, help='Evaluation using kinetics I3D backbone (not built)')
    parser.add_argument('-VGG', type=bool, help='Evaluation using VGG backbone (needs -vgg_path)')
    parser.add_argument('-DTI3D', type=bool, help='Evaluation using DTDB I3D backbone')
    parser.add_argument('-clips_npy', type=str, help="start frames: clips [N, T, 3, H, W] (frame 0 is used) or [N, 3, H, W], in [-1, 1]")
    parser.add_argument('-i3d_path', type=str, help="checkpoint of the dynamic-texture I3D (I3D_16.pth.tar / I3D_32.pth.tar)")
    parser.add_argument('-vgg_path', type=str, help="torchvision vgg16 state_dict file (vgg16-397923af.pth) for -VGG; never downloaded")
    parser.add_argument('-seed', type=int, default=249, help="seed of the latent residuals (the reference fixes 249)")
    parser.add_argument('-embed_npy', type=str, help="[N,E] conditioning embeddings (one row per start frame)")
    parser.add_argument('-embed_seed', type=int, help="draw synthetic conditioning embeddings with this seed")
    parser.add_argument('-dec_mma', type=str, choices=["auto", "0", "1", "fp16"], default=None, help="decoder matrix-core mode")
    args = parser.parse_args(argv)
    for flag, why in NOT_BUILT.items():
        if getattr(args, flag):
            raise SystemExit(f"eval_diversity: -{flag} is not built: {why}")
    for flag, (paths, why) in NEEDS_PATHS.items():
        if getattr(args, flag) and not all(getattr(args, p) for p in paths):
            raise SystemExit(f"eval_diversity: -{flag} is not built: {why}")
    if not args.DTI3D and not args.VGG:
        raise SystemExit("eval_diversity: nothing to evaluate -- pass -DTI3D True or -VGG True -vgg_path FILE (the scores of this script that "
                         "are built)")
    if args.n_realiz < 2:
        parser.error("-n_realiz must be >= 2: the score compares the samples of one start frame with each other")
    if not args.clips_npy:
        raise SystemExit("eval_diversity: the data loaders are not built -- pass the start frames with -clips_npy FILE")
    return args


def main(argv=None):
    args = parse(argv)
    os.environ["HIP_VISIBLE_DEVICES"] = args.gpu   # the reference sets CUDA_VISIBLE_DEVICES
    import numpy as np
    import torch
    from get_model import Model
    from metrics.Diversity.I3D import compute_DTI3D_diversity
    from metrics.DTFVD import DTFVD_Score

    path_ds = f'{args.dataset}/{args.texture}/' if args.dataset == 'DTDB' else f'{args.dataset}'
    ckpt_path = f'./models/{path_ds}/stage2/' if not args.ckpt_path else args.ckpt_path
    model = Model(ckpt_path, args.seq_length, mma=args.dec_mma)
    x = torch.from_numpy(np.load(args.clips_npy).astype(np.float32))
    if x.dim() == 5:
        x = x[:, 0]
    if x.dim() != 4 or x.shape[1] != 3:
        raise SystemExit(f"-clips_npy: expected [N, T, 3, H, W] or [N, 3, H, W], got {tuple(x.shape)}")
    embeds = None
    if args.embed_npy:
        embeds = torch.from_numpy(np.load(args.embed_npy).astype(np.float32))
    elif args.embed_seed is not None:
        E = model.flow.flow.cond_channels - 3 * model.flow.cond_size
        embeds = torch.randn(x.size(0), E, generator=torch.Generator().manual_seed(args.embed_seed))
    torch.manual_seed(args.seed)

    seq_fake = []
    with torch.no_grad():
        for i in range(0, x.size(0), args.bs):
            emb = embeds[i:i + args.bs].cuda() if embeds is not None else None
            seq_fake.append(model.sample(x[i:i + args.bs].cuda().contiguous(), args.n_realiz, embed=emb))   # [b, R, T, 3, H, W] on the device
            model.check()
    seq1 = torch.cat(seq_fake)
    del model

    result = None
    if args.VGG:
        from metrics.Diversity.VGG import compute_vgg_diversity
        from stage2_cINN.AE.modules.vgg16 import vgg16
        result = compute_vgg_diversity(seq1, vgg16(path=args.vgg_path).cuda())
    if args.DTI3D:
        I3D = DTFVD_Score.load_model(length=32 if args.seq_length > 16 else 16, path=args.i3d_path).cuda()
        result = compute_DTI3D_diversity(seq1, I3D)
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
