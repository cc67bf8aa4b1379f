#!/usr/bin/env python
"""Synthesis-quality CLI, mirror of the reference's ``eval_synthesis_quality.py``:

    python eval_synthesis_quality.py -gpu 0 -dataset DTDB -texture fire -ckpt_path DIR/ -clips_npy real.npy -DTFVD True [-seq_length 16] [-bs 6]

One video is sampled per real clip from its first frame, and the generated set is compared with the real one.  Built: ``-DTFVD`` (the
Frechet distance in the features of the dynamic-texture I3D, metrics/DTFVD, on the device; the length-32 network when
``-seq_length > 16``) and ``-LPIPS True -vgg_path FILE -lpips_path FILE`` (LPIPS on the native VGG-16 trunk over the compared frames
flattened to images, the reference's rule: the mean over floor(n / 10) batch means; the files are torchvision's vgg16 state_dict and the
``vgg.pth`` lin weights of the LPIPS release, nothing is downloaded) and ``-FID True -inception_path FILE`` (the Frechet distance in the
2048 features of the native FID Inception-v3, metrics/FID, over the compared frames flattened to images in batches of 50 -- the
reference's ``calculate_FID``, which drops the ragged last batch; the file is pytorch-fid's ``pt_inception-2015-12-05-6726825d.pth``); they
print the reference's lines.  ``-FVD`` (the TensorFlow FVD) exits with a "not built" message, and so do ``-LPIPS`` and ``-FID`` without
their paths.

The reference's data package is out of scope, so the real clips come from ``-clips_npy FILE``: ``[N, seq_length + 1, 3, H, W]`` float in
[-1, 1], what ``get_eval_loader(dataset, seq_length + 1, ...)`` yields.  Which real frames are compared keeps the reference's per-dataset
rule (``eval_synthesis_quality.py:45-58``): bair -- the conditioning frame in front of the generated ones, the last generated frame
dropped, against ``seq[:, :-1]``; iPER -- the conditioning frame in front of all generated frames against the whole ``seq``; every other
dataset (the dynamic textures) -- the generated frames alone against ``seq[:, :-1]``.  ``-i3d_path`` overrides the checkpoint of the
I3D (default: the reference's ``./models/DTI3D/...``), ``-seed`` the reference's fixed 249; ``-embed_npy`` / ``-embed_seed`` / ``-dec_mma``
as in ``generate_samples.py``.  The frames stay on the device; ``Model.synthesize`` is called where the reference calls ``Model.forward``
(the same frames without the batch slice of quirk Q3, which ``-bs`` <= ``-seq_length`` never reaches)."""
import argparse
import os
import sys

NOT_BUILT = {"FVD": "the TensorFlow FVD (metrics/FVD, a TF-hub I3D) is not built; the Kinetics FVD on the device is "
                    "metrics/PyTorch_FVD (utils.auxiliaries.evaluate_FVD_prior)"}


NEEDS_PATHS = {"LPIPS": (("vgg_path", "lpips_path"), "LPIPS needs the VGG-16 ImageNet weights and the LPIPS lin weights, which are not part of this "
                                                     "package: pass -vgg_path FILE (torchvision's vgg16 state_dict) and -lpips_path FILE "
                                                     "(vgg.pth of the LPIPS release)"),
               "FID": (("inception_path",), "FID needs the FID Inception-v3 weights, which are not part of this package and are never downloaded: "
                                            "pass -inception_path FILE (pytorch-fid's pt_inception-2015-12-05-6726825d.pth)")}


def parse(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument('-gpu', type=str, required=True, help="Define GPU on which to run")
    parser.add_argument('-dataset', type=str)
    parser.add_argument('-texture', type=str, required=False, help='Specify texture when using DTDB')
    parser.add_argument('-ckpt_path', type=str, required=False, help="Specify path if outside of repo for chkpt")
    parser.add_argument('-data_path', type=str, required=False, help="(reference flag; the data package is not built, use -clips_npy)")
    parser.add_argument('-seq_length', type=int, default=16)
    parser.add_argument('-bs', type=int, default=6, help='Batchsize')
    parser.add_argument('-FID', type=bool)
    parser.add_argument('-FVD', type=bool)
    parser.add_argument('-DTFVD', type=bool)
    parser.add_argument('-LPIPS', type=bool)
    parser.add_argument('-clips_npy', type=str, help="real clips [N, seq_length + 1, 3, H, W] in [-1, 1]")
    parser.add_argument('-i3d_path', type=str, help="checkpoint of the dynamic-texture I3D (I3D_16.pth.tar / I3D_32.pth.tar)")
    parser.add_argument('-vgg_path', type=str, help="torchvision vgg16 state_dict file (vgg16-397923af.pth) for -LPIPS; never downloaded")
    parser.add_argument('-lpips_path', type=str, help="lin weights of the LPIPS release (vgg.pth: lin{k}.model.1.weight) for -LPIPS; never downloaded")
    parser.add_argument('-inception_path', type=str, help="FID Inception state_dict file (pt_inception-2015-12-05-6726825d.pth) for -FID; never downloaded")
    parser.add_argument('-seed', type=int, default=249, help="seed of the latent residuals (the reference fixes 249)")
    parser.add_argument('-embed_npy', type=str, help="[N,E] conditioning embeddings (one row per clip)")
    parser.add_argument('-embed_seed', type=int, help="draw synthetic conditioning embeddings with this seed")
    parser.add_argument('-dec_mma', type=str, choices=["auto", "0", "1", "fp16"], default=None, help="decoder matrix-core mode")
    args = parser.parse_args(argv)
    for flag, why in NOT_BUILT.items():
        if getattr(args, flag):
            raise SystemExit(f"eval_synthesis_quality: -{flag} is not built: {why}")
    for flag, (paths, why) in NEEDS_PATHS.items():
        if getattr(args, flag) and not all(getattr(args, p) for p in paths):
            raise SystemExit(f"eval_synthesis_quality: -{flag} is not built: {why}")
    if not args.DTFVD and not args.LPIPS and not args.FID:
        raise SystemExit("eval_synthesis_quality: nothing to evaluate -- pass -DTFVD True or -LPIPS True -vgg_path FILE -lpips_path FILE or "
                         "-FID True -inception_path FILE (the metrics of this script that are built)")
    if not args.clips_npy:
        raise SystemExit("eval_synthesis_quality: the data loaders are not built -- pass the real clips with -clips_npy FILE "
                         "([N, seq_length + 1, 3, H, W] in [-1, 1])")
    return args


def compared_frames(dataset, seq, seq_gen):
    """The reference's per-dataset rule: (generated, real) as they enter the metric."""
    import torch
    if dataset == 'bair':
        return torch.cat((seq[:, :1], seq_gen[:, :-1]), dim=1), seq[:, :-1]
    if dataset == 'iPER':
        return torch.cat((seq[:, :1], seq_gen), dim=1), seq
    return seq_gen, seq[:, :-1]


def main(argv=None):
    args = parse(argv)
    os.environ["HIP_VISIBLE_DEVICES"] = args.gpu   # the reference sets CUDA_VISIBLE_DEVICES
    import numpy as np
    import torch
    from get_model import Model
    from metrics.DTFVD import DTFVD_Score

    path_ds = f'{args.dataset}/{args.texture}/' if args.dataset == 'DTDB' else f'{args.dataset}'
    ckpt_path = f'./models/{path_ds}/stage2/' if not args.ckpt_path else args.ckpt_path
    model = Model(ckpt_path, args.seq_length, mma=args.dec_mma)
    clips = torch.from_numpy(np.load(args.clips_npy).astype(np.float32))
    if clips.dim() != 5 or clips.shape[2] != 3 or clips.shape[1] != args.seq_length + 1:
        raise SystemExit(f"-clips_npy: expected [N, {args.seq_length + 1}, 3, H, W], got {tuple(clips.shape)}")
    embeds = None
    if args.embed_npy:
        embeds = torch.from_numpy(np.load(args.embed_npy).astype(np.float32))
    elif args.embed_seed is not None:
        E = model.flow.flow.cond_channels - 3 * model.flow.cond_size
        embeds = torch.randn(clips.size(0), E, generator=torch.Generator().manual_seed(args.embed_seed))
    torch.manual_seed(args.seed)

    seq_real, seq_fake = [], []
    with torch.no_grad():
        for i in range(0, clips.size(0), args.bs):
            seq = clips[i:i + args.bs].cuda()
            emb = embeds[i:i + args.bs].cuda() if embeds is not None else None
            seq_gen = model.synthesize(seq[:, 0].contiguous(), embed=emb)
            model.check()
            fake, real = compared_frames(args.dataset, seq, seq_gen)
            seq_fake.append(fake)
            seq_real.append(real)
    seq1, seq2 = torch.cat(seq_fake, 0), torch.cat(seq_real, 0)   # on the device
    del model
    assert seq2.shape == seq1.shape, (tuple(seq1.shape), tuple(seq2.shape))

    result = None
    if args.FID or args.LPIPS:
        pd_imgs = seq1.reshape(-1, *seq1.shape[2:])
        gt_imgs = seq2.reshape(-1, *seq2.shape[2:])
    if args.FID:
        from metrics.FID.FID_Score import calculate_FID
        from metrics.FID.inception import InceptionV3
        print('Evaluate FID')
        inception = InceptionV3(path=args.inception_path)   # normalize_input=False as in the reference: the frames enter in [-1, 1]
        batch_size = 50
        FID, _ = calculate_FID(inception, pd_imgs, gt_imgs, batch_size, 2048)
        del inception
        torch.cuda.empty_cache()
        print(f'FID score of {FID}')
        result = FID
    if args.LPIPS:
        from stage2_cINN.AE.modules.LPIPS import LPIPS, lpips_score
        print('Evaluate LPIPS')
        lpips_vgg = LPIPS(vgg_path=args.vgg_path, lin_path=args.lpips_path).cuda().eval()
        result = lpips_score(lpips_vgg, pd_imgs, gt_imgs)
        del lpips_vgg
        print(f'LPIPS score of {result}')
    if args.DTFVD:
        print('Evaluate DTFVD')
        batch_size = 40
        if args.seq_length > 16:
            I3D = DTFVD_Score.load_model(length=32, path=args.i3d_path).cuda()
            DTFVD = DTFVD_Score.calculate_FVD32(I3D, seq1, seq2, batch_size, True)
        else:
            I3D = DTFVD_Score.load_model(length=16, path=args.i3d_path).cuda()
            DTFVD = DTFVD_Score.calculate_FVD(I3D, seq1, seq2, batch_size, True)
        print(f'DTFVD score of {DTFVD}')
        result = DTFVD
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
