#!/usr/bin/env python
"""Stage-1 reconstruction CLI: scores a stage-1 (VAE) checkpoint the way the reference's ``stage1_VAE/main.py`` validates it every epoch.

    python eval_reconstruction.py -gpu 0 -ckpt_path DIR/ -clips_npy real.npy [-bs 6] [-seed 42] [-data_range 2.0]
                                  [-vgg_path FILE -lpips_path FILE] [-per_frame OUT.npy]

``-ckpt_path`` is a stage-1 directory: ``config_stage1.yaml`` and the checkpoints as ``get_model.py`` reads them, ``best_PFVD_GEN.pth`` and
``best_PFVD_ENC.pth.tar`` (``-ckpt_decoder`` / ``-ckpt_encoder`` name others, without the suffix).  ``-clips_npy`` holds the real clips
``[N, T + 1, 3, H, W]`` float in [-1, 1] (the data loaders are out of scope); T is the decoder's clip length.  ``validator`` runs once:
every batch is encoded from frames 1.., decoded from frame 0 and scored on the device (csrc/i2v_recon.hip), and one line per key is
printed with the mean over the batches, as the reference's ``Logging.log`` gives it: Loss_L1, LPIPS, L_KL, PSNR, SSIM.  LPIPS needs
``-vgg_path`` (torchvision's vgg16 state_dict) and ``-lpips_path`` (``vgg.pth`` of the LPIPS release); without the two it is skipped, and the
script says so.  ``-data_range`` fixes the range of PSNR and SSIM (2.0 for frames in [-1, 1]); the default is the reference's, the range
of the data of each batch.  ``-per_frame OUT.npy`` writes the ``[2, T]`` PSNR and SSIM curves averaged over the clips."""
import argparse
import os
import sys


class Logging:
    """The part of the reference's ``utils.auxiliaries.Logging`` that validation uses: per-key lists, ``log()`` = their means."""

    def __init__(self, keys):
        self.keys = list(keys)
        self.reset()

    def reset(self):
        self.dic = {k: [] for k in self.keys}

    def append(self, loss_dic):
        for k in self.keys:
            self.dic[k].append(loss_dic[k])

    def get_iteration_mean(self, horizon=50):
        return [sum(v[-horizon:]) / max(len(v[-horizon:]), 1) for v in self.dic.values()]

    def log(self):
        return [sum(v) / len(v) for v in self.dic.values()]


def parse(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument('-gpu', type=str, required=True, help="Define GPU on which to run")
    parser.add_argument('-ckpt_path', type=str, help="stage-1 directory: config_stage1.yaml, best_PFVD_GEN.pth, best_PFVD_ENC.pth.tar")
    parser.add_argument('-clips_npy', type=str, help="real clips [N, T + 1, 3, H, W] in [-1, 1]")
    parser.add_argument('-bs', type=int, default=6, help='Batchsize')
    parser.add_argument('-seed', type=int, default=42, help="seed of the encoder's posterior draw (the reference's main seeds 42)")
    parser.add_argument('-data_range', type=float, default=None, help="fixed range of PSNR / SSIM (2.0 for [-1, 1]); default: from the data")
    parser.add_argument('-vgg_path', type=str, help="torchvision vgg16 state_dict file (vgg16-397923af.pth) for LPIPS; never downloaded")
    parser.add_argument('-lpips_path', type=str, help="lin weights of the LPIPS release (vgg.pth) for LPIPS; never downloaded")
    parser.add_argument('-per_frame', type=str, help="write the [2, T] per-frame PSNR and SSIM curves (mean over the clips) to this .npy")
    parser.add_argument('-ckpt_decoder', type=str, default="best_PFVD_GEN", help="decoder checkpoint name (+ .pth)")
    parser.add_argument('-ckpt_encoder', type=str, default="best_PFVD_ENC", help="encoder checkpoint name (+ .pth.tar)")
    args = parser.parse_args(argv)
    if not args.ckpt_path:
        raise SystemExit("eval_reconstruction: pass the stage-1 directory with -ckpt_path DIR (config_stage1.yaml and the two checkpoints)")
    if not args.clips_npy:
        raise SystemExit("eval_reconstruction: the data loaders are not built -- pass the real clips with -clips_npy FILE "
                         "([N, T + 1, 3, H, W] in [-1, 1])")
    if bool(args.vgg_path) != bool(args.lpips_path):
        raise SystemExit("eval_reconstruction: LPIPS needs both -vgg_path FILE (torchvision's vgg16 state_dict) and -lpips_path FILE (vgg.pth of "
                         "the LPIPS release); pass both, or neither to skip LPIPS")
    if args.data_range is not None and not args.data_range > 0:
        raise SystemExit(f"eval_reconstruction: -data_range must be positive, got {args.data_range}")
    if args.bs < 1:
        raise SystemExit(f"eval_reconstruction: -bs must be at least 1, got {args.bs}")
    return args


def main(argv=None):
    args = parse(argv)
    os.environ["HIP_VISIBLE_DEVICES"] = args.gpu   # the reference sets CUDA_VISIBLE_DEVICES
    import numpy as np
    import torch
    import i2v_config
    from stage1_VAE.main import validator
    from stage1_VAE.modules import decoder as net
    from stage1_VAE.modules.loss import Backward
    from stage1_VAE.modules.resnet3D import Encoder

    path = os.path.join(args.ckpt_path, "")
    config = i2v_config.load(path + "config_stage1.yaml")
    decoder = net.Generator(config.Decoder).cuda()
    decoder.load_state_dict(torch.load(path + args.ckpt_decoder + ".pth", map_location="cpu")["state_dict"])
    encoder = Encoder(dic=config.Encoder).cuda()
    encoder.load_state_dict(torch.load(path + args.ckpt_encoder + ".pth.tar", map_location="cpu")["state_dict"])
    _ = decoder.eval(), encoder.eval()

    clips = torch.from_numpy(np.load(args.clips_npy).astype(np.float32))
    if clips.dim() != 5 or clips.shape[2] != 3 or clips.shape[1] < 2:
        raise SystemExit(f"-clips_npy: expected [N, T + 1, 3, H, W], got {tuple(clips.shape)}")

    lpips = None
    if args.vgg_path:
        from stage2_cINN.AE.modules.LPIPS import LPIPS
        lpips = LPIPS(vgg_path=args.vgg_path, lin_path=args.lpips_path).cuda().eval()
    else:
        print("LPIPS is skipped: pass -vgg_path FILE -lpips_path FILE to score it (the weights are not part of this package)")
    backward = Backward(config, lpips=lpips)
    backward.data_range = args.data_range
    backward.per_image = bool(args.per_frame)
    keys = ["Loss_L1"] + (["LPIPS"] if lpips is not None else []) + ["L_KL", "PSNR", "SSIM"]
    logger = Logging(keys)
    loader = [{"seq": clips[i:i + args.bs]} for i in range(0, clips.size(0), args.bs)]

    torch.manual_seed(args.seed)
    validator(config, decoder, encoder, logger, 0, loader, backward)
    result = dict(zip(keys, logger.log()))
    for k, v in result.items():
        print(f"{k}: {v!r}")
    if args.per_frame:
        curves = torch.stack([torch.cat([c[i] for c in backward.curves], 0).mean(0) for i in (0, 1)])   # [2, T]: PSNR, SSIM
        np.save(args.per_frame, curves.cpu().numpy())
        print(f"per-frame PSNR and SSIM curves {tuple(curves.shape)} written to {args.per_frame}")
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
