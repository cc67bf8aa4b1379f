"""Mirror of the reference's ``stage1_VAE/main.py`` entry points.  ``validator`` (main.py:58-87) is built, with the reference's signature:
it runs ``Backward.eval`` over any iterable of ``{"seq": [B, T + 1, 3, H, W]}`` dicts -- the motion encoder, the decoder, LPIPS and the
reconstruction metrics all run on HIP kernels -- and fills ``logger`` with Loss_L1, (LPIPS,) L_KL, PSNR and SSIM per batch.  The video plot
(``aux.plot_vid``) and wandb are left out.  ``trainer`` and ``main`` exit with a message: stage-1 training is not built."""
import torch

try:
    from tqdm import tqdm
except ImportError:  # progress bars are optional
    tqdm = None

NOT_BUILT = ("stage-1 training is not built: of the backward passes Backward.forward needs, those of the motion encoder and of the two "
             "discriminators exist, the decoder's and the gradient penalty's double backward do not (stage1_VAE/modules/loss.py); validation "
             "is -- build the models (stage1_VAE.modules.decoder.Generator, "
             "resnet3D.Encoder), a Backward(opt, lpips) and call validator(...) on your own iterable of {'seq': ...} batches, or run "
             "eval_reconstruction.py on a stage-1 checkpoint directory (README: Scoring a stage-1 checkpoint)")


def trainer(opt, network, enc, disc_t, disc_s, logger, epoch, data_loader, optimizer, backward):
    raise SystemExit("stage1_VAE/main.py: trainer: " + NOT_BUILT)


def validator(opt, network, enc, logger, epoch, data_loader, backward):
    """One pass over the evaluation set (main.py:58-87); returns the last batch's ``[seq_gen, seq_orig]`` (on the device)."""
    _ = network.eval()
    logger.reset()
    data_iter = tqdm(data_loader, position=2, ascii=True) if tqdm is not None else data_loader
    if tqdm is not None:
        data_iter.set_description('Epoch {} | Eval | L1: --- | Percep: ---'.format(epoch))
    verbose_idx = (opt.Training['verbose_idx'] if opt is not None and getattr(opt, "Training", None) else None) or 0
    sequences = None
    with torch.no_grad():
        for image_idx, file_dict in enumerate(data_iter):
            seq = file_dict["seq"].float().cuda()   # [B, T + 1, C, H, W]
            sequences = backward.eval(network, enc, seq, logger)
            if tqdm is not None and hasattr(logger, "get_iteration_mean") and (verbose_idx and image_idx % verbose_idx == 0 and image_idx
                                                                                  or image_idx == 5):
                loss_log = logger.get_iteration_mean(10)
                data_iter.set_description('Epoch {} | Eval | L1: {:.3f} | Percep: {:.3f}'.format(epoch, loss_log[0], loss_log[1]))
    torch.cuda.empty_cache()
    return sequences


def main(opt=None):
    raise SystemExit("stage1_VAE/main.py: " + NOT_BUILT)


if __name__ == "__main__":
    main()
