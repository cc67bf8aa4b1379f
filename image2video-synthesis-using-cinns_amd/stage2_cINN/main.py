"""Mirror of the reference's ``stage2_cINN/main.py`` training entry points: ``trainer`` and ``validator`` with the reference's
signatures (main.py:20-71).  They work on any iterable of ``{"seq": [B, T, 3, H, W] (, "cond": [B, 3])}`` dicts; the frozen
motion encoder, the frozen conditioning embedder and the flow all run on HIP kernels, and with ``cINN.differentiable = True``
the loop ``loss.backward(); optimizer.step()`` trains the flow (csrc/i2v_flow_train.hip).  Data loaders, FVD evaluation and
CSV / wandb logging of the reference's ``main()`` are out of scope."""
import torch

try:
    from tqdm import tqdm
except ImportError:  # progress bars are optional
    tqdm = None


def _batches(data_loader, epoch):
    it = tqdm(data_loader, position=2) if tqdm is not None else data_loader
    if tqdm is not None:
        it.set_description(f"Epoch {epoch} || Loss: --- ")
    return it


def _flow_inputs(encoder, file_dict, opt):
    """seq -> (z [B, z_dim] from the frozen motion encoder on frames 1.., cond = [x0] or [x0, position])."""
    seq = file_dict["seq"].float().cuda()
    with torch.no_grad():
        post, *_ = encoder(seq[:, 1:].transpose(1, 2))
    cond = [seq[:, 0], file_dict["cond"]] if opt.Training["control"] else [seq[:, 0]]
    return post.reshape(post.size(0), -1).detach(), cond


def trainer(cINN, encoder, epoch, data_loader, logger, optimizer, loss_func, opt):
    """One epoch of flow training (main.py:20-46)."""
    cINN.train()
    logger.reset()
    data_iter = _batches(data_loader, epoch)
    for image_idx, file_dict in enumerate(data_iter):
        z, cond = _flow_inputs(encoder, file_dict, opt)
        gauss, logdet = cINN(z, cond)
        loss = loss_func(gauss, logdet, logger, mode="train")
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        if tqdm is not None and image_idx % 20 == 0:
            data_iter.set_description(f"Epoch {epoch} || Loss: {loss.item():.3f}")
    torch.cuda.empty_cache()


def validator(cINN, encoder, epoch, data_loader, logger, loss_func, opt):
    """One pass over the evaluation set without gradients (main.py:49-71)."""
    cINN.eval()
    logger.reset()
    data_iter = _batches(data_loader, epoch)
    with torch.no_grad():
        for image_idx, file_dict in enumerate(data_iter):
            z, cond = _flow_inputs(encoder, file_dict, opt)
            gauss, logdet = cINN(z, cond)
            loss = loss_func(gauss, logdet, logger, mode="eval")
            if tqdm is not None and image_idx % 20 == 0:
                data_iter.set_description(f"Epoch {epoch} || Loss: {loss.item():.3f}")
    torch.cuda.empty_cache()


def main(opt=None):
    raise SystemExit("stage2_cINN/main.py: the reference's main() needs its datasets and omegaconf, which do not "
                     "ship with this package; build the models (get_model.py), set cINN.differentiable = True and call "
                     "trainer(...) / validator(...) on your own iterable of {'seq': ...} batches, then "
                     "utils.auxiliaries.evaluate_FVD_prior(...) with metrics.PyTorch_FVD.FVD_logging.load_model() to pick the "
                     "checkpoint (README: Training the cINN, Evaluating FVD)")


if __name__ == "__main__":
    main()
