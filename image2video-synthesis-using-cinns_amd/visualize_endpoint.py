#!/usr/bin/env python
"""Endpoint-controlled sampling CLI, mirror of the reference's ``visualize_endpoint.py``:

    python visualize_endpoint.py -gpu 0 -img_path DIR/ -cond_npy POS.npy [-ckpt_path DIR/] [-n_samples 15] [-n_realiz 8]
                                 [-seq_length 16] [-bs 6]

For each of the first ``n_samples`` start frames it samples ``n_realiz`` videos of the endpoint-controlled model
(``Training.control``) and writes ``endpoint_{i}.gif`` (the realizations side by side, ``convert_seq2gif``) and ``endpoint_{i}.png``
(their last frames, tiled as ``torchvision.utils.save_image(..., normalize=True)`` tiles them: 8 per row, padding 2, min-max over
the tensor).  There is no dataset loader: the start frames come from the images under ``-img_path`` (sorted, as in
``generate_samples.py``), the endpoint positions from ``-cond_npy`` ([N, 3] in [0, 1]: the bins ``INN.embed_pos`` takes).
``-embed_npy`` / ``-embed_seed`` / ``-seed`` / ``-out_path`` work as in ``generate_samples.py``.

The residuals are drawn in the reference's order -- realization outer, batch inner (one ``randn(batch, z_dim)`` per model call) --
so a seeded run draws the reference's latents; the videos are then decoded through ``Model.sample`` with those residuals, which
embeds and runs the decoder's SPADE branches once per start frame instead of once per realization.
"""
import argparse
import math
import os

import numpy as np
import torch

from generate_samples import img_suffix, load_images, save_gif


def main(argv=None):
    import glob
    parser = argparse.ArgumentParser()
    parser.add_argument("-gpu", type=str, required=True, help="Define GPU on which to run")
    parser.add_argument("-dataset", type=str, default="bair", help="Specify dataset (the reference supports bair only)")
    parser.add_argument("-ckpt_path", type=str, required=False, help="If ckpt outside of repo")
    parser.add_argument("-seq_length", type=int, default=16)
    parser.add_argument("-n_samples", type=int, default=15, help="How many start frames (test instances) are visualised")
    parser.add_argument("-n_realiz", type=int, default=8, help="How many realizations generated for each test instance")
    parser.add_argument("-bs", type=int, default=6, help="Batchsize")
    parser.add_argument("-img_path", type=str, required=True, help="directory of start-frame images")
    parser.add_argument("-cond_npy", type=str, required=True, help="[N,3] endpoint positions in [0,1], one row per image")
    parser.add_argument("-embed_npy", type=str, help="[N,E] conditioning embeddings (one row per image)")
    parser.add_argument("-embed_seed", type=int, help="draw synthetic conditioning embeddings with this seed")
    parser.add_argument("-seed", type=int, help="seed the CPU generator the latent residuals are drawn from, right before sampling")
    parser.add_argument("-out_path", type=str, help="override ./assets/results/bair_endpoint/")
    parser.add_argument("-dec_mma", type=str, choices=["auto", "0", "1", "fp16"], default=None, help="decoder matrix-core mode")
    parser.add_argument("-dev_out", action="store_true",
                        help="quantise and tile the GIF frames on the GPU (i2v_pipeline.FrameSink): the same bytes, a quarter of the transfer")
    args = parser.parse_args(argv)
    if args.n_realiz < 1 or args.n_samples < 1 or args.bs < 1:
        parser.error("-n_realiz, -n_samples and -bs must be >= 1")
    os.environ["HIP_VISIBLE_DEVICES"] = args.gpu

    from get_model import Model
    from utils import auxiliaries as aux

    ckpt_path = f"./models/{args.dataset}/stage2_control/" if not args.ckpt_path else args.ckpt_path
    img_list = []
    for suffix in img_suffix:
        img_list.extend(sorted(glob.glob(args.img_path + f"*.{suffix}")))
    if not img_list:
        raise SystemExit(f"no images found under {args.img_path}")
    model = Model(ckpt_path, args.seq_length, mma=args.dec_mma)
    if not model.flow.control:
        raise SystemExit("visualize_endpoint needs an endpoint-controlled checkpoint (Training.control)")
    imgs = load_images(img_list, model.config.Data["img_size"])
    cond = torch.from_numpy(np.load(args.cond_npy).astype(np.float32))
    if cond.dim() != 2 or cond.shape[1] != 3 or cond.shape[0] < imgs.size(0):
        raise SystemExit(f"-cond_npy: expected [N>={imgs.size(0)}, 3] positions, got {tuple(cond.shape)}")
    E = model.flow.flow.cond_channels - 3 * model.flow.cond_size
    if args.embed_npy:
        embeds = torch.from_numpy(np.load(args.embed_npy).astype(np.float32))
    elif args.embed_seed is not None:
        embeds = torch.randn(imgs.size(0), E, generator=torch.Generator().manual_seed(args.embed_seed))
    else:
        embeds = None

    # the batches the reference's loop visits: full batches until n_samples frames are covered
    bs, K = args.bs, args.n_realiz
    batches, n = [], 0
    for i in range(math.ceil(imgs.size(0) / bs)):
        batches.append((i * bs, min((i + 1) * bs, imgs.size(0))))
        n += batches[-1][1] - batches[-1][0]
        if n >= args.n_samples:
            break
    if args.seed is not None:
        torch.manual_seed(args.seed)
    # residual draws in the reference's order (visualize_endpoint.py:37-45): realization outer, batch inner
    res = [[torch.randn(b1 - b0, model.z_dim) for (b0, b1) in batches] for _ in range(K)]
    if args.dev_out:
        return _main_dev_out(args, model, imgs, cond, embeds, batches, res)
    videos = []
    with torch.no_grad():
        for j, (b0, b1) in enumerate(batches):
            r = torch.stack([res[k][j] for k in range(K)], 1)   # [b, K, z_dim]: realization k of frame f
            emb = embeds[b0:b1].cuda() if embeds is not None else None
            videos.append(model.sample(imgs[b0:b1].cuda(), K, cond=cond[b0:b1], residual=r.cuda(), embed=emb).cpu())
            model.check()
    videos = torch.cat(videos)[:args.n_samples]   # [N, K, T, 3, H, W]

    from PIL import Image
    save_path = args.out_path or "./assets/results/bair_endpoint/"
    os.makedirs(os.path.dirname(save_path), exist_ok=True)
    for idx, vid in enumerate(videos):
        save_gif(save_path + f"endpoint_{idx}.gif", aux.convert_seq2gif(vid), fps=3)
        Image.fromarray(aux.tile_images(vid[:, -1])).save(save_path + f"endpoint_{idx}.png")
    print(f"Animations saved in {save_path}")


def _main_dev_out(args, model, imgs, cond, embeds, batches, res):
    """``-dev_out``: every start frame's strip of K realizations (its own peak, as ``convert_seq2gif`` per image) goes through a
    ``FrameSink`` while the batch's videos stay on the device; only the last frames (``vid[:, -1]``, a sixteenth of the data) are copied
    as floats, for the ``tile_images`` PNG, whose host code is unchanged."""
    from PIL import Image
    from i2v_pipeline import FrameSink, FrameSinkBudgetError
    from utils import auxiliaries as aux
    K = args.n_realiz
    save_path = args.out_path or "./assets/results/bair_endpoint/"
    os.makedirs(os.path.dirname(save_path), exist_ok=True)
    sink, idx = FrameSink("peak"), 0
    with torch.no_grad():
        for j, (b0, b1) in enumerate(batches):
            r = torch.stack([res[k][j] for k in range(K)], 1)   # [b, K, z_dim]: realization k of frame f
            emb = embeds[b0:b1].cuda() if embeds is not None else None
            vids = model.sample(imgs[b0:b1].cuda(), K, cond=cond[b0:b1], residual=r.cuda(), embed=emb)   # [b, K, T, 3, H, W], device
            model.check()
            for vid in vids[:max(0, args.n_samples - idx)]:
                try:
                    sink.add(vid)
                    sink.finish()
                    gif = sink.result()
                except FrameSinkBudgetError as e:
                    print(f"-dev_out: {e}")
                    gif = aux.convert_seq2gif(vid).astype(np.uint8)
                save_gif(save_path + f"endpoint_{idx}.gif", gif, fps=3)
                Image.fromarray(aux.tile_images(vid[:, -1])).save(save_path + f"endpoint_{idx}.png")
                idx += 1
    print(f"Animations saved in {save_path}")


if __name__ == "__main__":
    main()
