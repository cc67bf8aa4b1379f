"""The reconstruction-metric kernels (csrc/i2v_recon.hip) and the stage-1 validation surface on the GPU against the float64 oracle of
tests/recon_common.py, at the gate derived there (measured maxima: profiles/recon_gate.md).  Shapes: one valid SSIM position, rows and
columns that are no multiple of a tile, a shape that crosses a tile edge in both directions, several tiles per plane, and
the strided view ``seq[:, 1:]``.  Then KL, ``Backward.eval`` end to end on the small seeded encoder and the nf-8 decoder, and the CLI."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import encoder_cfgs as ec
import i2v_native
import i2v_synth as synth
import recon_common as rc
import vgg_common as vc
from conftest import PKG, load_golden
from i2v_native import I2VError
from stage1_VAE import main as stage1_main
from stage1_VAE.modules import loss as loss_mod

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 3, 11, 11), (1, 2, 3, 11, 40), (3, 1, 1, 12, 75), (2, 2, 3, 43, 33), (1, 5, 3, 64, 64), (1, 2, 3, 128, 128)]
KL_CASES = [(1, 1), (3, 64), (130, 64)]
ENCODER = "nodown_l0"   # 64 x 64, 16 frames, z_dim 64: what the nf-8 decoder of model_nf8 returns


def T(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    i2v_native.lib()  # fails loudly if libi2v_hip.so is missing
    torch.set_grad_enabled(False)


@functools.lru_cache(maxsize=None)
def case(shape, data_range=None):
    """[(name, real, generated, oracle result)] of a shape: computed once, shared, never written to."""
    return [(name, real, gen, rc.oracle(real, gen, data_range)) for name, real, gen in rc.families(100 + shape[-1], shape)]


def _scalars(s):
    s = s.cpu()
    return {"l1": s[0], "mse": s[1], "psnr": s[2], "ssim": s[3]}


@pytest.mark.parametrize("shape", SHAPES)
def test_scalars_and_rows_vs_oracle(shape):
    for name, real, gen, ref in case(shape):
        s, rows, rng = i2v_native.recon_stats(real.cuda(), gen.cuda())
        print(f"{shape} {name}")
        res = rc.check_scalars(_scalars(s), ref)
        rows_ok = rc.gate("per-image rows", rows, ref["per_image"], ref["bound_per_image"])[0]
        assert rc.all_ok(res) and rows_ok, (shape, name)
        assert float(s[4]) == ref["terms"] == shape[0] * shape[1] * shape[2] * (shape[3] - 10) * (shape[4] - 10)
        want = torch.stack([real.min(), real.max(), gen.min(), gen.max()]).double()
        assert torch.equal(rng.cpu(), want) and torch.equal(i2v_native.recon_range(real.cuda(), gen.cuda()).cpu(), want)
        # the scalars ARE the rows summed in index order
        tot = [0.0, 0.0, 0.0]
        for row in rows.cpu().tolist():
            tot = [a + b for a, b in zip(tot, row)]
        n = real.numel()
        assert float(s[0]) == tot[0] / n and float(s[1]) == tot[1] / n and float(s[3]) == tot[2] / ref["terms"]


@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_range_public_surface_and_curves(shape):
    for name, real, gen, ref in case(shape, 2.0):
        m = loss_mod.recon_metrics(real.cuda(), gen.cuda(), data_range=2.0, per_image=True)
        assert all(m[k].dim() == 0 and m[k].is_cuda and m[k].dtype == torch.float64 for k in rc.SCALARS)
        print(f"{shape} data_range 2.0 {name}")
        assert rc.all_ok(rc.check_scalars(m, ref))
        psnr_i, ssim_i = rc.per_image_curves(ref)
        assert tuple(m["psnr_per_image"].shape) == tuple(m["ssim_per_image"].shape) == shape[:2]
        b_ssim = ref["bound_per_image"][:, 2] / (shape[2] * (shape[3] - 10) * (shape[4] - 10)) + 2 * rc.U * ssim_i.abs()
        b_psnr = (10 / np.log(10)) * (ref["bound_per_image"][:, 1] / ref["per_image"][:, 1] + 8 * rc.U * (1 + psnr_i.abs()))
        assert rc.gate("ssim per image", m["ssim_per_image"], ssim_i, b_ssim)[0] and rc.gate("psnr per image", m["psnr_per_image"], psnr_i, b_psnr)[0]
    name, real, gen, ref = case(shape)[1]
    flat = (real.cuda().reshape(-1, *shape[2:]), gen.cuda().reshape(-1, *shape[2:]))          # the reference's call: [N, C, H, W]
    got = {"psnr": loss_mod.psnr(*flat), "ssim": loss_mod.ssim(*flat), "l1": ref["l1"], "mse": ref["mse"]}
    assert rc.all_ok(rc.check_scalars(got, ref, what="psnr(), ssim()"))
    assert torch.equal(loss_mod.recon_metrics(real.cuda(), gen.cuda())["ssim"], got["ssim"])


def test_identical_inputs_and_repeatability():
    for shape in ((1, 1, 3, 11, 11), (2, 2, 3, 43, 33), (1, 2, 3, 64, 64)):
        for name, real, gen, _ in case(shape):
            x = real.cuda()
            for dr in (None, 2.0):
                s, rows, _ = i2v_native.recon_stats(x, x.clone(), dr)
                assert float(s[3]) == 1.0 and float(s[2]) == float("inf") and float(s[0]) == 0.0 and float(s[1]) == 0.0, (shape, name, s)
                assert torch.equal(rows[:, 2], torch.full_like(rows[:, 2], shape[2] * (shape[3] - 10) * (shape[4] - 10)))
            a, b = i2v_native.recon_stats(x, gen.cuda()), i2v_native.recon_stats(x, gen.cuda())
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_strided_view_is_read_in_place_bit_for_bit():
    real, gen = rc.pair(77, (2, 5, 3, 16, 23), 0.1)
    seq, out = real.cuda(), gen.cuda()
    view, gview = seq[:, 1:], out[:, :4]
    assert not view.is_contiguous() and i2v_native._recon_view(view, "test")[0].data_ptr() == view.data_ptr()     # no copy
    for dr in (None, 2.0):
        a = i2v_native.recon_stats(view, gview, dr)
        b = i2v_native.recon_stats(view.contiguous(), gview.contiguous(), dr)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (dr is not None or torch.equal(a[2], b[2]))
    ref = rc.oracle(view.cpu().contiguous(), gview.cpu().contiguous())
    assert rc.all_ok(rc.check_scalars(_scalars(i2v_native.recon_stats(view, gview)[0]), ref, what="strided"))


def test_refusals():
    x = torch.zeros(1, 2, 3, 10, 16, device="cuda")
    with pytest.raises(I2VError, match="11 x 11"):
        i2v_native.recon_stats(x, x)
    with pytest.raises(I2VError, match="11 x 11"):
        loss_mod.ssim(x.transpose(3, 4).contiguous(), x.transpose(3, 4).contiguous(), data_range=2.0)
    y = torch.zeros(1, 2, 3, 16, 16, device="cuda")
    with pytest.raises(I2VError, match="do not match"):
        i2v_native.recon_stats(y, y[:, :1])
    with pytest.raises(I2VError, match="float32"):
        i2v_native.recon_stats(y.double(), y.double())
    s, _, _ = i2v_native.recon_stats(y, y)                       # constant frames: R = 0, 0 / 0 -- NaN as in the reference, not an error
    assert bool(torch.isnan(s[3]))


@pytest.mark.parametrize("b,d", KL_CASES)
def test_kl(b, d):
    g = torch.Generator().manual_seed(600 + b)
    mu, lv = torch.randn(b, d, generator=g), 0.5 * torch.randn(b, d, generator=g) - 0.3
    want, bound = rc.kl_oracle(mu, lv)
    got = loss_mod.KL(mu.cuda(), lv.cuda())
    assert got.dim() == 0 and got.dtype == torch.float64 and float(bound / want.abs()) < rc.REL_CEILING
    assert rc.gate(f"KL {b} x {d}", got, want, bound)[0]
    assert torch.equal(got, loss_mod.KL(mu.cuda(), lv.cuda()))
    assert torch.equal(got, loss_mod.KL(mu.cuda().view(b, d, 1, 1), lv.cuda().view(b, d, 1, 1)))     # the encoder's [B, z, 1, 1] heads


# ---------------------------------------------------------------------------------------------------------------- Backward.eval, the CLI

def _decoder_cfg():
    _, meta = load_golden("model_nf8")
    return meta, {"channel_factor": meta["synth_dec"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"], "upsample_t": meta["upsample_t"],
                  "spectral_norm": True}


def _encoder_cfg():
    c = ec.CASES[ENCODER]
    a = c["synth"]
    return c, {"res_type_encoder": "resnet18", "use_max_pool": False, "z_dim": a["z_dim"], "channels": a["channels"], "stride_s": a["stride_s"],
               "stride_t": c["stride_t"]}


@functools.lru_cache(maxsize=None)
def _models():
    from stage1_VAE.modules.decoder import Generator
    from stage1_VAE.modules.resnet3D import Encoder
    meta, dcfg = _decoder_cfg()
    gen = Generator(dcfg)
    gen.load_state_dict(T(synth.decoder_state_dict(**meta["synth_dec"])))
    c, ecfg = _encoder_cfg()
    enc = Encoder(ecfg)
    enc.load_state_dict(T(synth.encoder3d_state_dict(**c["synth"])))
    return gen.cuda().eval(), enc.cuda().eval()


@functools.lru_cache(maxsize=None)
def _lpips(tmp):
    from stage2_cINN.AE.modules.LPIPS import LPIPS
    vgg_path, lin_path = os.path.join(tmp, "vgg16.pth"), os.path.join(tmp, "vgg.pth")
    vc.save_torchvision_file(vgg_path, 41)
    vc.save_lin_file(lin_path, 42)
    return LPIPS(vgg_path=vgg_path, lin_path=lin_path).cuda().eval(), vgg_path, lin_path


def _clips(n, seed=23):
    """[n, 17, 3, 64, 64] in (-1, 1): a smooth clip per sample."""
    return rc.smooth_field(seed, (n, 17, 3, 64, 64)).float()


class ListLogger:
    def __init__(self):
        self.rows = []

    def reset(self):
        self.rows = []

    def append(self, d):
        self.rows.append(d)


def _check_eval_row(row, seq_gen, seq_orig, enc, lp):
    ref = rc.oracle(seq_orig.cpu().contiguous(), seq_gen.cpu())
    got = {"l1": row["Loss_L1"], "mse": ref["mse"], "psnr": row["PSNR"], "ssim": row["SSIM"]}
    assert rc.all_ok(rc.check_scalars(got, ref, what="Backward.eval"))
    _, mu, logvar = enc(seq_orig.transpose(1, 2))
    want, bound = rc.kl_oracle(mu.cpu().reshape(mu.size(0), -1), logvar.cpu().reshape(mu.size(0), -1))
    assert rc.gate("Backward.eval L_KL", row["L_KL"], want, bound)[0]
    if lp is not None:
        flat = lambda x: x.reshape(-1, *x.shape[2:])   # noqa: E731
        assert row["LPIPS"] == pytest.approx(float(lp(flat(seq_orig), flat(seq_gen)).mean()), rel=1e-6)


def test_backward_eval_end_to_end(tmp_path_factory):
    gen, enc = _models()
    lp = _lpips(str(tmp_path_factory.mktemp("lpips")))[0]
    seq = _clips(2).cuda()
    logger = ListLogger()
    bw = loss_mod.Backward(None, lpips=lp)
    torch.manual_seed(3)
    seq_gen, seq_orig = bw.eval(gen, enc, seq, logger)
    assert seq_gen.is_cuda and seq_orig.is_cuda and seq_gen.shape == seq_orig.shape == (2, 16, 3, 64, 64) and seq_orig.data_ptr() == seq[:, 1:].data_ptr()
    assert len(logger.rows) == 1 and list(logger.rows[0]) == ["Loss_L1", "LPIPS", "L_KL", "PSNR", "SSIM"]
    assert all(isinstance(v, float) for v in logger.rows[0].values())
    _check_eval_row(logger.rows[0], seq_gen, seq_orig, enc, lp)
    torch.manual_seed(3)
    again = ListLogger()
    bw.eval(gen, enc, seq, again)
    assert again.rows == logger.rows                                                     # same seed, same bits
    plain = ListLogger()
    torch.manual_seed(3)
    loss_mod.Backward(None).eval(gen, enc, seq, plain)
    assert list(plain.rows[0]) == ["Loss_L1", "L_KL", "PSNR", "SSIM"] and all(plain.rows[0][k] == logger.rows[0][k] for k in plain.rows[0])


def test_validator_and_cli_print_the_same_numbers(tmp_path_factory):
    import yaml
    gen, enc = _models()
    tmp = tmp_path_factory.mktemp("stage1")
    lp, vgg_path, lin_path = _lpips(str(tmp_path_factory.mktemp("lpips_cli")))
    meta, dcfg = _decoder_cfg()
    c, ecfg = _encoder_cfg()
    with open(tmp / "config_stage1.yaml", "w") as f:
        yaml.safe_dump({"Decoder": dcfg, "Encoder": ecfg, "Training": {"verbose_idx": 20}}, f)
    torch.save({"state_dict": T(synth.decoder_state_dict(**meta["synth_dec"]))}, tmp / "best_PFVD_GEN.pth")
    torch.save({"state_dict": T(synth.encoder3d_state_dict(**c["synth"]))}, tmp / "best_PFVD_ENC.pth.tar")
    clips = _clips(3, seed=29)
    np.save(tmp / "clips.npy", clips.numpy())

    # in process: validator over batches of 2 and 1, per-frame curves on
    from eval_reconstruction import Logging
    keys = ["Loss_L1", "LPIPS", "L_KL", "PSNR", "SSIM"]
    logger = Logging(keys)
    bw = loss_mod.Backward(None, lpips=lp)
    bw.per_image = True
    torch.manual_seed(42)
    last = stage1_main.validator(None, gen, enc, logger, 0, [{"seq": clips[:2]}, {"seq": clips[2:]}], bw)
    assert [len(v) for v in logger.dic.values()] == [2] * 5 and last[0].shape == (1, 16, 3, 64, 64)
    want = dict(zip(keys, logger.log()))
    curves = torch.stack([torch.cat([cv[i] for cv in bw.curves], 0).mean(0) for i in (0, 1)]).cpu().numpy()
    assert curves.shape == (2, 16)

    cmd = [sys.executable, os.path.join(PKG, "eval_reconstruction.py"), "-gpu", "0", "-ckpt_path", str(tmp), "-clips_npy", str(tmp / "clips.npy"), "-bs", "2",
           "-vgg_path", vgg_path, "-lpips_path", lin_path, "-per_frame", str(tmp / "curves.npy")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=PKG, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {k: float(v) for k, v in re.findall(r"^(\w+): ([-+.\deinf]+)$", r.stdout, flags=re.M)}
    print(r.stdout)
    assert list(got) == keys
    for k in keys:
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    assert np.allclose(np.load(tmp / "curves.npy"), curves, rtol=1e-12, atol=0)

    r = subprocess.run(cmd[:10], capture_output=True, text=True, cwd=PKG, timeout=300)          # without the two LPIPS paths
    assert r.returncode == 0, r.stderr[-2000:]
    assert "LPIPS is skipped" in r.stdout and not re.search(r"^LPIPS: ", r.stdout, flags=re.M)
    got2 = {k: float(v) for k, v in re.findall(r"^(\w+): ([-+.\deinf]+)$", r.stdout, flags=re.M)}
    assert list(got2) == ["Loss_L1", "L_KL", "PSNR", "SSIM"] and all(got2[k] == got[k] for k in got2)
