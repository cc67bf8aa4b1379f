"""CPU-side checks of the stage-1 validation surface: the float64 oracle of tests/recon_common.py against itself in pytorch_lightning's
pad-and-crop order, the deliberate errors the gate has to reject, KL / hinge_loss / fmap_loss against the fixture written from the reference's
own functions, the new native symbols, the refusals without a GPU and the CLI's argument errors."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest
import torch

import i2v_native
import recon_common as rc
from conftest import GOLDEN, PKG, REPO, load_golden
from stage1_VAE import main as stage1_main
from stage1_VAE.modules import loss as loss_mod

NEW_SYMBOLS = ["i2v_recon_workspace_bytes", "i2v_recon_range", "i2v_recon_stats", "i2v_kl_normal"]
SHAPES = [(1, 1, 3, 11, 11), (1, 2, 3, 11, 40), (2, 2, 3, 43, 33), (1, 2, 3, 64, 64)]


def _golden_inputs():
    spec = importlib.util.spec_from_file_location("make_golden_recon", os.path.join(GOLDEN, "make_golden_recon.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.inputs()


# ---------------------------------------------------------------------------------------------------------------- the oracle

@pytest.mark.parametrize("shape", SHAPES)
def test_valid_form_equals_reflect_pad_and_crop(shape):
    for name, real, gen in rc.families(300 + shape[-1], shape):
        a, b = rc.oracle(real, gen), rc.oracle(real, gen, form="reflect")
        assert a["ssim_map"].shape == b["ssim_map"].shape == (shape[0] * shape[1], shape[2], shape[3] - 10, shape[4] - 10)
        worst = float((a["ssim_map"] - b["ssim_map"]).abs().max())
        print(f"{shape} {name}: valid vs reflect-pad-and-crop, max |d ssim map| {worst:.2e}")
        assert worst <= 1e-13 and abs(float(a["ssim"] - b["ssim"])) <= 1e-13 and a["terms"] == b["terms"]


def test_identical_inputs_give_one_and_inf():
    for _, real, _ in rc.families(17, (2, 2, 3, 16, 23)):
        ref = rc.oracle(real, real.clone())
        assert float(ref["ssim"]) == 1.0 and float(ref["psnr"]) == float("inf") and float(ref["l1"]) == 0.0
        assert bool((ref["ssim_map"] == 1.0).all())


def test_psnr_takes_the_range_of_the_generated_frames_only():
    real, gen = rc.pair(5, (1, 2, 3, 16, 16), 0.1)
    ref, wide = rc.oracle(real, gen), rc.oracle(2 * real, gen)            # a wider real clip moves the MSE but not R
    assert float(ref["range_psnr"]) == float(wide["range_psnr"]) == float(gen.double().max() - gen.double().min())
    assert float(wide["range_ssim"]) > float(ref["range_ssim"])
    fixed = rc.oracle(real, gen, data_range=2.0)
    assert float(fixed["range_psnr"]) == float(fixed["range_ssim"]) == 2.0 and float(fixed["mse"]) == float(ref["mse"])


@pytest.mark.parametrize("shape", SHAPES)
def test_gate_accepts_the_other_order_and_rejects_deliberate_errors(shape):
    for name, real, gen in rc.families(100 + shape[-1], shape):
        ref = rc.oracle(real, gen)
        print(f"{shape} {name}")
        assert rc.all_ok(rc.check_scalars(rc.oracle(real, gen, form="reflect"), ref, what="reflect form"))   # same formula, another order
        for m in rc.MUTATIONS:
            res = rc.check_scalars(rc.oracle(real, gen, mutate=m), ref, verbose=False)
            assert not rc.all_ok(res), (shape, name, m)
        # the fp32 window sums are what a gate at 1e-7 could not tell from the float64 kernel
        fp32 = rc.oracle(real, gen, mutate="fp32_sums")
        rel = abs(float(fp32["ssim"] - ref["ssim"])) / abs(float(ref["ssim"]))
        assert rel > float(ref["bound_ssim"] / ref["ssim"].abs()) and rc.check_scalars(fp32, ref, verbose=False)["ssim"][0] is False
        rows_ok = rc.gate("per-image rows, fp32 sums", fp32["per_image"], ref["per_image"], ref["bound_per_image"], verbose=False)[0]
        assert not rows_ok


def test_kl_oracle_bound_and_fixture():
    arr, meta = load_golden("recon")
    x = _golden_inputs()
    for b, d in meta["kl_cases"]:
        mu, lv = x[f"kl_{b}x{d}"]
        value, bound = rc.kl_oracle(mu, lv)
        ref32, ref64 = arr[f"kl_{b}x{d}"]
        assert abs(float(value) - ref64) <= float(bound) and float(bound) < rc.REL_CEILING * abs(float(value))
        assert abs(float(value) - ref32) <= 1e-5 * abs(float(value))


# ---------------------------------------------------------------------------------------------------------------- surface

def test_hinge_and_fmap_loss_match_the_reference():
    arr, _ = load_golden("recon")
    x = _golden_inputs()
    f1, f2 = x["fmap"]
    assert float(loss_mod.fmap_loss(f1, f2, "L1")) == pytest.approx(arr["fmap"][0], rel=1e-6)
    assert float(loss_mod.fmap_loss(f1, f2, "L2")) == pytest.approx(arr["fmap"][1], rel=1e-6)
    fake, orig = x["hinge"]
    assert float(loss_mod.hinge_loss(fake, orig, "disc")) == pytest.approx(arr["hinge"][0], rel=1e-6)
    assert float(loss_mod.hinge_loss(fake, orig, "gen")) == pytest.approx(arr["hinge"][1], rel=1e-6)
    assert loss_mod.hinge_loss(fake, orig, "other") is None


def test_header_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(REPO, "include", "i2v_hip.h")).read()
    declared = set(re.findall(r"\b(i2v_[a-z0-9_]+)\s*\(", header))
    lib = i2v_native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in i2v_native.SYMBOLS and hasattr(lib, name), name
    for ref in ("stage1_VAE/modules/loss.py", "Backward.eval :183-216", "KL :10-12", "loss.py:191", ":194 ssim", ":199 the L1 error"):
        assert ref in header, ref
    assert "i2v_recon.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    for name in ("stage1_VAE/modules/loss.py", "stage1_VAE/main.py", "eval_reconstruction.py"):
        text = open(os.path.join(PKG, name)).read()
        assert not re.search(r"^\s*(import|from) (pytorch_lightning|wandb|omegaconf|torchmetrics)", text, flags=re.M), name


def test_size_query_and_refusals_need_no_gpu():
    lib = i2v_native.lib()
    assert lib.i2v_recon_workspace_bytes(2, 4, 3, 64, 64) > 0
    assert lib.i2v_recon_workspace_bytes(0, 4, 3, 64, 64) == 0 and lib.i2v_recon_workspace_bytes(2, 4, 3, 64, -1) == 0
    # bad arguments are refused before any launch, so these return without a device
    assert lib.i2v_recon_stats(None, None, 1, 1, 3, 16, 16, 0, 0, None, 2.0, None, None, None, 0, None) == -1
    assert lib.i2v_recon_range(None, None, 1, 1, 3, 16, 16, 0, 0, None, None, 0, None) == -1
    assert lib.i2v_kl_normal(None, None, 1, 1, None, None) == -1
    assert b"i2v_kl_normal" in lib.i2v_last_error()


def test_every_entry_refuses_to_run_without_a_gpu():
    x = torch.zeros(1, 2, 3, 16, 16)
    for call in (lambda: i2v_native.recon_range(x, x), lambda: i2v_native.recon_stats(x, x), lambda: i2v_native.recon_stats(x, x, 2.0),
                 lambda: i2v_native.kl_normal(torch.zeros(2, 4), torch.zeros(2, 4)), lambda: loss_mod.KL(torch.zeros(2, 4), torch.zeros(2, 4)),
                 lambda: loss_mod.psnr(x[0], x[0]), lambda: loss_mod.ssim(x[0], x[0], data_range=2.0), lambda: loss_mod.recon_metrics(x, x, per_image=True)):
        with pytest.raises(i2v_native.I2VError):
            call()
    with pytest.raises(i2v_native.I2VError, match="data_range"):
        i2v_native.recon_stats(x, x, data_range=0.0)
    with pytest.raises(i2v_native.I2VError, match=r"\[B,T,C,H,W\]"):
        i2v_native.recon_stats(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))


def test_backward_forward_raises_and_training_entry_points_exit():
    bw = loss_mod.Backward({"Training": {"w_kl": 1e-6, "w_recon": 2.0}, "Data": {"sequence_length": 17}})
    assert bw.w_kl == 1e-6 and bw.w_mse == 2.0 and bw.seq_length == 17 and bw.lpips is None and bw.w_GP is None
    assert loss_mod.Backward(None).w_kl is None
    with pytest.raises(NotImplementedError, match="discriminators") as e:
        bw.forward(None, None, None, None, None, None, 0, None)
    assert "backward passes" in str(e.value) and "decoder" in str(e.value) and "encoder" in str(e.value)
    with pytest.raises(SystemExit, match="not built"):
        stage1_main.main()
    with pytest.raises(SystemExit, match="not built"):
        stage1_main.trainer(None, None, None, None, None, None, 0, [], None, None)


@pytest.mark.parametrize("argv,word", [
    ([], "-ckpt_path DIR"),
    (["-ckpt_path", "d"], "-clips_npy FILE"),
    (["-ckpt_path", "d", "-clips_npy", "c.npy", "-vgg_path", "a.pth"], "-lpips_path FILE"),
    (["-ckpt_path", "d", "-clips_npy", "c.npy", "-lpips_path", "a.pth"], "-vgg_path FILE"),
    (["-ckpt_path", "d", "-clips_npy", "c.npy", "-data_range", "0"], "-data_range must be positive"),
    (["-ckpt_path", "d", "-clips_npy", "c.npy", "-bs", "0"], "-bs must be at least 1"),
])
def test_cli_argument_errors(argv, word):
    r = subprocess.run([sys.executable, os.path.join(PKG, "eval_reconstruction.py"), "-gpu", "0"] + argv, capture_output=True, text=True, cwd=PKG)
    assert r.returncode != 0 and word in r.stderr, (r.returncode, r.stderr)


def test_cli_help_lists_the_flags():
    r = subprocess.run([sys.executable, os.path.join(PKG, "eval_reconstruction.py"), "--help"], capture_output=True, text=True, cwd=PKG)
    assert r.returncode == 0, r.stderr
    for f in ("-gpu", "-ckpt_path", "-clips_npy", "-bs", "-seed", "-data_range", "-vgg_path", "-lpips_path", "-per_frame"):
        assert re.search(rf"(^|\s){f}\b", r.stdout), f
