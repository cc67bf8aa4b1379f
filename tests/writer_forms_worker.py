"""Worker of tests/test_gpu_writer_stores.py: runs in a process of its own with I2V_LIB_PATH pointing at the MEASUREMENT build of the
library (lib/libi2v_hip_measure.so), the only build that reads I2V_MOD4_FORM and carries every store / loop form of the F(4,3) operand
writer (modulate_wino4_kernel, csrc/i2v_dec_writers.hip): 0 = 8-byte half-piece stores and loads inside the frame (the writer up to round 6),
1 = 16-byte stores (what the production library holds), 3 = 16-byte stores + frame-ahead loads.  Unset = the production form.

argv[1] = JSON {"upsample_s", "upsample_t", "img"}.  For the split mode (nf = 32), the one-term mode ("fp16", nf = 32) and the shared-map
form (realizations = 3) it taps the conv_0 operand (which = 1) and the conv_1 operand (which = 3) of every block whose conv runs an F(4,3)
kernel, into NaN-filled buffers, under every form, and compares bytes and frames against form 0.  Last stdout line: JSON."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "image2video-synthesis-using-cinns_amd")):
    sys.path.insert(0, p)
import i2v_native  # noqa: E402
import i2v_synth as synth  # noqa: E402
from stage1_VAE.modules.decoder import Generator  # noqa: E402

assert os.path.basename(i2v_native.LIB_PATH) == "libi2v_hip_measure.so", i2v_native.LIB_PATH
torch.set_grad_enabled(False)
cfg = json.loads(sys.argv[1])
NF, B = 32, 2
NAMES = ("head_0", "g_0", "g_1", "g_2", "g_3", "g_4")
CIN_F, COUT_F = (16, 16, 16, 8, 4, 2), (16, 16, 8, 4, 2, 1)
F43 = ("conv_wino4_f16x3", "conv_wino4_f16")
FORMS = ("0", "1", "3", None)     # None: the switch unset
PRODUCTION_FORM = 1
bad, checked, shapes = [], 0, set()


def levels():
    """Per block: (T, H, W) of the level it runs at (i2v_dec_create)."""
    T, S, out = 1, 4, []
    for k in range(6):
        ut, us = (1, 1) if k == 0 else (2, 2) if k <= 3 else (cfg["upsample_t"][k - 4], cfg["upsample_s"][k - 4])
        T, S = T * ut, S * us
        out.append((T, S, S))
    return out


def make(mma):
    g = Generator({"channel_factor": NF, "z_dim": 64, "upsample_s": cfg["upsample_s"], "upsample_t": cfg["upsample_t"],
                   "spectral_norm": True, "mma": mma})
    g.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.decoder_state_dict(seed=5, channel_factor=NF).items()})
    return g.cuda().eval()


def run(form, fn):
    if form is None:
        os.environ.pop("I2V_MOD4_FORM", None)
    else:
        os.environ["I2V_MOD4_FORM"] = form
    try:
        out = fn()
        # the switch reached the launch: the measurement build reports the form its last writer launch ran (unset: the production form)
        ran = int(i2v_native.lib().i2v_measure_mod4_last_form())
        if ran != int(form if form is not None else PRODUCTION_FORM):
            bad.append(["form not switched", form, ran])
        return out
    finally:
        os.environ.pop("I2V_MOD4_FORM", None)


x0, z, _ = synth.bench_inputs(3 * B, cfg["img"], 64)
x0, z = x0.cuda(), z.cuda()
lv = levels()
for mode, mma, K in (("split", 1, 1), ("one-term", "fp16", 1), ("shared", 1, 3), ("one-term shared", "fp16", 3)):
    gen = make(mma)
    img, lat = (x0[:B], z[:B]) if K == 1 else (x0[:B], z[:B * K])
    call = (lambda: gen(img, lat)) if K == 1 else (lambda: gen(img, lat, realizations=K))
    h = gen.native()
    h.set_profile(True)
    call()
    torch.cuda.synchronize()
    kern = {r["layer"]: r["kernel"] for r in h.get_layer_profile()}
    h.set_profile(False)
    taps = [(k, which) for k in range(6) for which, conv in ((1, "conv_0"), (3, "conv_1")) if kern[f"{NAMES[k]}.{conv}"] in F43]
    assert taps, kern

    def tap(k, which):
        T, H, W = lv[k]
        C = CIN_F[k] * NF if which == 1 else min(CIN_F[k], COUT_F[k]) * NF
        n = B * K * T * H * W * ((C + 63) // 64 * 64) * 3 // 2        # floats: 6 bytes per activation of the padded tensor, at the most
        dst = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        h.debug_tap(k, which, dst)
        call()
        h.debug_tap(0, 0, None)
        torch.cuda.synchronize()
        shapes.add((W, C, which))
        return dst.view(torch.int32)

    ref_frames = run("0", call).clone()
    ref_taps = {kw: run("0", lambda: tap(*kw)) for kw in taps}
    for kw, v in ref_taps.items():
        written = int((v != 0x7FC00000).sum())     # (the fill's bit pattern)
        if written < v.numel() // 4:
            bad.append([mode, "0", list(kw), "tap holds almost nothing"])
    for form in FORMS[1:]:
        if not torch.equal(run(form, call), ref_frames):
            bad.append([mode, form, "frames"])
        checked += 1
        for kw in taps:
            got = run(form, lambda: tap(*kw))
            if not torch.equal(got, ref_taps[kw]):
                bad.append([mode, form, list(kw), int((got != ref_taps[kw]).sum())])
            checked += 1
            del got
    del ref_taps
torch.cuda.synchronize()
print(json.dumps({"checked": checked, "bad": bad, "shapes": sorted(shapes)}))
