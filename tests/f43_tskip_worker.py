"""Worker of tests/test_gpu_f43_tskip.py: runs in a process of its own with I2V_LIB_PATH on the MEASUREMENT build of the library, the
only build in which I2V_W4_TSKIP=0 sends the F(4,3) layers to the full tap loops of conv_wino4_f16x3_kernel (the parent's kernel, the
bit reference) instead of conv_wino4e_f16x3_kernel, which skips the (kt, row block) units that read only the clip's temporal zero
padding.  Part by part (argv[1]: "blocks", "decoders", "goldens", "units"), JSON on the last stdout line."""
import json
import os
import re
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "image2video-synthesis-using-cinns_amd")):
    sys.path.insert(0, p)
import i2v_native  # noqa: E402
import i2v_synth as synth  # noqa: E402

assert os.path.basename(i2v_native.LIB_PATH) == "libi2v_hip_measure.so", i2v_native.LIB_PATH
torch.set_grad_enabled(False)
os.environ["I2V_DEC_WINO4"] = "2"      # F(4,3) wherever its tiling allows (small grids too)
W4_EDGE, W4_EDGE_ONE, W4_SPLIT, W4_ONE = 7, 8, 0, 1   # W4Form (csrc/i2v_conv16w4_dev.h)


def dead_share(T, KT, tdup):
    """Closed form of the issue's table: dead units / units of a launch with T input frames (TT = 4, or 2 for the two-frame pairs)."""
    TT = 4 if T % 4 == 0 else 2
    nbT = T // TT
    if tdup:       # per parity ONE end: all row blocks of one frame of one t-brick, of 2 kt x 4 row blocks x nbT bricks
        return (4 // TT) / (2 * 4 * nbT)
    return 2 * (4 // TT) / (3 * 4 * nbT)


class Trace:
    """I2V_W4_TRACE lines (one per F(4,3) launch, on stderr) of what runs inside the block."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        os.environ["I2V_W4_TRACE"] = "1"
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        os.environ.pop("I2V_W4_TRACE")
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        self.launches = [{k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)(?= |$)", ln)} for ln in text.splitlines() if ln.startswith("wino4:")]
        sys.stderr.write("".join(ln + "\n" for ln in text.splitlines() if not ln.startswith("wino4:")))


def both(fn):
    """fn() on the full loops (I2V_W4_TSKIP=0) and on the edge kernel (default), with the launches of each."""
    os.environ["I2V_W4_TSKIP"] = "0"
    with Trace() as t0:
        ref = fn()
    os.environ.pop("I2V_W4_TSKIP")
    with Trace() as t1:
        out = fn()
    return ref, out, t0.launches, t1.launches


def blocks():
    """Stand-alone GeneratorBlocks (i2v_gblock_forward: SPADE + 3x3x3 conv_0 with fused statistics, ADAIN + conv_1 with the residual
    epilogue) at 16 x 16: Cin x Cout = 64 -> 64, 32 -> 32, 32 -> 64, 64 -> 32 over the pairs below, T = 2 .. 16, B = 1 and 3, 32- and
    64-channel workgroups.  Bit equality with the full loops, the fp64 block oracle at the stand-alone block's gates."""
    from oracle import decoder_ref
    from stage1_VAE.modules import decoder as dec
    from test_gpu_decoder_configs import CONTRACT, METRICS, ZD, _block_sd, _gate, metrics
    bad, n = [], 0
    for n_in, n_out in ((64, 64), (32, 64), (64, 32)):
        sd = _block_sd(n_in, n_out, seed=n_in * 7 + n_out)
        sd64 = {"blk." + k: v.double().cuda() for k, v in sd.items()}
        blk = dec.GeneratorBlock(n_in, n_out, True, ZD)
        blk.load_state_dict(sd)
        blk = blk.cuda().eval()
        g = torch.Generator().manual_seed(n_in + n_out)
        for T in (2, 4, 8, 16):
            for B in (1, 3):
                x = torch.randn(B, n_in, T, 16, 16, generator=g).cuda()
                img = (2 * torch.rand(B, 3, 24, 40, generator=g) - 1).cuda()
                z = torch.randn(B, ZD, generator=g).cuda()
                ref64 = decoder_ref.generator_block(sd64, "blk", x.double(), z.double(), img.double(), faithful=False)
                # workgroup forms: the plan's own (at these sizes 32-channel workgroups: 512 threads where the layer has 64 output channels,
                # the 256-thread geometry -- row blocks spanning two frames, never the edge form -- where it has 32), 64-channel
                # workgroups, and the 512-thread geometry for the 32-channel layers too
                for sw in ({}, {"I2V_W4_BN": "64"}, {"I2V_W4_NTH": "512"}):
                    os.environ.update(sw)
                    ref, out, l0, l1 = both(lambda: blk(x, z, img))
                    for k in sw:
                        os.environ.pop(k)
                    tag = f"{n_in}->{n_out} T={T} B={B} {sw}"
                    n += 1
                    if not torch.equal(ref, out):
                        bad.append(f"{tag}: bits differ, max {float((ref - out).abs().max()):.3g}")
                    m = metrics(out, ref64, 1, (0, 2))
                    for metric in METRICS:
                        gate = min(_gate("gblock", metric), CONTRACT)
                        if not m[metric] <= gate:
                            bad.append(f"{tag}: {metric} {m[metric]:.3e} > {gate:.1e}")
                    # T = 2: a 3x3x3 halo brick of 2 x 16 rows does not fit the kernel's V buffers -- no F(4,3) launch at all
                    # (SPADE's 2-D conv is a 3-tap launch of the same entry: never the edge form)
                    want = 0 if T == 2 else 2
                    f0, f1 = ([(r["Cin"], r["Cout"], r["form"]) for r in ls if r["KT"] == 3] for ls in (l0, l1))
                    edge = [W4_EDGE if f[1] % 64 == 0 or "I2V_W4_NTH" in sw else W4_SPLIT for f in f1]
                    if len(f0) != want or len(f1) != want or any(f[2] != W4_SPLIT for f in f0) or [f[2] for f in f1] != edge or \
                            any(r["form"] != W4_SPLIT for r in l0 + l1 if r["KT"] == 1):
                        bad.append(f"{tag}: launches {f0} / {f1}")
        assert blk.native().status() == 0
    return {"cases": n, "bad": bad}


def _decoder(nf, ups, upt, seed, mma=1):
    h = i2v_native.NativeDecoder(nf, 64, list(ups), list(upt), True, mma=mma)
    h.load({k: torch.from_numpy(np.asarray(v)) for k, v in synth.decoder_state_dict(seed=seed, channel_factor=nf).items()})
    return h


def decoders():
    """Decoder handles (temporal-duplication pair kernels with T_out = 4, 8, 16 and both parities, residuals through the x2 / x2
    up-sampling map, the lrelu epilogue of the last block, fused statistics): nf = 8 and nf = 16, B = 1 and 3, split-fp16 and the one-term
    fp16 form (mma = "fp16").  Bit equality of the frames, and per F(4,3) layer the profile's issued-MFMA FLOPs shrink by exactly the
    closed-form dead share."""
    bad, n, shares = [], 0, {}
    for nf, mma in ((8, 1), (16, 1), (8, 3), (16, 3)):
        h = _decoder(nf, (2, 1), (2, 1), 300 + nf, mma)
        kname, f_edge, f_full = ("conv_wino4_f16x3", W4_EDGE, W4_SPLIT) if mma == 1 else ("conv_wino4_f16", W4_EDGE_ONE, W4_ONE)
        for B in (1, 3):
            g = torch.Generator().manual_seed(nf + B)
            img = (2 * torch.rand(B, 3, 48, 80, generator=g) - 1).cuda()
            z = torch.randn(B, 64, generator=g).cuda()
            prof = []

            def run():
                h.set_profile(True)
                out = h.forward(img, z).clone()
                torch.cuda.synchronize()
                h.get_profile()
                prof.append({r["layer"]: r for r in h.get_layer_profile()})
                return out
            ref, out, l0, l1 = both(run)
            h.set_profile(False)
            n += 1
            if not torch.equal(ref, out):
                bad.append(f"nf={nf} B={B}: bits differ, max {float((ref - out).abs().max()):.3g}")
            # the launches of the two runs pair up one to one (same layers, same order); edge form wherever 3-D taps run on 512 threads
            if len(l0) != len(l1):
                bad.append(f"nf={nf} B={B}: {len(l0)} vs {len(l1)} launches")
            lay = [name for name in i2v_native.NativeDecoder.LAYER_NAMES if prof[0][name]["kernel"] == kname]
            l3d = [r for r in l1 if r["KT"] >= 2]
            if len(l3d) != len(lay):
                bad.append(f"nf={nf} B={B}: {len(l3d)} 3-D launches for layers {lay}")
                continue
            for name, r in zip(lay, l3d):
                edge = r["TT"] * r["TH"] == 32 and r["TT"] in (2, 4) and r["nvirt"] > 0 and r["form"] == f_edge
                thin = r["form"] == f_full        # 256-thread geometry: row blocks span two frames, nothing to skip
                want = 1.0 - dead_share(r["T"], r["KT"], r["tdup"]) if edge else 1.0
                got = prof[1][name]["mfma_flops"] / prof[0][name]["mfma_flops"]
                shares[f"{name} T={r['T']} KT={r['KT']} mma={mma}"] = round(got, 6)
                if not (edge or thin) or abs(got - want) > 1e-12:
                    bad.append(f"nf={nf} mma={mma} B={B} {name}: form {r['form']} issued share {got} (closed form {want})")
        assert h.status() == 0
    return {"cases": n, "bad": bad, "shares": shares}


def goldens():
    """The whole decoders of the dec_nf64_bair and dec_nf32_128 goldens, 3 samples (grids that are not a multiple of the CU count), in
    split-fp16 mode (held to the golden) and in the one-term fp16 mode."""
    from conftest import load_golden, rel_l2
    from stage1_VAE.modules.decoder import Generator
    bad = []
    for name, mma in (("dec_nf64_bair", 1), ("dec_nf32_128", 1), ("dec_nf64_bair", "fp16"), ("dec_nf32_128", "fp16")):
        g, meta = load_golden(name)
        x0, z, _ = synth.bench_inputs(3, g["img"].shape[-1], 64)
        x0[1], z[1] = torch.from_numpy(g["img"][0]), torch.from_numpy(g["z"][0])
        x0, z = x0.cuda(), z.cuda()
        os.environ.pop("I2V_DEC_WINO4", None)          # the shipped kernel choice
        gen = Generator({"channel_factor": meta["synth"]["channel_factor"], "z_dim": 64, "upsample_s": meta["upsample_s"],
                         "upsample_t": meta["upsample_t"], "spectral_norm": True, "mma": mma})
        gen.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.decoder_state_dict(**meta["synth"]).items()})
        gen = gen.cuda().eval()
        ref, out, l0, l1 = both(lambda: gen(x0, z))
        if not torch.equal(ref, out):
            bad.append(f"{name} mma={mma}: bits differ, max {float((ref - out).abs().max()):.3g}")
        if mma == 1 and rel_l2(out[1:2, ..., ::2, ::2].cpu(), g["out_s2"]) >= 2e-5:
            bad.append(f"{name}: golden")
        edge = W4_EDGE if mma == 1 else W4_EDGE_ONE
        if not any(r["form"] == edge for r in l1) or any(r["form"] in (W4_EDGE, W4_EDGE_ONE) for r in l0):
            bad.append(f"{name} mma={mma}: forms {[r['form'] for r in l0]} / {[r['form'] for r in l1]}")
    return {"cases": 4, "bad": bad}


def units():
    """Every unit of the decoder nf40_bair with F(4,3) on every layer it tiles (pairs included) within the float64 bounds of
    tests/test_gpu_dec_units.py -- convs and fused statistics on the edge kernel."""
    import pytest
    import test_gpu_dec_units as tu
    from test_gpu_decoder_configs import _inputs
    sd, img, z = _inputs("nf40_bair")
    mp = pytest.MonkeyPatch()
    try:
        tu.test_decoder_units_vs_fp64({"name": "nf40_bair", "sd": sd, "img": img.cuda(), "z": z.cuda()}, "mma1_w4all", mp)
    finally:
        mp.undo()
    return {"cases": 1, "bad": [], "worst": {k: round(v, 4) for k, v in tu.WORST.items()}}


if __name__ == "__main__":
    res = {"blocks": blocks, "decoders": decoders, "goldens": goldens, "units": units}[sys.argv[1]]()
    torch.cuda.synchronize()
    print(json.dumps(res))
