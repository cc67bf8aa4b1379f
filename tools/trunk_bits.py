"""Digests of the I3D, Inception-v3 and VGG-16 trunks for A/B runs of changes to their conv kernels or their host code: prints one sha256
per case over the output bytes of every conv-unit and Mixed case of tests/i3d_units_common.py (both I3D variants) and of
tests/fid_common.py, and of one whole trunk each at its smallest legal input (2 clips of 9 x 32 x 32 frames through the Kinetics I3D and,
repeated to 16 and 32 frames, through the two dynamic-texture I3Ds; 2 images of 75 x 75 through Inception) with the trunks' size queries.  ``vgg`` as the only argument prints the VGG-16 / LPIPS group alone: every conv and dgrad unit case
of tests/vgg_common.py and tests/lpips_grad_common.py, the taps (and the saved buffer) at three shapes, LPIPS and its frame gradient,
one pair reduction and the three size queries.  Two builds of the library compute the same function iff the two outputs are equal, e.g.

    python tools/trunk_bits.py > a.txt;  I2V_LIB_PATH=<other build, relative to the repository> python tools/trunk_bits.py > b.txt

The digests depend on the toolchain (fmaf contraction), so they are compared between builds on one machine, never stored."""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "image2video-synthesis-using-cinns_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch   # noqa: E402

import fid_common as fc          # noqa: E402
import i2v_native                # noqa: E402
import i3d_units_common as uc    # noqa: E402
import lpips_grad_common as lg   # noqa: E402
import vgg_common as vc          # noqa: E402

SENTINEL = -777.25
SEED_FID = 91


def sha(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


def cl5(x):
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def i3d_cases():
    nets = {}
    for v in ("kin", "dt"):
        nets[v] = i2v_native.NativeI3D(uc.CLASSES[v], dt_length=None if v == "kin" else 16)
        nets[v].load(uc.state_dict(v))
    for case in uc.unit_cases():   # into a channel slice of a sentinel-filled buffer, as tests/test_gpu_i3d_units.py does
        n, unit, x = nets[case["variant"]], case["unit"], uc.unit_input(case)
        if unit == uc.UNIT_STEM:
            x = torch.cat([x, uc.randn(case["seed"] + 7, (x.shape[0], 1, *x.shape[2:]))], 1)
        _, cout, od = n.unit_shape(unit, *x.shape[2:])
        out = torch.full((x.shape[0], *od, cout + 20), SENTINEL, dtype=torch.float32, device="cuda")
        n.unit_forward(unit, cl5(x), out, 12)
        print(f"i3d unit {case['id']} {sha(out)}", flush=True)
    for case in uc.MIXED_CASES:
        i = uc.BLOCKS.index(case["block"])
        x = uc.randn(case["seed"], (case["shape"][0], uc.fc.MIXED[i][1], *case["shape"][1:]))
        print(f"i3d mixed {case['id']} {sha(nets[case['variant']].mixed_forward(i, cl5(x)))}", flush=True)
    frames = torch.from_numpy(fc.clips(15001, 2, 9, 32, 32)).cuda().contiguous()
    print(f"i3d trunk kin 2x9x32x32 {sha(nets['kin'].forward(frames, True))}", flush=True)
    L = i2v_native.lib()
    print(f"i3d sizes kin 2x9x32x32 workspace {L.i2v_i3d_workspace_bytes(nets['kin']._h, 2, 9, 32, 32)} features "
          f"{L.i2v_i3d_features_workspace_bytes(nets['kin']._h, 2, 9, 32, 32)} steps {L.i2v_i3d_feature_steps(nets['kin']._h, 9)}", flush=True)
    nets[32] = i2v_native.NativeI3D(uc.CLASSES["dt"], dt_length=32)
    nets[32].load(uc.state_dict("dt"))
    for length, n in ((16, nets["dt"]), (32, nets[32])):   # the dynamic-texture trunks: 9 source frames repeated to the network's length
        print(f"i3d trunk dt{length} 2x9x32x32 t_out {length} {sha(n.features(frames, True, length))}", flush=True)
        print(f"i3d sizes dt{length} 2x{length}x32x32 features {L.i2v_i3d_features_workspace_bytes(n._h, 2, length, 32, 32)} steps "
              f"{L.i2v_i3d_feature_steps(n._h, length)}", flush=True)


def inception_cases():
    for case in fc.conv_cases():   # the channel slices of tests/test_gpu_fid.py
        x, (w, bn) = fc.conv_input(case), fc.conv_params(case)
        xc = fc.to_cl(x, pad4=case["cin"] == 3)
        in_off, out, out_off = 0, None, 0
        if case["slices"]:
            in_off, out_off = 8, 12
            wide = torch.full((*xc.shape[:3], xc.shape[3] + 20), 1e30)
            wide[..., in_off:in_off + xc.shape[3]] = xc
            xc = wide
            (kh, kw), s, (ph, pw), (h, wd) = case["kernel"], case["stride"], case["padding"], case["hw"]
            out = torch.full((x.shape[0], (h + 2 * ph - kh) // s + 1, (wd + 2 * pw - kw) // s + 1, case["cout"] + 16), SENTINEL, device="cuda")
        full = i2v_native.inception_conv_unit(xc.cuda(), w, bn, case["stride"], case["padding"], in_off=in_off, out=out, out_off=out_off)
        print(f"inception conv {case['id']} {sha(full)}", flush=True)
    net = i2v_native.NativeInception()
    net.load(fc.fid_state_dict(SEED_FID))
    for block, batch, hw in fc.MIXED_CASES:
        bi = fc.BLOCK_NAMES.index(block)
        x = fc.randn(13000 + bi, (batch, fc.MIXED[bi][2], *hw))
        print(f"inception mixed {block} {sha(net.mixed(bi, fc.to_cl(x).cuda()))}", flush=True)
    x = torch.from_numpy(fc.clips(14075, 2, 1, 75, 75))[:, 0].contiguous().cuda()
    print(f"inception trunk 2x75x75 {sha(*net.features(i2v_native.inception_input_stage(x, resize=False), (0, 1, 2, 3)))}", flush=True)
    print(f"inception sizes 2x75x75 workspace {[i2v_native.lib().i2v_inception_workspace_bytes(net._h, 2, 75, 75, b) for b in range(4)]} blocks "
          f"{[net.block_shape(2, 75, 75, b) for b in range(4)]}", flush=True)


def vgg_cases():
    from stage2_cINN.AE.modules.LPIPS import LPIPS
    cl = lambda t: None if t is None else vc.to_cl(t).cuda()  # noqa: E731
    for case in vc.conv_cases():
        x, (w, b) = vc.conv_input(case), vc.conv_params(case)
        print(f"vgg conv {case['id']} {sha(i2v_native.vgg_conv_unit(vc.to_cl(x, pad4=case['cin'] == 3).cuda(), w, b))}", flush=True)
    for case in lg.dgrad_cases():
        g, w, add, y, _ = lg.dgrad_inputs(case)
        print(f"vgg dgrad {case['id']} {sha(i2v_native.vgg_dgrad_unit(cl(g), w, cl(add), cl(y)))}", flush=True)
    for case in lg.first_cases():
        g, w, _, _, _ = lg.dgrad_inputs(case)
        print(f"vgg dgrad {case['id']} {sha(i2v_native.vgg_dgrad_unit(cl(g), w, frames=bool(case['frames'])))}", flush=True)
    sd = {k: torch.from_numpy(v) for k, v in vc.vgg_state_dict(lg.SEED_W).items()}
    sd.update({k: torch.from_numpy(v) for k, v in vc.lin_state_dict(lg.SEED_LIN).items()})
    net = i2v_native.NativeVGG()
    net.load(sd)
    shapes = ((3, 16, 16), (2, 35, 29), (1, 24, 40))
    for i, (n, h, w) in enumerate(shapes):
        x = vc.to_cl(vc.randn(8600 + i, (n, 3, h, w)), pad4=True).cuda()
        print(f"vgg taps {n}x{h}x{w} {sha(*net.features(x))}", flush=True)
        taps, saved = net.features(x, save=True)
        print(f"vgg taps saved {n}x{h}x{w} {sha(*taps)} buffer {sha(saved.buf)}", flush=True)
        print(f"vgg sizes {n}x{h}x{w} workspace {i2v_native.lib().i2v_vgg_workspace_bytes(net._h, n, h, w)} saved {net.saved_bytes(n, h, w)} "
              f"backward {i2v_native.lib().i2v_vgg_backward_workspace_bytes(net._h, n, h, w)}", flush=True)
    m = LPIPS()
    m.load_state_dict(_lpips_module_state(sd), strict=False)
    m = m.cuda().eval()
    x0 = torch.from_numpy(vc.clips(8700, 2, 1, 35, 29))[:, 0].contiguous().cuda()
    x1 = torch.from_numpy(vc.clips(8701, 2, 1, 35, 29))[:, 0].contiguous().cuda().requires_grad_(True)
    with torch.enable_grad():
        val = m(x0, x1)
        val.mean().backward()
    print(f"vgg lpips 2x35x29 values {sha(val.detach())} frame gradient {sha(x1.grad)}", flush=True)
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    i2v_native.vgg_pairdiff_update(vc.randn(8800, (5, 3, 7, 64)).cuda(), acc)
    print(f"vgg pairdiff R5 {sha(acc)}", flush=True)


def _lpips_module_state(sd):
    """The native state_dict under the keys of the LPIPS holder module (its trunk's parameters live under ``net.``)."""
    out = {"net." + hk: sd[k] for hk, k in zip(vc.holder_keys(), vc.vgg_state_dict(lg.SEED_W))}
    out.update({k: v for k, v in sd.items() if k.startswith("lin")})
    return out


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    if sys.argv[1:] == ["vgg"]:
        vgg_cases()
    else:
        i3d_cases()
        inception_cases()
        vgg_cases()
