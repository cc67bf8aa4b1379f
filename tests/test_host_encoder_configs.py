"""Motion-encoder configurations (tests/encoder_cfgs.py) on the CPU: the float64 oracle against the reference module's outputs, the
ledger of which kernel path each case reaches, and how far three modelled indexing mistakes move the result.  CPU-only."""
import numpy as np
import pytest
import torch

import encoder_cfgs as ec
import i2v_synth as synth
from conftest import load_golden, rel_l2
from oracle import encoder_ref

torch.set_grad_enabled(False)
REF_TOL = 1e-5   # float64 oracle vs the reference's fp32 module: the reference's own rounding (measured <= 1.8e-6)
GATE = 1e-4      # the project's parity gate on the GPU (test_gpu_encoder_configs.TOL)


def sd64(args):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.encoder3d_state_dict(**args).items()}


def clip(case, head=None, total=None):
    """The case's clip from its seed; checked against the stored head / checksum where the fixture has them."""
    x = 2 * torch.rand(*case["x_shape"], generator=torch.Generator().manual_seed(case["x_seed"])) - 1
    if head is not None:
        assert np.array_equal(x.reshape(-1)[:16].numpy(), head) and abs(float(x.double().sum()) - float(total)) < 1e-6
    return x


def oracle64(case, sd=None, x=None):
    a = case["synth"]
    sd = sd64(a) if sd is None else sd
    x = clip(case).double() if x is None else x
    return encoder_ref.encoder(sd, x, a["channels"], a["stride_s"], case["stride_t"])


def test_fp64_oracle_vs_reference_module():
    g, meta = load_golden("enc3d_cfgs")
    assert sorted(meta["cases"]) == sorted(ec.REF_NAMES)
    for name in ec.REF_NAMES:
        case = meta["cases"][name]
        assert case == {k: ec.CASES[name][k] for k in case}, name   # the fixture was made from the table as it stands
        x = clip(case, g[name + "_x_head"], g[name + "_x_sum"])
        mu, logvar = oracle64(case, x=x.double())
        e_mu, e_lv = rel_l2(g[name + "_mu"], mu), rel_l2(g[name + "_logvar"], logvar)
        print(f"{name}: reference fp32 module vs fp64 oracle  mu {e_mu:.2e}  logvar {e_lv:.2e}")
        assert mu.dtype == torch.float64 and e_mu <= REF_TOL and e_lv <= REF_TOL, (name, e_mu, e_lv)
    for name in ("enc3d_bair", "enc3d_land"):
        g, meta = load_golden(name)
        case = dict(meta, name=name)
        mu, logvar = oracle64(case, x=clip(case, g["x_head"], g["x_sum"]).double())
        e_mu, e_lv = rel_l2(g["mu"], mu), rel_l2(g["logvar"], logvar)
        print(f"{name}: reference fp32 module vs fp64 oracle  mu {e_mu:.2e}  logvar {e_lv:.2e}")
        assert e_mu <= REF_TOL and e_lv <= REF_TOL, (name, e_mu, e_lv)


def test_cases_reach_every_kernel_path():
    reached = {}
    for name, c in ec.CASES.items():
        a = c["synth"]
        reached[name] = ec.encoder_paths(a["channels"], a["stride_s"], c["stride_t"], c["x_shape"][2])
    for name in ("enc3d_bair", "enc3d_land"):
        _, meta = load_golden(name)
        reached[name] = ec.encoder_paths(meta["synth"]["channels"], meta["synth"]["stride_s"], meta["stride_t"], meta["x_shape"][2])
    # every weight set / kernel of a first block, with and without the downsample branch where one can be missing: a strided first
    # block always has one (spatial stride: resnet3D.py:180; temporal stride only: refused without)
    want = {(m, True) for m in ec.MEMBERS} | {("c1_16", False)}
    assert {p for paths in reached.values() for p in paths} == want
    t1 = {name for name, paths in reached.items() if any(m.endswith("_t1") for m, _ in paths)}
    assert t1 == {"t8", "t7_128", "t3", "st2_ss1_t1"}
    assert ("fp32_t1", True) in reached["st2_ss1_t1"] and ("fp32_strided", True) in reached["st2_ss1"]
    assert reached["nodown_l0"][0] == ("c1_16", False) and reached["dtdb"][0] == ("s2d", True)
    assert not t1 & {"enc3d_bair", "enc3d_land"}   # what the two older fixtures never ran
    with pytest.raises(ValueError):   # the configuration i2v_encoder3d_create refuses
        ec.encoder_paths([64, 64, 32, 48, 64], [1, 2, 2, 2], [2, 2, 2, 1], 15)
    # the cases the reference can build have its 64-channel stem; every case ends in the [1,4,4] map of conv_mu / conv_var
    for name, c in ec.CASES.items():
        a, (_, _, frames, h, w) = c["synth"], c["x_shape"]
        assert (a["channels"][0] == 64) == (name in ec.REF_NAMES)
        t = (frames - 1) // 2 + 1
        assert t & (t - 1) == 0
        for st in c["stride_t"]:
            t = (t + 1) // 2 if st == 2 else t
        assert (t, h // 2 // int(np.prod(a["stride_s"])), w // 2 // int(np.prod(a["stride_s"]))) == (1, 4, 4), name


def test_modelled_mistakes_move_mu_ten_gates():
    """Case c0_16 in float64: a dropped corner tap of a strided conv, a dropped output channel and a dropped image row each move mu by
    more than ten times the GPU gate, so the end-to-end comparison sees them.  (Measured: 1.5e-1, 5.8e-2, 7.7e-2.)"""
    case = ec.CASES["c0_16"]
    sd, x = sd64(case["synth"]), clip(case).double()
    mu, _ = oracle64(case, sd, x)

    def moved(key=None, edit=None, xin=x, rows=slice(None)):
        sd2 = dict(sd)
        if key is not None:
            sd2[key] = sd[key].clone()
            edit(sd2[key])
        mu2, _ = oracle64(case, sd2, xin)
        return rel_l2(mu2[rows], mu[rows])

    def zero_tap(w):
        w[:, :, 0, 0, 0] = 0

    def zero_channel(w):
        w[-1] = 0

    e_tap = moved("layer.1.0.downsample.0.weight", zero_tap)
    e_ch = moved("layer.2.0.conv1.weight", zero_channel)
    x2 = x.clone()
    x2[-1, :, :, -1, :] = 0
    e_row = moved(xin=x2, rows=slice(-1, None))
    print(f"c0_16 sensitivity of mu: corner tap {e_tap:.2e}  output channel {e_ch:.2e}  image row {e_row:.2e}")
    assert min(e_tap, e_ch, e_row) > 10 * GATE, (e_tap, e_ch, e_row)
