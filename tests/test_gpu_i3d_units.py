"""The I3D kernels unit by unit against float64 at ragged shapes: one conv unit, one Mixed block, one max pool and the head of a LOADED
``i2v_i3d`` handle, run through the sub-module entries (``i2v_i3d_unit_forward``, ``_mixed_forward``, ``_maxpool_forward``,
``_head_forward``) at small maps with H != W, both variants, vs the plain torch float64 oracles of tests/i3d_units_common.py (pinned to
the reference's own modules by tests/test_host_i3d_units.py).

Gate (i3d_units_common.gate): element-wise |got - ref64| <= gamma(n) S + 2^-24 |ref64| -- the dot-product bound of any summation
order -- and rel-L2 <= 1e-4 per batch row; max pools bit for bit.  No slack factor: fp32 torch on the CPU stays below 0.06 of the
bound at these cases (test_host_i3d_units.py), measured GPU maxima are in profiles/i3d_units_gate.md."""
import ctypes

import pytest
import torch

import i2v_native
import i3d_units_common as uc

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
OUT_PAD, OUT_OFF = 20, 12

_NETS = {}


def net(variant, length=None):
    """One loaded handle per variant (and per average-pool length of the dynamic-texture variant), shared by the module."""
    key = (variant, None if variant == "kin" else (length or 16))
    if key not in _NETS:
        n = i2v_native.NativeI3D(uc.CLASSES[variant], dt_length=key[1])
        n.load(uc.state_dict(variant))
        _NETS[key] = n
    return _NETS[key]


def cl(x):
    """[B, C, T, H, W] -> channels-last [B, T, H, W, C] on the device"""
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def ncthw(y):
    return y.permute(0, 4, 1, 2, 3).cpu()


def run_unit(n, case, x):
    """The unit into channels [12, 12 + cout) of a sentinel-filled buffer of cout + 20 channels -> (output [B, cout, To, Ho, Wo], dims)."""
    unit = case["unit"]
    xc = x
    if unit == uc.UNIT_STEM:   # the stem's input layout has 4 channels; the 4th meets zero weights, whatever it holds
        xc = torch.cat([x, uc.randn(case["seed"] + 7, (x.shape[0], 1, *x.shape[2:]))], 1)
    cin, cout, od = n.unit_shape(unit, *x.shape[2:])
    assert cin == xc.shape[1] and cout == uc.unit_spec(case["variant"], unit)[2]
    out = torch.full((x.shape[0], *od, cout + OUT_PAD), SENTINEL, dtype=torch.float32, device="cuda")
    n.unit_forward(unit, cl(xc), out, OUT_OFF)
    torch.cuda.synchronize()
    out = out.cpu()
    lo, hi = out[..., :OUT_OFF], out[..., OUT_OFF + cout:]
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), "the unit wrote outside its channel slice"
    return out[..., OUT_OFF:OUT_OFF + cout].permute(0, 4, 1, 2, 3).contiguous(), od


UNIT_CASES = uc.unit_cases()


@pytest.mark.parametrize("case", UNIT_CASES, ids=[c["id"] for c in UNIT_CASES])
def test_unit_vs_float64(case):
    n = net(case["variant"])
    x = uc.unit_input(case)
    ref, S, nb = uc.unit_oracle(case["variant"], case["unit"], x)
    got, od = run_unit(n, case, x)
    ok, ratio, l2 = uc.gate(got, ref, S, nb)
    print(f"I3DUNITS unit {case['id']}: dims {od}, |err| / bound {ratio:.3e}, rel-L2 {l2:.3e}")
    assert tuple(od) == tuple(ref.shape[2:])
    assert ok, (ratio, l2)


LADDER_MULTI = [c for c in UNIT_CASES if c["shape"] in uc.M_LADDER[2:]]


@pytest.mark.parametrize("case", LADDER_MULTI, ids=[c["id"] for c in LADDER_MULTI])
def test_batch_rows_equal_single_sample_runs_bitwise(case):
    n = net(case["variant"])
    x = uc.unit_input(case)
    both, _ = run_unit(n, case, x)
    for b in range(x.shape[0]):
        one, _ = run_unit(n, case, x[b:b + 1])
        assert torch.equal(one[0], both[b]), b


@pytest.mark.parametrize("case", uc.MIXED_CASES, ids=[c["id"] for c in uc.MIXED_CASES])
def test_mixed_block_vs_float64(case):
    """Branch by branch: the second conv of branch 1 and 2 is checked against the oracle applied to the GPU's own first-conv output (the
    unit entry; the kernel is deterministic, so it is the block's temporary), so the bound stays per layer."""
    variant, block = case["variant"], case["block"]
    n = net(variant)
    i = uc.BLOCKS.index(block)
    name, cin, o = uc.fc.MIXED[i]
    B, T, H, W = case["shape"]
    x = uc.randn(case["seed"], (B, cin, T, H, W))
    xc = cl(x)
    out = n.mixed_forward(i, xc)
    first = [ncthw(n.unit_forward(uc.mixed_unit(block, j), xc)) for j in (1, 3)]
    torch.cuda.synchronize()
    assert tuple(out.shape) == (B, T, H, W, o[0] + o[2] + o[4] + o[5])
    got = ncthw(out)
    for j, t in zip((1, 3), first):   # the first convs themselves
        ref, S, nb = uc.unit_oracle(variant, uc.mixed_unit(block, j), x)
        ok, ratio, l2 = uc.gate(t, ref, S, nb)
        assert ok, (j, ratio, l2)
    lo, worst = 0, (0.0, 0.0)
    for b, (ref, S, nb) in enumerate(uc.mixed_oracle(variant, block, x, first)):
        ok, ratio, l2 = uc.gate(got[:, lo:lo + ref.shape[1]], ref, S, nb)
        worst = max(worst, (ratio, l2))
        assert ok, (b, ratio, l2)
        lo += ref.shape[1]
    assert lo == got.shape[1]
    print(f"I3DUNITS mixed {case['id']}: |err| / bound {worst[0]:.3e}, rel-L2 {worst[1]:.3e}")


POOL_CASES = uc.pool_cases()


@pytest.mark.parametrize("case", POOL_CASES, ids=[c["id"] for c in POOL_CASES])
def test_maxpool_bit_for_bit(case):
    n = net(case["variant"])
    x = uc.pool_input(case)
    ref = uc.maxpool_oracle(case["variant"], x, case["kernel"], case["stride"])
    assert n.maxpool_shape(case["kernel"], case["stride"], *x.shape[2:]) == tuple(ref.shape[2:])
    got = ncthw(n.maxpool_forward(cl(x), case["kernel"], case["stride"]))
    assert torch.equal(got, ref)


@pytest.mark.parametrize("case", uc.HEAD_CASES, ids=[c["id"] for c in uc.HEAD_CASES])
def test_head_vs_float64(case):
    """Average pool (both layouts), classifier and time mean.  The logits' bound is composed per layer from the GPU's own pooled
    features: with cls = conv(pooled) (bound b_t = gamma(K + 2) S_t + u |cls_t| per time step) and logits = mean_t cls_t, the error is at
    most mean_t b_t + gamma(T' + 1) mean_t (|cls_t| + b_t) + u |logits|."""
    variant = case["variant"]
    n = net(variant, case["length"])
    B, T = case["shape"]
    x = uc.randn(case["seed"], (B, 1024, T, 7, 7))
    pooled, feats, logits = (t.cpu() for t in n.head_forward(cl(x)))
    ref, S, nb = uc.avgpool_oracle(x, case["pool_t"])
    assert tuple(feats.shape) == tuple(ref.shape) and torch.equal(pooled.transpose(1, 2), feats)
    ok, ratio, l2 = uc.gate(feats, ref, S, nb)
    cls, Sc, nc = uc.unit_oracle(variant, uc.UNIT_HEAD, feats[..., None, None])
    cls, Sc = cls[..., 0, 0], Sc[..., 0, 0]
    b_t = uc.gamma(nc) * Sc + uc.U * cls.abs()
    want = cls.mean(2)
    bound = b_t.mean(2) + uc.gamma(cls.shape[2] + 1) * (cls.abs() + b_t).mean(2) + uc.U * want.abs()
    ok2, ratio2, l22 = uc.gate_bound(logits, want, bound)
    print(f"I3DUNITS head {case['id']}: avgpool |err| / bound {ratio:.3e}, rel-L2 {l2:.3e}; logits |err| / bound {ratio2:.3e}, rel-L2 {l22:.3e}")
    assert tuple(logits.shape) == (B, uc.CLASSES[variant])
    assert ok, (ratio, l2)
    assert ok2, (ratio2, l22)


def test_argument_refusals():
    """Null pointers, C % 4 != 0, an unknown unit, a short workspace or output and a slice that does not fit are refused before any launch."""
    lib = i2v_native.lib()
    n = net("kin")
    h, st = n._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    INVALID, WORKSPACE = -1, -4
    x = torch.zeros(1, 2, 5, 4, 192, device="cuda")
    out = torch.full((1, 2, 5, 4, 256), SENTINEL, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    u = uc.mixed_unit("mixed_3b", 3)   # 192 -> 16
    od = (ctypes.c_int32 * 3)()
    a = (1, 2, 5, 4)
    assert lib.i2v_i3d_unit_forward(None, u, x.data_ptr(), *a, 192, out.data_ptr(), 36, 12, out.numel(), st) == INVALID
    assert lib.i2v_i3d_unit_forward(h, u, None, *a, 192, out.data_ptr(), 36, 12, out.numel(), st) == INVALID
    assert lib.i2v_i3d_unit_forward(h, u, x.data_ptr(), *a, 192, None, 36, 12, out.numel(), st) == INVALID
    assert lib.i2v_i3d_unit_forward(h, 58, x.data_ptr(), *a, 192, out.data_ptr(), 36, 12, out.numel(), st) == INVALID
    assert lib.i2v_i3d_unit_forward(h, -1, x.data_ptr(), *a, 192, out.data_ptr(), 36, 12, out.numel(), st) == INVALID
    assert lib.i2v_i3d_unit_forward(h, u, x.data_ptr(), *a, 190, out.data_ptr(), 36, 12, out.numel(), st) == INVALID     # in_cs % 4
    assert lib.i2v_i3d_unit_forward(h, u, x.data_ptr(), *a, 188, out.data_ptr(), 36, 12, out.numel(), st) == INVALID     # in_cs < cin
    assert lib.i2v_i3d_unit_forward(h, u, x.data_ptr(), *a, 192, out.data_ptr(), 36, 21, out.numel(), st) == INVALID     # 21 + 16 > 36
    assert "do not fit" in lib.i2v_last_error().decode()
    assert lib.i2v_i3d_unit_forward(h, u, x.data_ptr(), *a, 192, out.data_ptr(), 36, -4, out.numel(), st) == INVALID
    assert lib.i2v_i3d_unit_forward(h, u, x.data_ptr(), *a, 192, out.data_ptr(), 36, 12, 40 * 36 - 1, st) == WORKSPACE
    assert lib.i2v_i3d_unit_shape(h, 99, 2, 5, 4, None, None, od) == INVALID and lib.i2v_i3d_unit_shape(None, u, 2, 5, 4, None, None, od) == INVALID
    need = lib.i2v_i3d_mixed_workspace_bytes(h, 0, *a)
    assert need >= 40 * 192 * 4 and lib.i2v_i3d_mixed_workspace_bytes(h, 9, *a) == 0
    assert lib.i2v_i3d_mixed_forward(h, 0, x.data_ptr(), *a, out.data_ptr(), ws.data_ptr(), need - 1, st) == WORKSPACE
    assert lib.i2v_i3d_mixed_forward(h, 9, x.data_ptr(), *a, out.data_ptr(), ws.data_ptr(), need, st) == INVALID
    assert lib.i2v_i3d_mixed_forward(h, 0, None, *a, out.data_ptr(), ws.data_ptr(), need, st) == INVALID
    assert lib.i2v_i3d_mixed_forward(h, 0, x.data_ptr(), *a, out.data_ptr(), None, need, st) == INVALID
    assert lib.i2v_i3d_mixed_forward(None, 0, x.data_ptr(), *a, out.data_ptr(), ws.data_ptr(), need, st) == INVALID
    p = (1, 3, 1, 2)
    assert lib.i2v_i3d_maxpool_forward(h, x.data_ptr(), *a, 190, *p, out.data_ptr(), out.numel(), st) == INVALID          # C % 4
    assert "multiple of 4" in lib.i2v_last_error().decode()
    assert lib.i2v_i3d_maxpool_forward(h, None, *a, 192, *p, out.data_ptr(), out.numel(), st) == INVALID
    assert lib.i2v_i3d_maxpool_forward(h, x.data_ptr(), *a, 192, *p, None, out.numel(), st) == INVALID
    assert lib.i2v_i3d_maxpool_forward(None, x.data_ptr(), *a, 192, *p, out.data_ptr(), out.numel(), st) == INVALID
    assert lib.i2v_i3d_maxpool_forward(h, x.data_ptr(), *a, 192, 1, 0, 1, 2, out.data_ptr(), out.numel(), st) == INVALID
    assert lib.i2v_i3d_maxpool_forward(h, x.data_ptr(), *a, 192, *p, out.data_ptr(), 2 * 3 * 2 * 192 - 1, st) == WORKSPACE
    assert lib.i2v_i3d_maxpool_shape(h, *p, 2, 5, 4, None) == INVALID
    xh = torch.zeros(1, 2, 7, 7, 1024, device="cuda")
    o1, o2, o3 = (torch.full((1024,), SENTINEL, device="cuda") for _ in range(3))
    needh = lib.i2v_i3d_head_workspace_bytes(h, 1, 2)
    assert needh >= 400 * 4 and lib.i2v_i3d_head_workspace_bytes(h, 1, 1) == 0
    assert lib.i2v_i3d_head_forward(h, xh.data_ptr(), 1, 2, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), ws.data_ptr(), needh - 1, st) == WORKSPACE
    assert lib.i2v_i3d_head_forward(h, xh.data_ptr(), 1, 1, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), ws.data_ptr(), needh, st) == INVALID
    assert lib.i2v_i3d_head_forward(h, None, 1, 2, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), ws.data_ptr(), needh, st) == INVALID
    assert lib.i2v_i3d_head_forward(h, xh.data_ptr(), 1, 2, o1.data_ptr(), None, o3.data_ptr(), ws.data_ptr(), needh, st) == INVALID
    assert lib.i2v_i3d_head_forward(None, xh.data_ptr(), 1, 2, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), ws.data_ptr(), needh, st) == INVALID
    # an unloaded handle is I2V_E_STATE
    raw = ctypes.c_void_p()
    assert lib.i2v_i3d_create(400, 3, ctypes.byref(raw)) == 0
    try:
        assert lib.i2v_i3d_unit_forward(raw, u, x.data_ptr(), *a, 192, out.data_ptr(), 36, 12, out.numel(), st) == -5
    finally:
        lib.i2v_i3d_destroy(raw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and all(bool((o == SENTINEL).all()) for o in (o1, o2, o3)), "a refused call launched something"
