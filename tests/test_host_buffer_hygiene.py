"""The buffer-hygiene harness (tests/buffer_hygiene_common.py) on trial, on the CPU: four fake entries in plain torch stand in for a native
entry with its binding.  The harness has to accept the clean one and reject each broken one with a message that names the property it
breaks; a harness that passes everything would make tests/test_gpu_buffer_hygiene.py worthless."""
import types

import pytest
import torch

import buffer_hygiene_common as bh


def _binding(entry):
    """A module that, like i2v_native, reaches torch through its global name: it sizes a workspace, allocates an output and calls the entry."""
    mod = types.ModuleType("fake_binding")
    mod.torch = torch

    def call(x):
        t = mod.torch
        ws = t.empty(4 * x.numel() + 256, dtype=t.uint8, device=x.device)
        out = t.empty_like(x)
        entry(x, out, ws)
        return [out]
    mod.call = call
    return mod


def clean(x, out, ws):
    part = ws[: 4 * x.numel()].view(torch.float32)
    part.copy_(x.reshape(-1) * 2)            # writes the slots it reads
    out.copy_((part + 1).view_as(x))


def overrun(x, out, ws):
    clean(x, out, ws)
    storage = torch.empty(0, dtype=torch.uint8).set_(ws.untyped_storage())       # the view a kernel has: the raw address
    end = ws.storage_offset() + ws.numel()
    storage[end: end + 4] = 0x5A                                                  # 4 bytes past the workspace


def stale_slot(x, out, ws):
    part = ws[: 4 * x.numel()].view(torch.float32)
    part[1:].copy_(x.reshape(-1)[1:] * 2)    # slot 0 is accumulated into, never zeroed
    part[0] += 2 * x.reshape(-1)[0]
    out.copy_((part + 1).view_as(x))


def _hole_binding():
    """``hole`` needs the entry content of its output: this binding simply never writes the last element."""
    mod = types.ModuleType("fake_binding_hole")
    mod.torch = torch

    def call(x):
        t = mod.torch
        ws = t.empty(4 * x.numel() + 256, dtype=t.uint8, device=x.device)
        out = t.empty_like(x)
        tmp = torch.empty_like(x)
        clean(x, tmp, ws)
        out.reshape(-1)[:-1] = tmp.reshape(-1)[:-1]
        return [out]
    mod.call = call
    return mod


X = torch.arange(1, 25, dtype=torch.float32).reshape(2, 3, 4) / 8


def test_clean_entry_is_accepted(monkeypatch):
    mod, stats = _binding(clean), {}
    outs = bh.run_three(lambda: mod.call(X), mod, monkeypatch, "clean", stats)
    assert torch.equal(outs[0], X * 2 + 1)
    assert stats == {"runs": 2, "allocations": 4, "uint8": 2, "uint8_bytes": 4 * 24 + 256, "foreign": 0, "last_uint8": [4 * 24 + 256]}
    assert mod.torch is torch, "the proxy is gone after the run"


def test_overrun_is_rejected(monkeypatch):
    mod = _binding(overrun)
    with pytest.raises(bh.HygieneError, match=r"writes stay inside.*allocation 0 \(empty, 352 bytes of torch.uint8\): 0 guard bytes changed before "
                                              r"the payload, 4 after"):
        bh.run_three(lambda: mod.call(X), mod, monkeypatch, "overrun")
    assert mod.torch is torch


def test_overrun_of_the_fill_value_itself_shows_in_the_other_run(monkeypatch):
    """A stray write of 0x00 is invisible on 0x00: that is why there are two fills."""
    def zero_past(x, out, ws):
        clean(x, out, ws)
        storage = torch.empty(0, dtype=torch.uint8).set_(ws.untyped_storage())
        storage[ws.storage_offset() - 2: ws.storage_offset()] = 0
    mod = _binding(zero_past)
    bh.run_guarded(lambda: mod.call(X), 0x00, mod, monkeypatch)
    with pytest.raises(bh.HygieneError, match="writes stay inside.*2 guard bytes changed before the payload, 0 after"):
        bh.run_guarded(lambda: mod.call(X), 0xFF, mod, monkeypatch)


def test_unwritten_output_element_is_rejected(monkeypatch):
    mod = _hole_binding()
    with pytest.raises(bh.HygieneError, match=r"prior contents do not matter: hole: output 0 \(2, 3, 4\) differs between the 0x00 and the 0xFF "
                                              r"run \(1 of 24 elements, the first at flat index 23\)"):
        bh.run_three(lambda: mod.call(X), mod, monkeypatch, "hole")


def test_stale_workspace_slot_is_rejected(monkeypatch):
    mod = _binding(stale_slot)
    with pytest.raises(bh.HygieneError, match=r"prior contents do not matter: stale: output 0 .* differs between the 0x00 and the 0xFF run "
                                              r"\(1 of 24 elements, the first at flat index 0\)"):
        bh.run_three(lambda: mod.call(X), mod, monkeypatch, "stale")


def test_nonfinite_rule_names_its_property():
    """An entry that reads poison in both guarded runs alike (a count of slots, say) gives equal bits on 0x00 and 0xFF only by luck; where
    the 0xFF run alone is non-finite the message names the read."""
    good, nan = [X.clone()], [torch.full_like(X, float("nan"))]
    with pytest.raises(bh.HygieneError, match="nothing unwritten is read"):
        bh.check_three(good, nan, nan, "nan")
    with pytest.raises(bh.HygieneError, match="plain and the guarded"):
        bh.check_three(good, [X + 1], [X + 1], "moved")
    bh.check_three(nan, nan, nan, "nan everywhere")       # the plain run's own NaNs are the entry's business, and compare by bits


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x5A])
def test_payload_offset_alignment_and_guards(fill):
    mod = types.ModuleType("m")
    mod.torch = torch
    with bh.proxied(mod, fill) as proxy:
        t = mod.torch
        made = [t.empty(7, dtype=t.uint8, device="cpu"), t.empty((3, 5), dtype=t.float64, device="cpu"), t.empty(2, 3, dtype=t.float16, device="cpu"),
                t.empty_like(X), t.zeros(5, dtype=t.float64, device="cpu"), t.zeros_like(X), t.full((4, 2), float("nan"), dtype=t.float64, device="cpu"),
                t.full((3,), 7, dtype=t.int32, device="cpu"), t.empty(0, dtype=t.float32, device="cpu")]
        assert [tuple(m.shape) for m in made] == [(7,), (3, 5), (2, 3), (2, 3, 4), (5,), (2, 3, 4), (4, 2), (3,), (0,)]
        assert [m.dtype for m in made] == [t.uint8, t.float64, t.float16, t.float32, t.float64, t.float32, t.float64, t.int32, t.float32]
        assert len(proxy.ledger) == len(made)
        for m, rec in zip(made, proxy.ledger):
            assert (m.data_ptr() - rec.whole.data_ptr() == bh.GUARD or not m.numel()) and rec.payload_range == (bh.GUARD, bh.GUARD + m.numel() * m.element_size())
            assert m.data_ptr() % bh.GRANULE == 0 and bh.GUARD % bh.GRANULE == 0
            assert rec.whole.numel() == rec.nbytes + 2 * bh.GUARD and rec.whole.dtype == torch.uint8 and rec.dtype == m.dtype
            assert all(bool((g == fill).all()) and g.numel() == bh.GUARD for g in rec.guards()), "zeros and full write the payload only"
            assert proxy.owns(m)
        assert not proxy.owns(X)
        poison = torch.tensor([fill] * 8, dtype=torch.uint8)
        assert bool((made[0] == fill).all()) and made[1].view(torch.uint8).reshape(-1)[:8].equal(poison), "empty: the payload holds the fill"
        assert bool((made[4] == 0).all()) and bool((made[5] == 0).all()) and bool(made[6].isnan().all()) and bool((made[7] == 7).all())
        proxy.check_guards()
    if fill == 0xFF:
        assert bool(made[1].isnan().all()) and bool(made[2].isnan().all()) and bool(made[3].isnan().all()), "all ones is a NaN in every float"


def test_everything_else_is_the_real_torch():
    proxy = bh.TorchProxy(0)
    assert proxy.Tensor is torch.Tensor and proxy.cuda is torch.cuda and proxy.cuda.device is torch.cuda.device
    assert proxy.float32 is torch.float32 and proxy.uint8 is torch.uint8 and proxy.float64 is torch.float64 and proxy.device is torch.device
    assert proxy.ones is torch.ones and proxy.from_numpy is torch.from_numpy and proxy.no_grad is torch.no_grad
    assert isinstance(X, proxy.Tensor)
    with pytest.raises(AttributeError):
        proxy.no_such_function
    pinned = proxy.empty(3, dtype=torch.float32, layout=torch.strided)      # a call that asks for more than dtype and device is torch's own
    assert not proxy.ledger and pinned.shape == (3,)


def test_same_bits_compares_nans_by_pattern():
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert bh.same_bits(a, a.clone()) and not torch.equal(a, a.clone())
    assert not bh.same_bits(a, torch.tensor([1.0, float("nan"), 0.0])), "-0 and +0 differ in bits"
    quiet = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert not bh.same_bits(quiet, torch.tensor([float("nan")])), "two NaNs of different payload"
    assert not bh.same_bits(a, a.double()) and not bh.same_bits(a, a[:2])
    assert bh.same_bits(a.double(), a.double()) and bh.same_bits(a.half(), a.half()) and bh.same_bits(a.to(torch.uint8), a.to(torch.uint8))


def test_flat_takes_nested_results():
    got = bh.flat((X, None, [X, (None, X)]))
    assert bh.flat(None) == [] and len(got) == 3 and all(t is X for t in got) and bh.flat(X)[0] is X
