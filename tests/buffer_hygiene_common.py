"""Shared by tests/test_host_buffer_hygiene.py and tests/test_gpu_buffer_hygiene.py: the harness that pins the contract on caller-owned
memory ("Caller-owned buffers").  Every native entry works in buffers that the binding (i2v_native.py) takes from torch: a
workspace, a ``saved`` buffer, the outputs.  The harness replaces the name ``torch`` in the binding's globals by a proxy whose ``empty``,
``empty_like``, ``zeros``, ``zeros_like`` and ``full`` allocate GUARD bytes more on each side, fill the WHOLE allocation with one byte and
hand out the middle.  A case runs three times -- plain, on 0x00 and on 0xFF (a NaN in fp16, fp32 and fp64, -1 in an integer) -- and

  writes stay inside        every guard byte still holds the fill byte after the run,
  prior contents are moot   the three runs return the same bits; a slot that nobody wrote shows as 0x00 against 0xFF,
  nothing unwritten is read no returned float is non-finite unless the plain run's is (0xFF poison propagates as NaN).

GUARD is a condition, not a measurement: 64 KiB is more than any row or tile of the small cases, and a multiple of 256, so the payload
lies on a boundary of the workspace carver's granule inside the allocator's 512-byte-aligned block -- and on no stronger one by design
of the caller (the allocator may still give more)."""
import contextlib

import torch

GUARD = 64 * 1024
GRANULE = 256
WRAPPED = ("empty", "empty_like", "zeros", "zeros_like", "full")


class HygieneError(AssertionError):
    """One property of the contract is broken; the message starts with the property's name."""


class Allocation:
    """One proxy allocation: ``whole`` = [guard | payload | guard] as uint8, all of it pre-filled with ``fill``."""

    def __init__(self, whole, nbytes, dtype, fill, what):
        self.whole, self.nbytes, self.dtype, self.fill, self.what = whole, nbytes, dtype, fill, what

    @property
    def payload_range(self):
        return GUARD, GUARD + self.nbytes

    def payload(self):
        return self.whole[GUARD: GUARD + self.nbytes]

    def guards(self):
        return self.whole[:GUARD], self.whole[GUARD + self.nbytes:]


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class TorchProxy:
    """Stands for the module ``torch``: every attribute is the real one's but the five allocating functions."""

    def __init__(self, fill):
        if not 0 <= int(fill) <= 255:
            raise ValueError("the fill is one byte")
        self.fill, self.ledger = int(fill), []

    def __getattr__(self, name):           # only reached for what the instance does not define itself
        return getattr(torch, name)

    # ------------------------------------------------------------------------------------------------------------------ allocation
    def _guarded(self, shape, dtype, device, what):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        device = torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        itemsize = torch.empty((), dtype=dtype).element_size()
        nbytes = _numel(shape) * itemsize
        raw = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
        if raw.data_ptr() % GRANULE:        # the host allocator aligns to 64 bytes only: take a 256-aligned window of a larger block
            raw = torch.empty(nbytes + 2 * GUARD + GRANULE, dtype=torch.uint8, device=device)
            skip = -raw.data_ptr() % GRANULE
            raw = raw[skip: skip + nbytes + 2 * GUARD]
        raw.fill_(self.fill)
        rec = Allocation(raw, nbytes, dtype, self.fill, what)
        self.ledger.append(rec)
        return rec.payload().view(dtype).view(tuple(int(s) for s in shape))

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            return tuple(size[0])
        return tuple(size)

    @staticmethod
    def _plain(kwargs):
        """True where the call asks for nothing but dtype and device: anything else (pinned memory, a layout, ``out=``) is torch's own."""
        return not set(kwargs) - {"dtype", "device"}

    def empty(self, *size, **kwargs):
        if not self._plain(kwargs):
            return torch.empty(*size, **kwargs)
        return self._guarded(self._shape(size), kwargs.get("dtype"), kwargs.get("device"), "empty")

    def zeros(self, *size, **kwargs):
        if not self._plain(kwargs):
            return torch.zeros(*size, **kwargs)
        return self._guarded(self._shape(size), kwargs.get("dtype"), kwargs.get("device"), "zeros").zero_()

    def full(self, size, fill_value, **kwargs):
        if not self._plain(kwargs):
            return torch.full(size, fill_value, **kwargs)
        dtype = kwargs.get("dtype")
        if dtype is None:
            dtype = torch.full((), fill_value).dtype
        return self._guarded(tuple(size), dtype, kwargs.get("device"), "full").fill_(fill_value)

    def empty_like(self, t, **kwargs):
        if not self._plain(kwargs):
            return torch.empty_like(t, **kwargs)
        return self._guarded(tuple(t.shape), kwargs.get("dtype", t.dtype), kwargs.get("device", t.device), "empty_like")

    def zeros_like(self, t, **kwargs):
        if not self._plain(kwargs):
            return torch.zeros_like(t, **kwargs)
        return self._guarded(tuple(t.shape), kwargs.get("dtype", t.dtype), kwargs.get("device", t.device), "zeros_like").zero_()

    # ------------------------------------------------------------------------------------------------------------------ the checks
    def damaged(self):
        """[(index in the ledger, record, bytes changed in the guard before, after)] of the allocations whose guards no longer hold the fill."""
        if not self.ledger:
            return []
        bad = []
        for device in {r.whole.device for r in self.ledger}:        # one transfer per device, not one per allocation
            idx = [i for i, r in enumerate(self.ledger) if r.whole.device == device]
            counts = torch.stack([torch.stack([(g != self.ledger[i].fill).sum() for g in self.ledger[i].guards()]) for i in idx]).tolist()
            bad += [(i, self.ledger[i], int(a), int(b)) for i, (a, b) in zip(idx, counts) if a or b]
        return sorted(bad, key=lambda e: e[0])

    def check_guards(self):
        bad = self.damaged()
        if bad:
            lines = [f"allocation {i} ({r.what}, {r.nbytes} bytes of {r.dtype}): {a} guard bytes changed before the payload, {b} after"
                     for i, r, a, b in bad]
            raise HygieneError(f"writes stay inside: fill 0x{self.fill:02X}: " + "; ".join(lines))

    def owns(self, t):
        """True where ``t`` lives in the payload of an allocation of this proxy."""
        if not t.numel():            # (an empty tensor has no address)
            return True
        lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        for r in self.ledger:
            base = r.whole.data_ptr() + GUARD
            if r.whole.device == t.device and base <= lo and hi <= base + r.nbytes:
                return True
        return False

    def count(self, dtype):
        return sum(1 for r in self.ledger if r.dtype == dtype)


@contextlib.contextmanager
def proxied(module, fill, monkeypatch=None):
    """Replaces the name ``torch`` in ``module``'s globals by a TorchProxy for the block; gives the proxy."""
    proxy = TorchProxy(fill)
    if monkeypatch is not None:
        with monkeypatch.context() as m:
            m.setattr(module, "torch", proxy)
            yield proxy
    else:
        real = module.torch
        module.torch = proxy
        try:
            yield proxy
        finally:
            module.torch = real


def _sync(tensors):
    if torch.cuda.is_available() and any(t.is_cuda for t in tensors if t is not None):
        torch.cuda.synchronize()


def flat(outs):
    """The tensors of a case's result (a tensor, or nested tuples / lists of tensors and None) in order."""
    if outs is None:
        return []
    if isinstance(outs, torch.Tensor):
        return [outs]
    return [t for o in outs for t in flat(o)]


def run_guarded(case, fill, module, monkeypatch=None, stats=None):
    """Runs ``case`` (a callable that builds its own fresh handle and returns tensors) with ``module``'s allocations guarded and filled with
    ``fill``, waits for the device, checks every guard byte of the ledger and gives the outputs.  ``stats`` (a dict) collects, for the
    ledger test, the number of uint8 allocations (workspaces and ``saved`` buffers: ``last_uint8`` holds this run's sizes, which are what the
    ``*_bytes`` functions reported) and of outputs that the proxy did not make."""
    with proxied(module, fill, monkeypatch) as proxy:
        outs = flat(case())
        _sync([r.whole for r in proxy.ledger])
        proxy.check_guards()
        if stats is not None:
            stats["runs"] = stats.get("runs", 0) + 1
            stats["allocations"] = stats.get("allocations", 0) + len(proxy.ledger)
            stats["uint8"] = stats.get("uint8", 0) + proxy.count(torch.uint8)
            stats["uint8_bytes"] = max(stats.get("uint8_bytes", 0), max([r.nbytes for r in proxy.ledger if r.dtype == torch.uint8], default=0))
            stats["foreign"] = stats.get("foreign", 0) + sum(1 for t in outs if not proxy.owns(t))
            stats["last_uint8"] = [r.nbytes for r in proxy.ledger if r.dtype == torch.uint8]
        outs = [t.clone() for t in outs]       # the ledger (and with it the guarded storage) ends with this call
    return outs


_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def same_bits(a, b):
    """Bit for bit, through integer views: NaNs compare by their pattern."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def _diff(a, b):
    d = bits(a) != bits(b)
    first = int(torch.nonzero(d.reshape(-1))[0])
    return f"{int(d.sum())} of {d.numel()} elements, the first at flat index {first}"


def check_three(plain, zeros, ones, name="case"):
    """The assertions on the three runs' outputs (lists of tensors in one order); each message starts with the property."""
    plain, zeros, ones = flat(plain), flat(zeros), flat(ones)
    if not (len(plain) == len(zeros) == len(ones)):
        raise HygieneError(f"prior contents do not matter: {name}: {len(plain)} / {len(zeros)} / {len(ones)} returned tensors")
    for i, (p, z, o) in enumerate(zip(plain, zeros, ones)):
        if p.shape != z.shape or p.shape != o.shape or p.dtype != z.dtype or p.dtype != o.dtype:
            raise HygieneError(f"prior contents do not matter: {name}: output {i} is {tuple(p.shape)} {p.dtype} plain, {tuple(z.shape)} {z.dtype} "
                               f"on 0x00, {tuple(o.shape)} {o.dtype} on 0xFF")
        if not same_bits(z, o):
            raise HygieneError(f"prior contents do not matter: {name}: output {i} {tuple(z.shape)} differs between the 0x00 and the 0xFF run "
                               f"({_diff(z, o)}): a slot is read or returned that this call did not write")
        if o.is_floating_point() and not bool(torch.isfinite(o).all()) and bool(torch.isfinite(p).all()):
            raise HygieneError(f"nothing unwritten is read: {name}: output {i} {tuple(o.shape)} has {int((~torch.isfinite(o)).sum())} non-finite "
                               "values on 0xFF and none in the plain run")
        if not same_bits(p, o):
            raise HygieneError(f"prior contents do not matter: {name}: output {i} {tuple(p.shape)} differs between the plain and the guarded runs "
                               f"({_diff(p, o)})")


def run_three(case, module, monkeypatch=None, name="case", stats=None):
    """Plain, guarded on 0x00, guarded on 0xFF; the contract's assertions; -> the 0xFF run's outputs (for the family's float64 gate)."""
    plain = [t.clone() for t in flat(case())]
    _sync(plain)
    zeros = run_guarded(case, 0x00, module, monkeypatch, stats)
    ones = run_guarded(case, 0xFF, module, monkeypatch, stats)
    check_three(plain, zeros, ones, name)
    return ones
