"""Two-stage pipelining of the sampling path over a stream of batches (generate_samples.py:44-54 loops over batches of
start frames): the cINN inverse pass of batch k+1 -- an 82-launch dependent chain that leaves most of the chip idle --
runs on a high-priority side stream underneath the decoder pass(es) of batch k.

    pf = LatentPrefetcher(lambda res, emb: flow(res, emb, reverse=True))
    t = pf.submit(res_0, emb_0)
    for k in range(n):
        z = pf.get(t)
        if k + 1 < n: t = pf.submit(res_{k+1}, emb_{k+1})     # enqueued before the decoder of batch k
        frames_k = decoder(x0_k, z)

Every batch still gets exactly one cINN pass and one decoder run; only the order of enqueueing changes, and the latent
draws keep the order of the serial loop."""
import os

import torch


class LatentPrefetcher:
    def __init__(self, latent_fn, device=None, enabled=True):
        self.latent_fn = latent_fn
        self.enabled = bool(enabled) and torch.cuda.is_available()
        # high priority: the chain's 82 small dependent launches get their workgroups dispatched in front of the decoder's big grids
        # (I2V_PREFETCH_PRIO=0: same priority as the caller's stream, for A/B runs)
        prio = int(os.environ.get("I2V_PREFETCH_PRIO", "-1"))
        self.stream = torch.cuda.Stream(device=device, priority=prio) if self.enabled else None

    def mark(self):
        """An event on the current stream: "everything enqueued so far is complete".  Pass it to ``submit(..., _ready=ev)`` when the
        arguments of the next pass are complete NOW but the submit itself comes later (behind the decoder's launches, see the
        shared-side-stream order below) -- the pass then does not wait for those launches."""
        if not self.enabled:
            return None
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def submit(self, *args, _ready=None, **kwargs):
        """Enqueue ``latent_fn(*args)`` on the side stream (after everything already enqueued on the current stream, so
        the arguments are complete; or after the event ``_ready`` of an earlier ``mark()``).  Returns a ticket for ``get``.

        When the decoder shares this stream for its own side work (``Generator.share_side_stream(pf.stream)``: ONE side stream per
        job, what a rank of a multi-GPU job should run) the usual order -- submit batch k + 1, then the decoder of batch k -- stays:
        the decoder handle then runs its two tiny first SPADE levels inline, so the main chain does not wait for the pass queued in
        front of its side work.  ``_ready`` lets a caller enqueue the pass BEHIND the decoder's launches without making it wait for
        them (``ev = pf.mark(); frames = decoder(...); t = pf.submit(..., _ready=ev)``)."""
        if not self.enabled:
            return (self.latent_fn(*args, **kwargs), None)
        ready = _ready
        if ready is None:
            ready = torch.cuda.Event()
            ready.record()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            z = self.latent_fn(*args, **kwargs)
            done = torch.cuda.Event()
            done.record()
        for a in list(args) + list(kwargs.values()):
            if torch.is_tensor(a) and a.is_cuda:
                a.record_stream(self.stream)      # the caller may drop its reference while the side stream still reads it
        return (z, done)

    def get(self, ticket):
        """The latent of a ticket, usable on the current stream."""
        z, done = ticket
        if done is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(done)
            if torch.is_tensor(z):
                z.record_stream(cur)
        return z


class FrameSinkBudgetError(RuntimeError):
    """``FrameSink.add`` refused a batch: keeping it would exceed the sink's device byte budget.  The sink is unchanged and usable."""


class FrameSink:
    """Device-side output stage of a job: decoder frames in, interleaved ``uint8`` on the host out, without a blocking ``.cpu()`` per
    batch and without the numpy permute (kernels: csrc/i2v_frames.hip).

    ``mode="peak"`` -- the GIF strip / grid of ``convert_seq2gif`` / ``convert_grid2gif``, byte for byte.  The whole job is scaled by ONE
    peak, so nothing can be quantised before the last batch is in: ``add(seq)`` keeps the batch's fp32 frames on the device (a
    reference, no copy) and folds its maximum into the running device peak; ``finish()`` converts every kept batch into its column
    block of one job-wide ``[T, K*H, cols*W, 3]`` device strip and starts ONE non-blocking copy into pinned memory; ``result()`` waits for
    that copy's event and returns the numpy view.  What is kept is bounded by ``budget_bytes`` (default: a quarter of the device memory
    free at construction); ``add`` raises ``FrameSinkBudgetError`` for a batch over it and leaves the sink as it was -- ``drain()`` hands
    the kept batches back so the caller can finish the job on the host path.

    ``mode="unit"`` -- ``to_uint8_clips`` of every batch (fixed scale, no peak): nothing is kept.  ``add(seq)`` converts at once into one of
    two device buffers and starts its copy into one of two pinned buffers on the sink's copy stream, so the copy of batch i runs under
    the decoder of batch i + 1; ``result()`` returns the OLDEST batch not yet collected as ``[n, T, H, W, 3]``.  At most two batches are
    in flight; a view returned by ``result()`` is valid until the next ``add``.

    Streams and lifetime: ``add`` / ``finish`` enqueue on the current stream, the copies run on ``self.stream``, ordered by events in both
    directions.  Only ``result()`` blocks the host.  The pinned buffers belong to the sink and are reused: a PEAK result is valid until
    the next ``finish()`` of the same sink, so copy what has to outlive it."""

    def __init__(self, mode="peak", budget_bytes=None, device=None, stream=None):
        if mode not in ("peak", "unit"):
            raise ValueError(f"FrameSink: mode must be 'peak' or 'unit', got {mode!r}")
        if budget_bytes is not None and (isinstance(budget_bytes, bool) or not isinstance(budget_bytes, int) or budget_bytes < 0):
            raise ValueError(f"FrameSink: budget_bytes must be an int >= 0, got {budget_bytes!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("FrameSink needs a HIP device (the host path is utils.auxiliaries.convert_seq2gif)")
        self.mode = mode
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.budget_bytes = torch.cuda.mem_get_info(self.device)[0] // 4 if budget_bytes is None else budget_bytes
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
        self._kept, self._kept_bytes, self._geom = [], 0, None
        self._peak = torch.empty(1, dtype=torch.float32, device=self.device)
        self._pinned = [None, None]      # host buffers (flat uint8, grown on demand)
        self._dev = [None, None]         # UNIT: device buffers of the two slots
        self._free = [None, None]        # UNIT: event "the copy out of slot s is done" (its device and pinned buffer may be rewritten)
        self._pending = []               # (slot, shape, event) of copies not yet collected, oldest first
        self._count = 0

    # ------------------------------------------------------------------------------------------------------------------ helpers
    def _host(self, slot, nbytes):
        if self._pinned[slot] is None or self._pinned[slot].numel() < nbytes:
            self._pinned[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self._pinned[slot][:nbytes]

    def _copy_out(self, slot, u8):
        """Start the device -> pinned copy of ``u8`` on the copy stream, behind everything enqueued on the current stream."""
        ready = torch.cuda.Event()
        ready.record()
        host = self._host(slot, u8.numel())
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            host.copy_(u8.view(-1), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        u8.record_stream(self.stream)
        self._pending.append((slot, tuple(u8.shape), done))
        return done

    # ---------------------------------------------------------------------------------------------------------------------- API
    def add(self, seq):
        """One batch of frames: a CUDA float32 ``[n, T, 3, H, W]`` strip block or ``[F, K, T, 3, H, W]`` grid block (sample blocks
        contiguous, any sample stride).  The caller must not overwrite ``seq`` before ``finish()`` (PEAK) / after this call returns the
        frames have been read by work enqueued on the current stream (UNIT)."""
        import i2v_native
        n, k, t, h, w, _ = i2v_native.frames_geometry(seq)
        if not seq.is_cuda or seq.device != self.device:
            raise i2v_native.I2VError(f"FrameSink.add: expected frames on {self.device}, got {seq.device}")
        if self.mode == "unit":
            if len(self._pending) >= 2:
                raise RuntimeError("FrameSink.add: two batches are in flight; collect one with result() first")
            slot = self._count % 2
            nbytes = seq.numel()
            if self._dev[slot] is None or self._dev[slot].numel() < nbytes:
                self._dev[slot] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if self._free[slot] is not None:
                torch.cuda.current_stream().wait_event(self._free[slot])   # the previous copy out of this slot has to be through
            u8 = self._dev[slot][:nbytes].view(*seq.shape[:-4], t, h, w, 3)
            i2v_native.frames_to_u8(seq, out=u8, mode="unit", layout="clips")
            self._free[slot] = self._copy_out(slot, u8)
            self._count += 1
            return
        geom = (k, t, h, w)
        if self._geom is not None and geom != self._geom:
            raise i2v_native.I2VError(f"FrameSink.add: batch geometry (K, T, H, W) = {geom} differs from the job's {self._geom}")
        nbytes = seq.numel() * 4 + seq.numel()          # the fp32 frames that stay + their share of the job-wide uint8 strip
        if self._kept_bytes + nbytes > self.budget_bytes:
            raise FrameSinkBudgetError(f"FrameSink: keeping this batch ({nbytes} bytes) on top of {self._kept_bytes} bytes exceeds the "
                                       f"budget of {self.budget_bytes} bytes; finish the job on the host path (drain())")
        i2v_native.frames_peak(seq, out=self._peak, accumulate=bool(self._kept))
        self._kept.append(seq)
        self._kept_bytes += nbytes
        self._geom = geom

    def drain(self):
        """PEAK mode: hand back the kept device batches (in ``add`` order) and empty the sink."""
        kept, self._kept, self._kept_bytes, self._geom = self._kept, [], 0, None
        return kept

    def finish(self):
        """PEAK mode: quantise every kept batch with the job's peak into one device strip and start its copy to the host."""
        import i2v_native
        if self.mode != "peak":
            raise RuntimeError("FrameSink.finish: UNIT mode converts in add(); collect with result()")
        if not self._kept:
            raise RuntimeError("FrameSink.finish: nothing was added")
        k, t, h, w = self._geom
        cols = [s.numel() // (k * t * 3 * h * w) for s in self._kept]
        strip = torch.empty(t, k * h, sum(cols) * w, 3, dtype=torch.uint8, device=self.device)
        col0 = 0
        for s, c in zip(self._kept, cols):
            i2v_native.frames_to_u8(s, peak=self._peak, out=strip, mode="peak", layout="strip", col0=col0)
            col0 += c * w
        slot = self._count % 2
        self._count += 1
        self._copy_out(slot, strip)
        self.drain()

    def result(self):
        """Wait for the oldest copy in flight and return its bytes as a numpy view of the pinned buffer."""
        if not self._pending:
            raise RuntimeError("FrameSink.result: no copy in flight (PEAK: call finish() first; UNIT: add() first)")
        slot, shape, done = self._pending.pop(0)
        done.synchronize()
        n = 1
        for d in shape:
            n *= d
        return self._pinned[slot][:n].numpy().reshape(shape)
