"""Asynchronous host-to-device uploads through a ring of pinned buffers, and the step-by-step fallback of the K-step graphs.

Why a ring, and why the event: a copy from pinned memory is asynchronous and, under hipGraph replay, the host runs many
steps ahead of the stream -- rewriting ONE staging buffer in place would let step t's DMA read the values of step t + k
(its learning rate, its augmentation draws: nothing faults, no tolerance trips).  So every upload takes the next of
`depth` buffers, and a buffer is rewritten only after the event recorded behind its last copy has completed.  This module
is the only place in lib/ that knows the rule; every consumer keeps a ring of its own shape, depth and lifetime."""
import torch


class UploadRing:
    """`depth` pinned host buffers of one shape and dtype, each with the event behind its last use.

        buf = ring.acquire()          # the next buffer; the host waits here until the device has read its last contents
        ... fill buf, issue dst.copy_(buf, non_blocking=True) -- one copy or several ...
        ring.release()                # the event behind those copies (on the current stream, or on `stream`)

    or, for one host tensor into one device tensor, ring.upload(dst, src)."""

    def __init__(self, depth, shape, dtype=torch.float32):
        self.bufs = [torch.zeros(tuple(shape), dtype=dtype, pin_memory=True) for _ in range(depth)]
        self.events = [None] * depth
        self.at = -1
        self.rows = self.bufs[0].shape[0]          # (consumers replace a ring whose buffers have too few rows)

    def acquire(self):
        self.at = (self.at + 1) % len(self.bufs)
        ev = self.events[self.at]
        if ev is not None:
            ev.synchronize()
        return self.bufs[self.at]

    def release(self, stream=None):
        """Behind the copies out of the acquired buffer.  Returns the event (predict_all makes its compute stream wait for it)."""
        ev = self.events[self.at] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream() if stream is None else stream)
        return ev

    def upload(self, dst, src):
        """dst (device) = src (host; its leading rows may be fewer than the buffers'), through the next buffer."""
        buf = self.acquire()[:src.shape[0]]
        buf.copy_(src)
        dst.copy_(buf, non_blocking=True)
        self.release()

    def drain(self):
        """Wait for every pending copy out of the ring (before it is dropped for a larger one)."""
        for ev in self.events:
            if ev is not None:
                ev.synchronize()


class ValueRing(UploadRing):
    """An UploadRing for values that mostly repeat from step to step (constant schedules): the upload is skipped while
    they do.  The owner calls forget() whenever something else rewrote the device copy."""
    sent = None

    def send(self, dst, values):
        """Upload `values` unless they are what was sent last (same shape, same contents); True if uploaded."""
        if self.sent is not None and torch.equal(values, self.sent):
            return False
        self.upload(dst, values)
        self.sent = values.clone()
        return True

    def forget(self):
        self.sent = None


def run_one_by_one(owner, run, steps, slots):
    """The steps of a run_steps call one call of run(step) at a time, where the K-step graph does not apply (or not yet).
    slots: the feeds are bound to the input pipeline, whose caller staged one record slot per step -- step j > 0 must gather
    from slot j, so it runs as eager launches with owner.prologue_slot(stream, j) as its prologue (slot 0 is what the
    one-step graph reads: step 0 takes the usual path)."""
    keep = owner.prologue, owner.use_graph
    try:
        for j, step in enumerate(steps):
            if slots and j > 0:
                owner.prologue, owner.use_graph = (lambda st, j=j: owner.prologue_slot(st, j)), False
            run(step)
    finally:
        owner.prologue, owner.use_graph = keep
