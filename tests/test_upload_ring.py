"""GPU: the ring of pinned upload buffers (lib/_upload.py) alone, with no net.

  * the host may not overtake the device: six uploads through a ring of TWO buffers, all queued behind a 2 ms spin kernel,
    each deliver their own values -- a ring that did not wait for the event behind a buffer's last copy would let the host
    rewrite buffer i % 2 before its copy ran (every log would read 4 or 5).  In the three forms the consumers use:
    upload(), acquire / fill in place / release, and the release recorded on a side stream;
  * the repeated-values cache: equal values are not sent again; a changed value, a changed shape, forget() -- and values
    the caller rewrote in place after sending them -- are;
  * drain, then a larger ring, while uploads are pending behind a spin: the pending uploads deliver their own values.

Every comparison is exact (the values are small integers)."""
import pytest
import torch

from lib import _hip
from lib._upload import UploadRing, ValueRing

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def spin(stream=None):
    """~2 ms of one workgroup on the stream: everything queued behind it is still pending while the host goes on."""
    st = torch.cuda.current_stream() if stream is None else stream
    _hip.check(_hip.load().mpnn_debug_spin(1, 64, 2000.0, st.cuda_stream), 'debug_spin')


@pytest.mark.parametrize('form', ['upload', 'acquire', 'side'])
def test_host_does_not_overtake_the_device(form):
    torch.cuda.set_device(DEV)
    ring = UploadRing(2, (16,))
    dst = torch.zeros(16, device=DEV)
    log = torch.full((6, 16), -1.0, device=DEV)
    main = torch.cuda.current_stream()
    if form == 'side':
        # (the first launch on a stream binds its hardware queue, which takes longer than the spin: done before it starts)
        side = torch.cuda.Stream(device=DEV)
        _hip.check(_hip.load().mpnn_debug_noop(side.cuda_stream), 'debug_noop')
        side.synchronize()
    spin()
    if form == 'side':
        behind_spin = torch.cuda.Event()
        behind_spin.record(main)
        side.wait_event(behind_spin)
    for i in range(6):
        if form == 'upload':
            ring.upload(dst, torch.full((16,), float(i)))
            log[i].copy_(dst)
        elif form == 'acquire':
            buf = ring.acquire()
            buf.numpy()[:] = i                                 # (filled in place, as the draw functions do)
            dst.copy_(buf, non_blocking=True)
            log[i].copy_(dst)
            ring.release()
        else:
            buf = ring.acquire()
            buf.fill_(float(i))
            with torch.cuda.stream(side):
                dst.copy_(buf, non_blocking=True)
                log[i].copy_(dst)
            ring.release(side)
    torch.cuda.synchronize()
    assert torch.equal(log.cpu(), torch.arange(6.0)[:, None].expand(6, 16))


def test_partial_rows_upload():
    """upload() of fewer leading rows than the buffers hold (K of STEPS_MAX steps) moves those rows only."""
    torch.cuda.set_device(DEV)
    ring = UploadRing(2, (4, 3))
    dst = torch.full((4, 3), -1.0, device=DEV)
    src = torch.arange(6.0).reshape(2, 3)
    ring.upload(dst[:2], src)
    torch.cuda.synchronize()
    assert torch.equal(dst[:2].cpu(), src) and bool((dst[2:] == -1).all())


def test_repeated_values_are_sent_once():
    torch.cuda.set_device(DEV)
    ring = ValueRing(2, (4, 4))
    dst = torch.zeros(4, 4, device=DEV)
    v = torch.arange(8.0).reshape(2, 4)

    def lands(values, rows):
        torch.cuda.synchronize()
        return torch.equal(dst[:rows].cpu(), values)

    assert ring.send(dst[:2], v) is True and lands(v, 2)
    dst.fill_(-1.0)
    assert ring.send(dst[:2], v.clone()) is False               # equal values: no upload, the destination is untouched
    torch.cuda.synchronize()
    assert bool((dst == -1).all())
    v2 = v.clone()
    v2[1, 3] = 99.0
    assert ring.send(dst[:2], v2) is True and lands(v2, 2)      # a changed value
    v3 = torch.cat([v2, torch.full((1, 4), 7.0)])
    assert ring.send(dst[:3], v3) is True and lands(v3, 3)      # a changed shape (its leading rows are what was sent last)
    assert ring.send(dst[:3], v3) is False
    dst.fill_(-1.0)
    ring.forget()
    assert ring.send(dst[:3], v3) is True and lands(v3, 3)      # forget(): whatever was sent last
    v3[0, 0] = 5.0                                              # the caller rewrites ITS tensor in place (Runner._hyp_stage)
    assert ring.send(dst[:3], v3) is True and lands(v3, 3)


def test_drain_then_a_larger_ring_while_uploads_are_pending():
    torch.cuda.set_device(DEV)
    ring = UploadRing(2, (4,))
    dst, log = torch.zeros(4, device=DEV), torch.full((2, 4), -1.0, device=DEV)
    spin()
    for i in range(2):
        ring.upload(dst, torch.full((4,), float(i + 1)))
        log[i].copy_(dst)
    ring.drain()                                                # the host waits here for the spin and both copies
    assert all(ev.query() for ev in ring.events)
    for buf in ring.bufs:                                       # (after drain the buffers are the host's again)
        buf.fill_(-7.0)
    ring = UploadRing(2, (32,))
    dst2, log2 = torch.zeros(32, device=DEV), torch.full((3, 32), -1.0, device=DEV)
    spin()
    for i in range(3):
        ring.upload(dst2, torch.full((32,), float(i + 10)))
        log2[i].copy_(dst2)
    torch.cuda.synchronize()
    assert torch.equal(log.cpu(), torch.tensor([1.0, 2.0])[:, None].expand(2, 4))
    assert torch.equal(log2.cpu(), torch.tensor([10.0, 11.0, 12.0])[:, None].expand(3, 32))
