"""GPU parity: how the weight-gradient slabs leave wgrad_body (csrc/bwd_bodies.h).

Where both slab base pointers and split_stride are 16-byte aligned (and Cout % 4 == 0) the epilogues restage the
workgroup's tile through LDS and store 16 bytes per lane, write-through; any other placement keeps the 4-byte-per-lane
stores.  Both forms write the same sums in the same order, so ONE build pins the wide stores to the dword ones: the slabs
must be bit-identical whatever the placement.  Every member runs through the C ABI with the weight-gradient member only,
against the float64 oracle of test_bwd_launches.py (hiputil.BwdCase), tolerance as there:
  dW, db : max|err| <= 1e-4 * (1 + max|ref|)
Slabs are pre-filled with NaN (every element must be written); everything around them -- in front of the first slab,
between the slabs, behind the last -- holds a sentinel that must come back unchanged.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from lib import _hip
from test_bwd_launches import M, close

ALIGN_PAD = 8           # floats between two slabs in the placement runs (keeps 16-byte alignment; the misaligned stride adds 1)


class Placed:
    """The three outputs of a member's weight gradients somewhere of our choosing.  `tensors` = [(name, size, offset in a
    slab)]; slab s of a tensor starts at base + shift + s * stride.  Everything else in the buffer is sentinel."""

    def __init__(self, cs, shift, stride, offs, span):
        import hiputil as U
        self.cs, self.shift, self.stride, self.offs = cs, shift, stride, offs
        self.split = cs.split
        self.buf = U.Guarded(shift + (self.split - 1) * stride + span)
        self.mask = np.zeros(self.buf.size, bool)                 # True: an output element
        for s in range(self.split):
            for o, sz in zip(offs, cs.sizes):
                self.mask[shift + s * stride + o: shift + s * stride + o + sz] = True
        self.init = np.where(self.mask, np.float32(np.nan), np.float32(U.SENTINEL)).astype(np.float32)
        w = cs.w
        w.dwa = self.buf.ptr(shift + offs[0])
        w.dwv = self.buf.ptr(shift + offs[1]) if cs.sizes[1] else None
        w.db = self.buf.ptr(shift + offs[2])
        w.split_stride = stride

    def poison(self):
        self.buf.fill(self.init)

    def check_and_get(self):
        """[split][tensor] arrays; every output element written, nothing else touched."""
        import hiputil as U
        got = self.buf.get()
        assert self.buf.guards_ok(), 'a write outside the buffer'
        assert np.isfinite(got[self.mask]).all(), 'an output element was not written'
        assert (got[~self.mask] == np.float32(U.SENTINEL)).all(), \
            ('a write outside the tensors', np.flatnonzero((got != np.float32(U.SENTINEL)) & ~self.mask)[:8])
        return [[got[self.shift + s * self.stride + o: self.shift + s * self.stride + o + sz].copy()
                 for o, sz in zip(self.offs, self.cs.sizes)] for s in range(self.split)]


def launch(cs, entry):
    import hiputil as U
    lib = _hip.load()
    if entry == 'scale':
        _hip.check(lib.mpnn_msconv_bwd_scale(None, None, C.byref(cs.w), U.stream()), 'bwd_scale')
    else:
        _hip.check(lib.mpnn_msconv_wgrad(C.byref(cs.w), U.stream()), 'wgrad')


def packed(cs, shift, stride_extra):
    """dwa | dwv | db back to back (the planner's layout), slabs ALIGN_PAD (+ stride_extra) floats apart."""
    total = sum(cs.sizes)
    stride = (total + 3) // 4 * 4 + ALIGN_PAD + stride_extra
    return Placed(cs, shift, stride, cs.offs, total)


def check_oracle(cs, slabs):
    """The slabs summed in slab order (float64 on the host: exact enough for the tolerance) against the oracle."""
    refs = [cs.dwa_ref.reshape(-1), cs.dwv_ref.reshape(-1) if cs.dwv_ref is not None else None, cs.db_ref]
    for k, (name, ref) in enumerate(zip(('dWa', 'dWv', 'db'), refs)):
        if ref is not None:
            close(sum(np.asarray(s[k], np.float64) for s in slabs), ref, 1e-4, name)


def same_slabs(a, b, what):
    for s, (sa, sb) in enumerate(zip(a, b)):
        for k, (ta, tb) in enumerate(zip(sa, sb)):
            assert np.array_equal(ta, tb), (what, 'slab %d tensor %d' % (s, k), np.abs(ta - tb).max())


# (placement: floats past a 16-byte boundary, floats added to an aligned stride)
PLACEMENTS = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1)]

MEMBERS = {
    # NINE, OT == 4: 64-channel group at 4x4 (ragged n = 5: two tiles)
    'ot4_64_4x4': (M(5, 4, 4, 64, gctx=8, a=('bn', 64, 8), split=2), 'scale'),
    # NINE, OT == 1: 16-channel group at 8x8
    'ot1_16_8x8': (M(3, 8, 8, 16, a=('bn', 16, 8), split=3), 'scale'),
    # 32 channels at 4x4: two 16-channel groups in mpnn_msconv_bwd_scale; the tap-slot form (OT == 2) in mpnn_msconv_wgrad
    'c32_4x4_scale': (M(5, 4, 4, 32, a=('bn', 32, 8), split=2), 'scale'),
    'tapslot_32_4x4': (M(5, 4, 4, 32, a=('bn', 32, 8), split=2), 'wgrad'),
    # SMALLC: image operands
    'smallc_img3_16x16': (M(2, 16, 16, 16, a=('img', 3, 0), split=3), 'scale'),
    'smallc_img1_16x16': (M(2, 16, 16, 16, gctx=8, a=('img', 1, 1), split=3), 'scale'),
    # a vertical operand
    'vert_16_8x8': (M(3, 8, 8, 16, a=('bn', 16, 8), Cv=16, split=2), 'scale'),
    'vert_64_4x4': (M(5, 4, 4, 64, a=('bn', 32, 8), Cv=64, split=2), 'scale'),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(MEMBERS))
def test_wide_stores_equal_dword_stores(name):
    """The slab base on a 16-byte boundary (the wide stores), 1, 2 and 3 floats past one, and an aligned base with a
    split_stride that is no multiple of 4 floats (the dword stores): bit-identical slabs."""
    import hiputil as U
    spec, entry = MEMBERS[name]
    cs = U.BwdCase(np.random.default_rng(zlib.crc32(name.encode())), spec)
    assert cs.split >= 2
    first = None
    for shift, extra in PLACEMENTS:
        pl = packed(cs, shift, extra)
        pl.poison()
        launch(cs, entry)
        torch.cuda.synchronize()
        slabs = pl.check_and_get()
        check_oracle(cs, slabs)
        if first is None:
            first = slabs
        else:
            same_slabs(first, slabs, 'shift %d, stride + %d' % (shift, extra))


TAILS = {
    'ot1_C20_Cv24': (M(3, 8, 8, 16, a=('bn', 20, 8), Cv=24, split=3), 'scale'),
    'ot1_C36_Cv24': (M(5, 4, 4, 16, gctx=8, a=('bn', 36, 8), Cv=24, split=2), 'scale'),
    'ot4_C20_Cv24': (M(5, 4, 4, 64, a=('bn', 20, 8), Cv=24, split=2), 'scale'),
    'ot4_C36_Cv24': (M(3, 8, 8, 64, a=('bn', 36, 8), Cv=24, split=3), 'scale'),
    'tapslot_C20_Cv24': (M(5, 4, 4, 32, a=('bn', 20, 8), Cv=24, split=2), 'wgrad'),
    'tapslot_C36_Cv24': (M(3, 8, 8, 32, a=('bn', 36, 8), Cv=24, split=3), 'wgrad'),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(TAILS))
def test_channel_tails(name):
    """Channel counts whose last 16-chunk is partial (rows cin >= C of the chunk must not be stored).  split_stride is
    exactly the largest tensor's size: behind that tensor comes the next slab, behind its last slab the guard; each
    tensor lives in a region of its own, so behind the smaller ones the sentinel starts at once -- a row stored beyond
    [9][C][Cout] changes a sentinel, another slab's rows (the oracle) or the guard.  Aligned, so the wide stores run;
    one float further, the dword stores: the same bits."""
    import hiputil as U
    spec, entry = TAILS[name]
    cs = U.BwdCase(np.random.default_rng(zlib.crc32(name.encode())), spec)
    stride = max(cs.sizes)
    assert stride % 4 == 0
    region = cs.split * stride + 4                       # (+ 4: the misaligned run's tensors stay apart too)
    offs = [0, region, 2 * region]
    runs = []
    for shift in (0, 1):
        pl = Placed(cs, shift, stride, offs, 2 * region + cs.sizes[2])
        pl.poison()
        launch(cs, entry)
        torch.cuda.synchronize()
        runs.append(pl.check_and_get())
        check_oracle(cs, runs[-1])
    same_slabs(runs[0], runs[1], 'aligned vs one float further')


@pytest.mark.gpu
def test_xcd_aware_tile_order():
    """n = 32 with a split of 8 takes the XCD-aware tile order (the member of test_bwd_launches' g7_four)."""
    import hiputil as U
    cs = U.BwdCase(np.random.default_rng(77), M(32, 16, 16, 16, a=('bn', 16, 8), Cv=16, split=8))
    assert cs.split == 8
    runs = []
    for shift, extra in [(0, 0), (1, 0), (0, 2)]:
        pl = packed(cs, shift, extra)
        pl.poison()
        launch(cs, 'scale')
        torch.cuda.synchronize()
        runs.append(pl.check_and_get())
        check_oracle(cs, runs[-1])
    same_slabs(runs[0], runs[1], 'aligned vs misaligned base')
    same_slabs(runs[0], runs[2], 'aligned vs misaligned stride')


@pytest.mark.gpu
def test_write_then_reduce_in_one_graph():
    """The weight-gradient launch and mpnn_slab_reduce on one stream, captured as ONE graph and replayed four times:
    fresh inputs and a poisoned slab buffer before every replay.  The reduced gradient equals, bit for bit, the fixed-order
    sum of the slabs read back (mpnn_slab_reduce's order, restated on the host in fp32), and the oracle."""
    import hiputil as U
    lib = _hip.load()
    spec = M(5, 4, 4, 64, a=('bn', 64, 8), Cv=64, split=2)
    rng = np.random.default_rng(4242)
    cases = [U.BwdCase(rng, spec) for _ in range(4)]            # four sets of inputs (and their references), made once
    cs = cases[0]                                               # its argument record and buffers are the captured ones
    total = sum(cs.sizes)
    stride = (total + 3) // 4 * 4
    pl = Placed(cs, 0, stride, cs.offs, total)
    grads = U.Guarded(total)
    tab = []
    for o, sz in zip(cs.offs, cs.sizes):
        for k in range(0, sz, _hip.slab_item_size(cs.split)):
            tab += [o + k, o + k, min(_hip.slab_item_size(cs.split), sz - k), cs.split, stride, 0]
    tab_d = U.dev(np.array(tab, np.int32), torch.int32)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    pl.poison()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        st = torch.cuda.current_stream().cuda_stream
        _hip.check(lib.mpnn_msconv_bwd_scale(None, None, C.byref(cs.w), st), 'bwd_scale')
        _hip.check(lib.mpnn_slab_reduce(pl.buf.ptr(), grads.ptr(), tab_d.data_ptr(), len(tab) // 6, st), 'slab_reduce')

    def replay(src):
        if src is not cs:                                       # fresh inputs into the captured buffers
            cs.gd.copy_(src.gd)
            cs.abn.sd.copy_(src.abn.sd)
            for k in ('sum', 'gamma', 'beta'):
                cs.abn.dev[k].copy_(src.abn.dev[k])
            cs.vd.copy_(src.vd)
        pl.poison()
        grads.fill(np.nan)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        slabs = pl.check_and_get()
        assert grads.guards_ok()
        got = grads.get()
        # mpnn_slab_reduce at a split of 2: item quads * 2 groups <= 256 or not, the sum of two slabs is slab 0 + slab 1
        # either way (0 + s0, then + s1: one fp32 addition, whose result does not depend on the grouping)
        want = np.concatenate([(slabs[0][k] + np.float32(0)) + slabs[1][k] for k in range(3)])
        assert np.array_equal(got, want), np.abs(got - want).max()
        close(got[:cs.sizes[0]], src.dwa_ref.reshape(-1), 1e-4, 'dWa')
        close(got[cs.offs[1]:cs.offs[2]], src.dwv_ref.reshape(-1), 1e-4, 'dWv')
        close(got[cs.offs[2]:], src.db_ref, 1e-4, 'db')

    replay(cases[0])
    replay(cases[1])
    replay(cases[2])
    replay(cases[3])
