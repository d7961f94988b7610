"""The forward conv launch of co-training (csrc/conv_fwd.hip: mpnn_msconv_fwd_group_rep, and the REP forms of the first
conv in csrc/conv_first.hip) alone, through the C ABI, on the GPU, against float64 -- with the BatchNorm statistics
(out_sum) that every training launch carries.

tests/test_cotrain.py compares a co-trained net with the same net stepped alone under the SAME planner setting: both
sides run the same bodies on the same grids, and a fault they share cancels.  Here every launch of the table below is
held, per net and member, to
  a. buffers: guards intact, every out / pool_out element written, the slots >= out_nslot of out_sum still zero;
  b. float64 (oracle/np_ops.py): 2e-5 (identity / image operand) or 3e-5 (BatchNorm on load) x (1 + max |ref|), the
     limits of tests/test_hip_conv.py and tests/test_conv_fwd_lists.py; pool_out = the 2x2 max of the launch's own out;
  c. statistics: out_sum over its slots against the float64 sum and sum of squares, per channel, of the launch's OWN
     stored fp32 out (the kernels sum the values they store; (b) links those to the oracle): 1e-5 * sum |term| + 1e-9,
     _sum_close of tests/test_conv_hw.py.  It holds with room at the one-workgroup-per-tile-row grids a large share
     gives: the worst error / limit measured over the table is 0.008 (the 4x4 member of the two-member row at share
     32), 0.004 on the 32-channel tiles, below 0.001 on the strips;
  d. the header's contract: net r launched alone with reps = 1 and the row's share writes the bits of the joint launch,
     and every SLOT of out_sum agrees to 1e-12 relative (the same workgroups add the same fp32 partials to the same
     slot; only the order of the fp64 atomics differs).  The scale of the 1e-12 is max |a| over all slots and channels
     of the member plus |a| of the element, not the element alone, as in same_dgrad of tests/test_bwd_launches.py: a
     slot's sum of a channel may nearly cancel.  The other nets' buffers stay poisoned;
  e. mpnn_msconv_fwd on the same record: the same bits; the multi-chunk strip bodies sum in another order and are held
     to 2e-5 x (1 + max |one|), as tests/test_hip_conv.py::test_strip_conv_kernel_two_or_three_chunks holds them;
  f. a member of a multi-member row launched alone at the same reps / share: the same bits, its out_sum (another grid)
     held to (c).  The body the lone launch selects is asserted too, listed in the row where it is not the joint one:
     at share 32 the two Cout % 32 members alone run the 32-channel tile (the same bits), and in the one-net rows a
     deep 4x4 member alone takes the K-split body (another summation order over K), held to 2e-5 x (1 + max) as
     tests/test_hip_conv.py::test_one_member_group_equals_single_launch holds it.

Every net of a launch has its own inputs, weights, bias, BatchNorm statistics / gamma / beta and output buffers, so a
workgroup that reads or writes another net's record misses (a) or (b).  `body_of` restates the launcher's selection
with `share` and every member asserts the body it is listed for.

The refusals of the launcher (host side, nothing launches) are test_rep_argument_errors, without a GPU."""
import os

import numpy as np
import pytest

from lib import _hip
import test_conv_fwd_lists as L
from test_conv_fwd_lists import Member, launch

gpu = pytest.mark.gpu

# member: (H, W, Ca, act mode, shift, Cv, Cout, pool, out_nslot)
FIRST = (8, 16, 3, 'img', 0, 0, 16, True, 8)
FIRST1 = (4, 16, 1, 'img', 0, 0, 16, False, 1)
IMGV = (8, 16, 3, 'img', 1, 16, 16, True, 8)
B16V = (8, 16, 16, 'batch', 0, 16, 16, True, 5)
B16W = (8, 16, 16, 'batch', 0, 16, 32, True, 8)
B8 = (8, 8, 32, 'batch', 0, 16, 32, True, 16)
B4 = (4, 4, 64, 'batch', 0, 0, 32, False, 1)
B4V = (4, 4, 32, 'batch', 0, 32, 16, False, 8)
B4S = (4, 4, 64, 'batch', 0, 0, 32, False, 8)
DEEP4 = (4, 4, 128, 'batch', 0, 0, 128, False, 8)
B16 = (8, 16, 16, 'batch', 0, 0, 16, True, 8)
B32K3 = (4, 32, 32, 'batch', 0, 16, 16, False, 5)
PIMG = (16, 16, 3, 'img', 1, 16, 16, True, 8)
PB32 = (32, 32, 16, 'batch', 0, 0, 16, True, 8)
W8 = (8, 8, 32, 'batch', 0, 32, 64, True, 8)
W4 = (4, 4, 64, 'batch', 0, 0, 128, False, 16)
PW4 = (4, 4, 64, 'batch', 0, 64, 64, False, 8)
PW8 = (8, 8, 64, 'batch', 0, 0, 64, True, 8)

# name -> (members: (case, the body it is listed for[, the body it runs ALONE at the row's reps / share, where another]),
#          n, reps, share)
ROWS = {
    'first conv': ([(FIRST, 'first')], 5, 3, 3),
    'first conv, no pool, 1 channel': ([(FIRST1, 'first')], 7, 2, 8),
    'g16+small | g16': ([(IMGV, 'g16+small'), (B16V, 'g16')], 5, 3, 3),
    'four bodies': ([(B16W, 'g16'), (B8, 'g8'), (B4, 'g4'), (B4V, 'g4')], 5, 2, 4),
    'four bodies, one net, n 5': ([(B16W, 'g16'), (B8, 'g8'), (B4, 'g4', 'ks4'), (B4V, 'g4', 'ks4')], 5, 1, 1),
    'four bodies, one net, n 32': ([(B16W, 'g16'), (B8, 'g8'), (B4, 'g4', 'ks4'), (B4V, 'g4', 'ks4')], 32, 1, 1),
    'deep 4x4 alone': ([(DEEP4, 'g4')], 5, 3, 3),
    'strips by share': ([(IMGV, 'stripk+small'), (B16, 'strip16')], 22, 2, 24),
    'stripk, 2 and 3 chunks': ([(B16W, 'stripk'), (B32K3, 'stripk')], 22, 3, 24),
    'strips, production': ([(PIMG, 'stripk+small'), (PB32, 'strip16')], 128, 2, 4),
    'wide8 with statistics': ([(W8, 'wide8')], 37, 2, 32),
    'wide4 with statistics': ([(W4, 'wide4')], 37, 2, 32),
    'wide, production': ([(PW4, 'wide4')], 128, 2, 8),
    'two Cout%32 members (not wide)': ([(W8, 'g8', 'wide8'), (B4S, 'g4', 'wide4')], 37, 2, 32),
    'deep 8x8 alone, production': ([(PW8, 'wide8')], 128, 2, 8),
}
ORDER_DIFFERS = ('stripk', 'stripk+small', 'ks8', 'ks4')     # bodies that sum in another order than mpnn_msconv_fwd


def bodies_of(mcs, n, reps, share):
    """fwd_group_launch's choice for the members of one launch (csrc/conv_fwd.hip), with `share`: the strip and the
    32-channel-tile thresholds are on n * share."""
    count, out = len(mcs), []
    for H, W, Ca, mode, shift, Cv, Cout, pool, _ in mcs:
        b = L.body_of(('', H, W, Ca, mode, shift, Cv, Cout, pool), n * share)
        big = W >= 16 and W % 16 == 0 and H % 4 == 0
        if count == 1 and mode == 'img' and 1 <= Ca <= 3 and not Cv and shift == 0 and Cout == 16 and big:
            b = 'first'                                        # conv_first.hip: the image -> 16 conv of a net, alone
        elif count == 1 and reps == 1 and share == 1 and mode == 'batch' and b in ('g8', 'g4') and \
                Ca % 32 == 0 and Cv % 32 == 0 and Ca + Cv >= 64:
            b = {'g8': 'ks8', 'g4': 'ks4'}[b]                  # K-split: one net only, never once share > 1 or reps > 1
        out.append(b)
    wide = all(b in ('g8', 'g4') and mc[6] % 32 == 0 and n * share >= L.WIDE_MIN and
               (mc[3] != 'batch' or (share > 1 and count == 1)) for b, mc in zip(out, mcs))
    return [{'g8': 'wide8', 'g4': 'wide4'}[b] for b in out] if wide else out


def body_of(mc, n, share, reps=1):
    """One member alone in its launch."""
    return bodies_of([mc], n, reps, share)[0]


class Net:
    """The members of one net: own data (salt), the float64 reference of every member computed once."""

    def __init__(self, mcs, n, r):
        self.ms = [Member(('m%d' % k,) + mc[:8], n, salt=101 * r + k + 1, out_nslot=mc[8]) for k, mc in enumerate(mcs)]
        self.refs = [m.ref(np.arange(n)) for m in self.ms]


def _poison(nets):
    for net in nets:
        for m in net.ms:
            m.poison()


def _untouched(m):
    out, pool = m.rows()
    return np.isnan(out).all() and (pool is None or np.isnan(pool).all()) and not m.sums().any()


def _bits(a, b):
    return a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_buffers(m, mc, got, sums, what):
    import hiputil as U
    out, pool = got
    assert np.isfinite(out).all(), what + ': out not written everywhere'
    assert (sums[mc[8]:] == 0).all(), what + ': a slot >= out_nslot of out_sum was written'
    if mc[7]:
        assert np.isfinite(pool).all(), what + ': pool_out not written everywhere'
        mine = U.pool2_np(out.reshape(m.n, m.H, m.W, m.Cout)).reshape(m.n, -1)
        assert np.array_equal(pool, mine), what + ': pool_out is not the 2x2 max of out'


def _check_oracle(m, ref, out, what):
    tol = 3e-5 if m.bn else 2e-5
    lim = tol * (1.0 + np.abs(ref).max())
    err = np.abs(out.reshape(ref.shape) - ref).max()
    print('%s: out worst error / limit = %.3f' % (what, err / lim))
    assert err <= lim, (what, err / lim)


def _check_stats(m, out, sums, what):
    """(c): the kernel's sums against the float64 sums of the fp32 values it stored."""
    o = out.reshape(-1, m.Cout).astype(np.float64)
    s = sums.sum(0)
    worst = 0.0
    for got, ref, bound in ((s[:m.Cout], o.sum(0), np.abs(o).sum(0)), (s[m.Cout:], (o * o).sum(0), (o * o).sum(0))):
        worst = max(worst, float((np.abs(got - ref) / (1e-5 * bound + 1e-9)).max()))
    print('%s: out_sum worst error / limit = %.3f' % (what, worst))
    assert worst <= 1.0, (what, worst)


def _same_slots(a, b, what):
    assert (np.abs(a - b) <= 1e-12 * (np.abs(a).max() + np.abs(a))).all(), (what, np.abs(a - b).max())


def _joint(nets, entry, reps, share):
    got = launch([net.ms for net in nets], entry=entry, reps=reps, share=share)
    return got, [[m.sums() for m in net.ms] for net in nets]


@gpu
@pytest.mark.parametrize('name', list(ROWS))
def test_rep_launch(name):
    members, n, reps, share = ROWS[name]
    mcs = [mb[0] for mb in members]
    count = len(mcs)
    assert bodies_of(mcs, n, reps, share) == [mb[1] for mb in members], 'the launcher selects other bodies than the row lists'
    entry = 'rep' if reps > 1 or share > 1 else 'group'        # (one net: mpnn_msconv_fwd_group)
    nets = [Net(mcs, n, r) for r in range(reps)]
    joint, jsums = _joint(nets, entry, reps, share)
    for r, net in enumerate(nets):                             # a, b, c
        for k, m in enumerate(net.ms):
            what = '%s, net %d member %d' % (name, r, k)
            _check_buffers(m, mcs[k], joint[r][k], jsums[r][k], what)
            _check_oracle(m, net.refs[k], joint[r][k][0], what)
            _check_stats(m, joint[r][k][0], jsums[r][k], what)
    for r, net in enumerate(nets):                             # d: the nets take turns with the same grids
        _poison(nets)
        turn, = launch([net.ms], entry='rep', reps=1, share=share)
        for k, m in enumerate(net.ms):
            what = '%s, net %d member %d alone in its turn' % (name, r, k)
            assert _bits(turn[k][0], joint[r][k][0]) and _bits(turn[k][1], joint[r][k][1]), what
            _same_slots(m.sums(), jsums[r][k], what)
        assert all(_untouched(m) for other in nets if other is not net for m in other.ms), 'another net was written'
    for r, net in enumerate(nets):                             # e: the plain launch of every record
        for k, m in enumerate(net.ms):
            what = '%s, net %d member %d: mpnn_msconv_fwd' % (name, r, k)
            one, = launch([m], entry='fwd')
            if members[k][1] in ORDER_DIFFERS:
                assert np.abs(one[0] - joint[r][k][0]).max() <= 2e-5 * (1.0 + np.abs(one[0]).max()), what
            else:
                assert _bits(one[0], joint[r][k][0]) and _bits(one[1], joint[r][k][1]), what
    if count > 1:                                              # f: every member alone at the same reps / share
        for k in range(count):
            alone = launch([[net.ms[k]] for net in nets], entry=entry, reps=reps, share=share)
            lone = body_of(mcs[k], n, share, reps)              # the kernel (f) runs: listed where it is not the joint body
            assert lone == members[k][-1], 'member %d alone runs %s, the row lists %s' % (k, lone, members[k][-1])
            differs = lone in ORDER_DIFFERS and members[k][1] not in ORDER_DIFFERS
            for r, net in enumerate(nets):
                what = '%s, net %d member %d alone' % (name, r, k)
                got = alone[r][0]
                if differs:                                    # (the K-split body of a deep member alone in one net)
                    assert np.abs(got[0] - joint[r][k][0]).max() <= 2e-5 * (1.0 + np.abs(got[0]).max()), what
                else:
                    assert _bits(got[0], joint[r][k][0]) and _bits(got[1], joint[r][k][1]), what
                sums = net.ms[k].sums()
                _check_buffers(net.ms[k], mcs[k], got, sums, what)
                _check_stats(net.ms[k], got[0], sums, what)


@gpu
def test_rep_launch_replayed_from_a_graph():
    """The 'four bodies' joint launch of two nets captured on a side stream and replayed twice over re-poisoned outputs
    and zeroed out_sum: the eager launch's bits both times, out_sum per slot to 1e-12."""
    import torch
    import hiputil as U
    lib = _hip.load()
    members, n, reps, share = ROWS['four bodies']
    mcs = [mb[0] for mb in members]
    nets = [Net(mcs, n, r) for r in range(reps)]
    eager, esums = _joint(nets, 'rep', reps, share)
    for r, net in enumerate(nets):                             # (the eager bits are themselves the oracle's, in every net)
        for k, m in enumerate(net.ms):
            _check_buffers(m, mcs[k], eager[r][k], esums[r][k], 'eager, net %d member %d' % (r, k))
            _check_oracle(m, net.refs[k], eager[r][k][0], 'eager, net %d member %d' % (r, k))
    recs = [m.rec for net in nets for m in net.ms]
    arr = (_hip.ConvFwdArgs * len(recs))(*recs)
    tab = _hip.to_device_table(recs, U.DEV)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    _poison(nets)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        st = torch.cuda.current_stream().cuda_stream
        _hip.check(lib.mpnn_msconv_fwd_group_rep(arr, tab.data_ptr(), len(mcs), reps, share, st), 'fwd_group_rep')
    torch.cuda.synchronize()
    assert all(_untouched(m) for net in nets for m in net.ms), 'the capture itself ran the launch'
    for i in range(2):
        _poison(nets)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for r, net in enumerate(nets):
            for k, m in enumerate(net.ms):
                what = 'replay %d, net %d member %d' % (i, r, k)
                got = m.rows()
                assert _bits(got[0], eager[r][k][0]) and _bits(got[1], eager[r][k][1]), what
                _same_slots(m.sums(), esums[r][k], what)


def test_rep_argument_errors():
    """The documented refusals of mpnn_msconv_fwd_group_rep (host-side checks: no device needed, nothing launches; the
    pointers are placeholders that the host code only tests for NULL).  Every one of the reps * count records gets the
    pointer checks of the single-net launchers -- a NULL in net 1's record must not reach the device."""
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load()
    FAKE, E_ARG = 0x1000, _hip.E_ARG                           # (never dereferenced)

    def rec(**kw):
        a = _hip.ConvFwdArgs()
        a.a.x, a.a.C, a.a.mode, a.a.shift = FAKE, 32, _hip.ACT_BN_BATCH, 0
        a.v, a.Cv, a.wa_pack, a.wv_pack, a.bias = FAKE, 16, FAKE, FAKE, FAKE
        a.out, a.pool_out, a.out_sum, a.out_nslot = FAKE, FAKE, FAKE, 8
        a.n, a.H, a.W, a.Cout = 7, 8, 8, 32
        for k, v in kw.items():
            if k in ('x', 'C', 'mode', 'shift'):
                setattr(a.a, k, v)
            else:
                setattr(a, k, v)
        return a

    def rep(recs, count, reps, share=0, args=True):
        arr = (_hip.ConvFwdArgs * len(recs))(*recs)
        return lib.mpnn_msconv_fwd_group_rep(arr if args else None, FAKE, count, reps, share, None)

    assert rep([rec(), rec()], 1, 0) == E_ARG                   # reps < 1
    assert rep([rec(), rec()], 1, -2) == E_ARG
    assert rep([rec() for _ in range(5)], 5, 1) == E_ARG        # count > 4
    assert rep([rec() for _ in range(10)], 5, 2) == E_ARG
    assert rep([rec()], 1, 1, args=False) == E_ARG              # NULL args
    assert rep([rec(), rec()], 1, 2, args=False) == E_ARG
    assert rep([rec(), rec()], 0, 2) == 0                       # an empty group: nothing to do
    assert rep([rec(), rec()], -1, 2) == 0
    # nets that differ: one field each
    for kw in (dict(n=6), dict(H=4, W=4, pool_out=None), dict(H=4), dict(W=4), dict(Cout=16), dict(C=16),
               dict(mode=_hip.ACT_BN_MOVING), dict(shift=1), dict(v=None), dict(v=None, wv_pack=None), dict(Cv=32),
               dict(out_nslot=4), dict(pool_out=None), dict(out_sum=None)):
        assert rep([rec(), rec(**kw)], 1, 2) == E_ARG, kw
        assert rep([rec(), rec(), rec(), rec(**kw)], 2, 2) == E_ARG, kw
        assert rep([rec(), rec(), rec(**kw)], 1, 3, 8) == E_ARG, kw
    # a NULL pointer in a record of net 1 (and of net 0), v without wv_pack
    for kw in (dict(x=None), dict(wa_pack=None), dict(bias=None), dict(out=None), dict(wv_pack=None)):
        assert rep([rec(), rec(**kw)], 1, 2) == E_ARG, kw
        assert rep([rec(), rec(), rec(**kw), rec()], 2, 2) == E_ARG, kw
        assert rep([rec(), rec(), rec(), rec(**kw)], 2, 2) == E_ARG, kw
        assert rep([rec(), rec(), rec(**kw)], 1, 3) == E_ARG, kw
        assert rep([rec(), rec(**kw)], 1, 2, 8) == E_ARG, kw
        assert rep([rec(**kw), rec()], 1, 2) == E_ARG, kw
        assert rep([rec(**kw)], 1, 1, 8) == E_ARG, kw
