"""mpnn_conf_gate (csrc/conf_gate.hip) alone, through the C ABI, on the GPU, against tests/conf_gate_ref.py.

Every array -- confidences, the threshold, router rows, sample list, count, child lists and their counts -- sits in its own
sentinel-guarded buffer.  The router rows are [images, 4] with NaN in the columns from n_sinks on; a fixed share of the rows
holds ties (two, three or all sinks equal, zeros of both signs); some confidences are NaN; the threshold is one of the
confidences, bit for bit, unless the case names another.  Everything is exact, no tolerance anywhere:

  * the rows equal the reference's bit for bit -- decisions, the untouched rows of images outside the list, the NaN padding;
  * every child list, sorted, is the reference's set and its count is on the device; entries beyond the count keep -1;
    sinks without a list leave nothing anywhere;
  * no guard changes; a child count that starts near the capacity drops what does not fit instead of writing past n.

n in {1, 63, 64, 65, 257}: around the 64-lane wave and the 256-thread workgroup; 2, 3 and 4 sinks with the exit sink first,
in the middle and last; with and without a permuted sample list whose device count is below its capacity."""
import ctypes as C

import numpy as np
import pytest

import conf_gate_ref as G
from lib import _hip

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
SINKS = ((2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0), (4, 2), (4, 3))
STRIDE = 4
INT_SENTINEL = -0x5A5A5A5B
NAN, INF = float('nan'), float('inf')


def _guarded_int(size):
    """hiputil.Guarded for int32 (its float sentinel does not fit an integer)."""
    import torch
    import hiputil as U

    class GuardedInt(U.Guarded):
        def __init__(self, size):
            self.size = size
            self.buf = torch.full((size + 2 * U.GUARD,), INT_SENTINEL, dtype=torch.int32, device=U.DEV)
            self.t = self.buf[U.GUARD:U.GUARD + size]

        def guards_ok(self):
            return bool((self.buf[:U.GUARD] == INT_SENTINEL).all() and (self.buf[U.GUARD + self.size:] == INT_SENTINEL).all())

    return GuardedInt(size)


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


class Rec:
    """One record: n samples (the capacity of its lists) of `images` images; listed: a permuted sample list of capacity n
    with a device count below it.  lists: the sinks that get a child list (default: all but the exit sink and, from three
    sinks on, one more that stays NULL); start: {sink: (count before the launch)}."""

    def __init__(self, n, S, ex, seed, listed, tau='conf', lists=None, start=None):
        import hiputil as U
        rng = np.random.default_rng(seed)
        self.n, self.S, self.ex = n, S, ex
        self.images = n + 37 if listed else n
        m = self.images
        conf = rng.random(m).astype(np.float32)
        conf[rng.random(m) < 0.1] = np.float32(NAN)
        r = np.full((m, STRIDE), NAN, np.float32)
        r[:, :S] = rng.standard_normal((m, S))
        for s in range(seed % 3, m, 3):                            # every third row: a tie
            how = (s // 3) % 4
            top = np.float32(np.abs(r[s, :S]).max() + 1.0)
            if how == 0:
                r[s, :S] = r[s, 0]
            elif how == 1:
                r[s, rng.choice(S, size=min(S, 2), replace=False)] = top
            elif how == 2:
                r[s, rng.choice(S, size=min(S, 3), replace=False)] = top
            else:
                r[s, :S] = np.where(rng.random(S) < 0.5, np.float32(0.0), np.float32(-0.0))
        self.idx = self.cnt = None
        if listed:
            self.idx = rng.permutation(m)[:n].astype(np.int32)
            self.cnt = max(n - max(n // 5, 1), 0) if n > 1 else 1
        on_list = self.idx[:self.cnt] if listed else np.arange(n)
        if isinstance(tau, str):                                   # one of the list's own confidences, bit for bit
            cand = np.sort(conf[on_list][~np.isnan(conf[on_list])])
            tau = cand[len(cand) // 2] if len(cand) else np.float32(0.5)
        self.tau = np.float32(tau)
        self.conf, self.r = conf, r
        self.ref = G.gate(conf, self.tau, r, S, ex, idx=self.idx, cnt=self.cnt, n=n)
        if lists is None:
            lists = [i for i in range(S) if i != ex]
            if S >= 3:
                lists = lists[1:] + [ex] if seed % 2 else lists[:-1]      # (one child sink without a list; sometimes the exit sink with one)
        self.lists, self.start = list(lists), dict(start or {})
        self.d_conf, self.d_tau, self.d_r = U.Guarded(m), U.Guarded(1), U.Guarded(m * STRIDE)
        self.d_conf.fill(conf); self.d_tau.fill(np.array([self.tau])); self.d_r.fill(r)
        self.d_idx = self.d_cnt = None
        if listed:
            self.d_idx, self.d_cnt = _guarded_int(n), _guarded_int(1)
            self.d_idx.fill(self.idx); self.d_cnt.t.fill_(self.cnt)
        self.d_list, self.d_lcnt = {}, {}
        for i in self.lists:
            self.d_list[i], self.d_lcnt[i] = _guarded_int(n), _guarded_int(1)
            self.d_list[i].t.fill_(-1); self.d_lcnt[i].t.fill_(self.start.get(i, 0))
        a = self.rec = _hip.ConfGateArgs()
        a.conf, a.tau, a.r, a.r_stride = self.d_conf.ptr(), self.d_tau.ptr(), self.d_r.ptr(), STRIDE
        a.n_sinks, a.exit_sink, a.n = S, ex, n
        if listed:
            a.idx, a.cnt = self.d_idx.ptr(), self.d_cnt.ptr()
        for i in self.lists:
            a.child_idx[i], a.child_cnt[i] = self.d_list[i].ptr(), self.d_lcnt[i].ptr()
        assert _hip.load().mpnn_conf_gate_check(C.byref(a)) == 0

    def buffers(self):
        out = [self.d_conf, self.d_tau, self.d_r] + list(self.d_list.values()) + list(self.d_lcnt.values())
        return out + ([self.d_idx, self.d_cnt] if self.d_idx is not None else [])

    def check(self):
        assert all(b.guards_ok() for b in self.buffers()), 'a guard changed'
        assert np.array_equal(bits(self.d_conf.get()), bits(self.conf)) and np.array_equal(bits(self.d_tau.get()), bits(self.tau))
        got = self.d_r.get().reshape(self.images, STRIDE)
        assert np.array_equal(bits(got), bits(self.ref['rows'])), 'rows'
        on = np.array(self.ref['imgs'], int)
        assert np.isnan(got[:, self.S:]).all()                    # (said once more in words)
        if len(on):
            assert np.array_equal(got[on, :self.S].argmax(1), [self.ref['d'][i] for i in on])
            assert (np.sort(got[on, :self.S], 1)[:, -1] == 1).all() and (got[on, :self.S].sum(1) == 1).all()
        rest = np.setdiff1d(np.arange(self.images), on)
        assert np.array_equal(bits(got[rest]), bits(self.r[rest])), 'a row outside the list changed'
        if self.d_idx is not None:
            assert np.array_equal(self.d_idx.get(), self.idx) and self.d_cnt.get()[0] == self.cnt
        for i in self.lists:
            k = self.start.get(i, 0)
            want = self.ref['children'][i]
            cnt, lst = int(self.d_lcnt[i].get()[0]), self.d_list[i].get()
            assert cnt == k + len(want), 'sink %d: count %d, %d arrivals behind %d' % (i, cnt, len(want), k)
            fit = min(cnt, self.n)
            assert (lst[:k] == -1).all() and (lst[fit:] == -1).all(), 'sink %d: written outside [start, count)' % i
            arrived = lst[k:fit]
            if cnt <= self.n:
                assert np.array_equal(np.sort(arrived), want), 'sink %d' % i
            else:                                                  # (what does not fit is dropped: a subset, nothing twice)
                assert len(set(arrived.tolist())) == len(arrived) and set(arrived.tolist()) <= set(want.tolist())


def launch(recs):
    import torch
    import hiputil as U
    tab = _hip.to_device_table([q.rec for q in recs], U.DEV)
    rc = _hip.load().mpnn_conf_gate(tab.data_ptr(), len(recs), max(q.n for q in recs), U.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('S,ex', SINKS)
@pytest.mark.parametrize('n', SIZES)
def test_gate_equals_the_reference(n, S, ex):
    for listed in (False, True):
        q = Rec(n, S, ex, seed=n * 11 + S * 3 + ex, listed=listed)
        if n >= 63:                                                # the case does decide both ways, and among children
            d = np.array(list(q.ref['d'].values()))
            assert (d == ex).sum() >= 5 and (d != ex).sum() >= 5
            assert S == 2 or len(set(d[d != ex].tolist())) == S - 1
            hit = q.conf[q.ref['imgs']] == q.tau
            assert hit.any() and all(q.ref['d'][i] == ex for i in np.array(q.ref['imgs'])[hit])     # conf == tau leaves
        assert launch([q]) == 0
        q.check()


def test_a_table_of_three_records_with_different_thresholds():
    recs = [Rec(257, 4, 2, seed=1, listed=True, tau=0.25), Rec(65, 2, 0, seed=2, listed=False, tau=0.75),
            Rec(64, 3, 1, seed=3, listed=True)]
    exits = [np.mean([d == q.ex for d in q.ref['d'].values()]) for q in recs]
    assert exits[0] > 0.5 > exits[1] > 0.05                        # (the thresholds do differ in effect)
    assert launch(recs) == 0
    for q in recs:
        q.check()


@pytest.mark.parametrize('tau', [NAN, INF, -INF])
@pytest.mark.parametrize('S,ex', [(2, 0), (3, 1), (4, 3)])
def test_nan_and_infinite_thresholds(tau, S, ex):
    for listed in (False, True):
        q = Rec(65, S, ex, seed=5 + S, listed=listed, tau=tau)
        d = np.array([q.ref['d'][i] for i in q.ref['imgs']])
        nan_conf = np.isnan(q.conf[q.ref['imgs']])
        assert nan_conf.any() and not nan_conf.all()
        if tau == -INF:                                            # everybody leaves but the NaN confidences
            assert np.array_equal(d == ex, ~nan_conf)
        else:                                                      # NaN: no; +inf: no finite confidence reaches it
            assert (d != ex).all()
        assert launch([q]) == 0
        q.check()


def test_every_confidence_nan():
    q = Rec(64, 3, 0, seed=9, listed=False, tau=0.0)
    q.conf[:] = np.float32(NAN)
    q.d_conf.fill(q.conf)
    q.ref = G.gate(q.conf, q.tau, q.r, 3, 0, n=64)
    assert all(d != 0 for d in q.ref['d'].values())
    assert launch([q]) == 0
    q.check()


@pytest.mark.parametrize('n', [65, 257])
def test_a_count_that_starts_near_the_capacity_never_writes_past_n(n):
    """tau = -inf sends every finite confidence to the exit sink, which has a list here that starts at n - 3: three
    arrivals fit, the others are dropped; the count still counts them all (as exit_ev_k's does)."""
    q = Rec(n, 3, 1, seed=n, listed=False, tau=-INF, lists=[0, 1, 2], start={1: n - 3, 2: 1})
    assert len(q.ref['children'][1]) > 10
    assert launch([q]) == 0
    q.check()
    assert int(q.d_lcnt[1].get()[0]) > n and (q.d_list[1].get()[n - 3:] >= 0).all()


def test_nothing_to_do_is_no_launch():
    q = Rec(64, 2, 0, seed=4, listed=True)
    lib = _hip.load()
    import hiputil as U
    tab = _hip.to_device_table([q.rec], U.DEV)
    assert lib.mpnn_conf_gate(tab.data_ptr(), 0, 64, U.stream()) == 0 and lib.mpnn_conf_gate(tab.data_ptr(), 1, 0, U.stream()) == 0
    # a device count of zero: a launch that leaves at once
    q.d_cnt.t.fill_(0)
    q.cnt = 0
    q.ref = G.gate(q.conf, q.tau, q.r, 2, 0, idx=q.idx, cnt=0, n=64)
    assert launch([q]) == 0
    q.check()
