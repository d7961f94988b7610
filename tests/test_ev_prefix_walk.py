"""mpnn_ev_prefix_walk (csrc/exit_ev.hip: ev_prefix_k) alone, through the C ABI, on the GPU, against tests/ev_walk_ref.py.

(The net tests reach the launch only through 8-block two-way chains: at most 8 records, all with head and router, one
list, counts of zero, no ties.)  Every array -- router outputs, c_err, d_cor, the lists and their counts -- sits in its
own sentinel-guarded buffer; r, c_err and d_cor are pre-filled with random finite values, the padding columns
r[:, n_sinks:r_stride] with NaN.  All comparisons are exact:

  * reached entries keep their bits (-0.0 included), unreached entries are +0.0, the NaN padding is untouched;
  * every list, sorted, is the reference's set, its count is on the device, no sample is in two lists, no guard changed;
  * a second launch on fresh inputs gives the same sets (the order inside a list depends on wave timing, the set does not).

Tables:
  chain8  eight two-way switches in a chain (head + router each, r_stride 4 as the engine lays them out), one list;
  mixed   test_exit_kernels.mixed_tree: a 3-way switch without a head on rows of stride 4, a 4-way and two 2-way
          switches, static and leaf records with a head and no router, five lists, two of them under one switch;
  cat64   64 records: a caterpillar of 32 two-way switches (even records) with a static head-only record hanging off
          each (odd records).  Records 32-63 keep their decisions in the kernel's SECOND 64-bit word: switches 16-31
          gate everything deeper and five of the six lists.  The router outputs send a quarter of the samples down the
          whole spine and a quarter to its last static record, so the deepest records are reached by >= 10 samples from
          n = 63 on (asserted against the reference).
Batch sizes 1, 63, 64, 65, 255, 256, 257, 1000: around the 64-lane wave and the 256-thread workgroup.
Ties in a fixed share of the rows: two, three or all sinks exactly equal, +0.0 against -0.0 -- the first index wins."""
import ctypes as C

import numpy as np
import pytest

import ev_walk_ref as W
from lib import _hip

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
INT_SENTINEL = -0x5A5A5A5B


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


def chain8():
    """switch k: sinks {its own leaf, switch k + 1}; the last one's second sink is the frontier block."""
    from oracle.route_ref import Tree
    nodes = []
    for k in range(8):
        nodes += [dict(sinks=[2 * k + 1, 2 * k + 2]), dict()]
    nodes.append(dict())
    tree = Tree(nodes)
    sw = list(range(0, 16, 2))
    return W.build(tree, sw, set(sw), [16], {i: 4 for i in sw})


def mixed():
    from test_exit_kernels import mixed_tree
    tree = mixed_tree()
    # 0 root (static, head), 1 A (3-way, NO head, stride 4), 2 / 4 / 9 leaves (head), 3 B, 5 D (static, head), 7 C (4-way),
    # 10 E (static, head), 11 F (2-way, no head, stride 3); lists: 6 (below D: B's sink 1), 8, 14 (C), 12 and 13 (both F's)
    return W.build(tree, [0, 1, 2, 3, 4, 5, 7, 9, 10, 11], {0, 2, 3, 4, 5, 7, 9, 10}, [6, 8, 12, 13, 14], {1: 4, 7: 4, 11: 3})


def cat64():
    """spine switch k = record 2k: sinks {static H_k = record 2k + 1 -> a block, switch k + 1}.  DFS preorder."""
    from oracle.route_ref import Tree
    nodes, spine, hang = [], [], []
    for k in range(32):
        i = len(nodes)
        spine.append(i); hang.append(i + 1)
        nodes += [dict(sinks=[i + 1, i + 3]), dict(sinks=[i + 2]), dict()]       # S_k, H_k, the block below H_k
    nodes.append(dict())                                                        # the block below S_31's second sink
    tree = Tree(nodes)
    fronts = [hang[5] + 1, hang[20] + 1, hang[25] + 1, hang[28] + 1, hang[31] + 1, len(nodes) - 1]
    tab = W.build(tree, spine + hang, set(hang) | set(spine[::3]), fronts, {s: 2 + k % 3 for k, s in enumerate(spine)})
    assert tab.count == 64 and [tab.n_sinks[j] > 0 for j in range(64)] == [j % 2 == 0 for j in range(64)]
    assert tab.parent[2:] == [j - 2 + j % 2 for j in range(2, 64)] and tab.front_parent == [10, 40, 50, 56, 62, 62]
    return tab


TABLES = {'chain8': chain8, 'mixed': mixed, 'cat64': cat64}


def router_outputs(tab, kind, n, rng):
    """r[j]: [n, r_stride[j]] float32, NaN in the padding columns; ties in a fixed share of the rows; chain8 and
    cat64: routes that reach the deep records."""
    r = []
    for j in range(tab.count):
        S, st = tab.n_sinks[j], tab.r_stride[j]
        if S == 0:
            r.append(None)
            continue
        x = np.full((n, st), np.nan, np.float32)
        x[:, :S] = rng.standard_normal((n, S))
        for s in range((3 * j) % 5, n, 5):                     # every fifth row of a switch
            how = (s // 5 + j) % 4
            top = np.float32(np.abs(x[s, :S]).max() + 1.0)
            if how == 0:                                       # all sinks equal
                x[s, :S] = x[s, 0]
            elif how == 1:                                     # the two (three) largest equal, somewhere in the row
                x[s, rng.choice(S, size=min(S, 2), replace=False)] = top
            elif how == 2:
                x[s, rng.choice(S, size=min(S, 3), replace=False)] = top
            else:                                              # zeros of both signs
                x[s, :S] = np.where(rng.random(S) < 0.5, np.float32(0.0), np.float32(-0.0))
        r.append(x)
    if kind == 'chain8':                                       # every third sample passes all eight switches
        for j in range(8):
            r[j][::3, :2] = (-1.0, 0.5 + j)
    if kind == 'cat64':
        for s in range(n):
            q, t = s % 4, s // 4
            stop = {0: 32, 1: 31, 2: t % 32}.get(q)            # the spine switch that sends s to its static record
            if stop is None:
                continue                                       # (a quarter of the samples: whatever the rows above say)
            for k in range(min(stop + 1, 32)):
                x = r[2 * k]
                if k < stop:
                    x[s, :2] = (-1.0, 0.5 + k)                 # down the spine
                elif (t + k) % 3 == 0:
                    x[s, :2] = (0.25, 0.25) if t % 2 else (0.0, -0.0)     # a tie: the first sink
                else:
                    x[s, :2] = (2.0, 1.0)
    return r


class Run:
    """One launch: guarded device copies of every array of a table, the record, the reference's answer."""

    def __init__(self, tab, kind, n, seed, pre=None):
        import hiputil as U
        rng = np.random.default_rng(seed)
        self.tab, self.n = tab, n
        self.r = router_outputs(tab, kind, n, rng)
        self.ce = [rng.standard_normal(n).astype(np.float32) if h else None for h in tab.has_head]
        self.dc = [(rng.random(n) < 0.5).astype(np.float32) if h else None for h in tab.has_head]
        self.ref = W.walk(tab, self.r, self.ce, self.dc)
        self.pre = pre or {}                                   # list -> entries it holds before the launch
        mk = lambda a: None if a is None else self._filled(U.Guarded(a.size), a)
        self.d_r, self.d_ce, self.d_dc = [mk(a) for a in self.r], [mk(a) for a in self.ce], [mk(a) for a in self.dc]
        self.lists, self.cnts = [], []
        for f in range(tab.n_front):
            lst, cnt = _guarded_int(n), _guarded_int(1)
            lst.t.fill_(-1); cnt.t.fill_(0)
            marks = self.pre.get(f, [])
            if marks:
                lst.fill(np.array(list(marks) + [-1] * (n - len(marks)), np.int32)); cnt.t.fill_(len(marks))
            self.lists.append(lst); self.cnts.append(cnt)
        a = self.rec = _hip.EvPrefixArgs()
        a.n, a.count, a.n_front = n, tab.count, tab.n_front
        for j in range(tab.count):
            a.parent[j], a.parent_sink[j], a.n_sinks[j], a.r_stride[j] = tab.parent[j], tab.parent_sink[j], tab.n_sinks[j], tab.r_stride[j]
            a.r[j] = self.d_r[j].ptr() if self.d_r[j] is not None else None
            a.c_err[j] = self.d_ce[j].ptr() if self.d_ce[j] is not None else None
            a.d_cor[j] = self.d_dc[j].ptr() if self.d_dc[j] is not None else None
        for f in range(tab.n_front):
            a.front_parent[f], a.front_sink[f] = tab.front_parent[f], tab.front_sink[f]
            a.front_idx[f], a.front_cnt[f] = self.lists[f].ptr(), self.cnts[f].ptr()

    @staticmethod
    def _filled(g, a):
        g.fill(a)
        return g

    def launch(self, n=None):
        import torch
        import hiputil as U
        if n is not None:
            self.rec.n = n
        dev = _hip.to_device_table([self.rec], U.DEV)
        rc = _hip.load().mpnn_ev_prefix_walk(C.byref(self.rec), dev.data_ptr(), U.stream())
        torch.cuda.synchronize()
        return rc

    def guards_ok(self):
        bufs = [b for b in self.d_r + self.d_ce + self.d_dc if b is not None] + self.lists + self.cnts
        return all(b.guards_ok() for b in bufs)

    def check_arrays(self, want_r, want_ce, want_dc):
        """Bit for bit: NaN padding, signed zeros and the +0.0 of cleared entries included."""
        bits = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)
        for j in range(self.tab.count):
            for name, buf, want in (('r', self.d_r[j], want_r[j]), ('c_err', self.d_ce[j], want_ce[j]), ('d_cor', self.d_dc[j], want_dc[j])):
                if buf is not None:
                    assert np.array_equal(bits(buf.get()), bits(want)), 'record %d: %s' % (j, name)

    def sets(self):
        """The lists as the launch left them: [(entries before the launch's own, sorted arrivals)], counts checked."""
        out = []
        for f in range(self.tab.n_front):
            k = len(self.pre.get(f, []))
            cnt, lst = int(self.cnts[f].get()[0]), self.lists[f].get()
            assert cnt == k + len(self.ref['fronts'][f]), 'list %d: count %d' % (f, cnt)
            assert cnt <= self.n and (lst[cnt:] == -1).all(), 'list %d: written past its count' % f
            out.append((lst[:k].tolist(), np.sort(lst[k:cnt])))
        return out


def _cases():
    return [(kind, n) for kind in TABLES for n in SIZES]


@pytest.mark.parametrize('kind,n', _cases())
def test_walk_equals_the_reference(kind, n):
    tab = TABLES[kind]()
    run = Run(tab, kind, n, seed=n * 7 + len(kind))
    ref = run.ref
    if kind == 'cat64':
        if n >= 63:                                            # the deepest records, all behind decisions of the second word
            assert min(ref['reach'][j].sum() for j in (62, 63)) >= 10 and min(len(ref['fronts'][f]) for f in (4, 5)) >= 10
    if kind == 'chain8' and n >= 63:
        assert len(ref['fronts'][0]) >= 10
    if kind == 'mixed' and n >= 255:
        assert all(len(s) > 0 for s in ref['fronts']) and all(x.any() and not x.all() for x in ref['reach'][2:])
    assert run.launch() == 0
    assert run.guards_ok()
    run.check_arrays(ref['r'], ref['c_err'], ref['d_cor'])
    for j in range(tab.count):                                 # (said once more in words: cleared is 0.0, padding stays NaN)
        if run.d_r[j] is not None:
            got = run.d_r[j].get().reshape(n, -1)
            assert np.isnan(got[:, tab.n_sinks[j]:]).all() and (got[~ref['reach'][j], :tab.n_sinks[j]] == 0.0).all()
            assert np.array_equal(got[ref['reach'][j], :tab.n_sinks[j]], run.r[j][ref['reach'][j], :tab.n_sinks[j]])
    sets = run.sets()
    seen = np.zeros(n, int)
    for f, (_, got) in enumerate(sets):
        assert np.array_equal(got, ref['fronts'][f]), 'list %d' % f
        seen[got] += 1
    assert (seen <= 1).all(), 'a sample in two lists'
    again = Run(tab, kind, n, seed=n * 7 + len(kind))           # fresh buffers, the same inputs
    assert again.launch() == 0 and again.guards_ok()
    for (_, a), (_, b) in zip(sets, again.sets()):
        assert np.array_equal(a, b)
    again.check_arrays(ref['r'], ref['c_err'], ref['d_cor'])


@pytest.mark.parametrize('kind,n,f', [('cat64', 257, 5), ('mixed', 1000, 3), ('chain8', 65, 0)])
def test_arrivals_are_appended_behind_what_a_list_holds(kind, n, f):
    """List f starts with count 3 and three marker entries: they stay, the arrivals follow them, the count is 3 + arrivals
    (3 + arrivals <= n here: the launch drops what does not fit a list of n entries, and nothing may be dropped)."""
    tab = TABLES[kind]()
    marks = [-7, -8, -9]
    run = Run(tab, kind, n, seed=n + f, pre={f: marks})
    arrivals = len(run.ref['fronts'][f])
    assert 0 < arrivals <= n - 3
    assert run.launch() == 0 and run.guards_ok()
    sets = run.sets()
    assert sets[f][0] == marks
    for g, (_, got) in enumerate(sets):
        assert np.array_equal(got, run.ref['fronts'][g]), 'list %d' % g
    run.check_arrays(run.ref['r'], run.ref['c_err'], run.ref['d_cor'])


def test_no_samples_no_launch():
    """n = 0: returns 0 and writes nothing."""
    tab = mixed()
    run = Run(tab, 'mixed', 64, seed=3)
    assert run.launch(n=0) == 0 and run.guards_ok()
    run.check_arrays(run.r, run.ce, run.dc)
    for lst, cnt in zip(run.lists, run.cnts):
        assert (lst.get() == -1).all() and cnt.get()[0] == 0
