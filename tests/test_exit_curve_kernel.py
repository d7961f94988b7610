"""mpnn_exit_curve (csrc/exit_curve.hip) alone, through the C ABI, on the GPU, against tests/exit_curve_ref.py -- exactly:
the sums are integers.

Random confidences, hits and router outputs in sentinel-guarded buffers whose strides exceed n; a share of the router rows
holds ties (two, three or all sinks equal, zeros of both signs), a share of the confidences is NaN; every threshold is one
of the confidences of its exit, bit for bit (conf == tau leaves), or -inf, +inf, NaN.  The trees: a 2-exit and an 8-exit
chain of switches, a static chain, the 15-block tree with 3-sink switches (a binary tree over three levels of blocks with an
exit under each, single-exit blocks under its ends) and a mix of gated, ungated (NaN) and static nodes.  n around the
64-lane wave and the 256-thread workgroup and beyond two workgroups; 1, 2 and 33 points.  Each case asserts that every
leaf's histogram is non-zero at some point -- a walk that never leaves exit 0 cannot pass -- and that no guard changed."""
import ctypes as C

import numpy as np
import pytest

import exit_curve_ref as R
from lib import _hip

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 600)
POINTS = (1, 2, 33)
NAN, INF = float('nan'), float('inf')
MS = 4
I64_SENTINEL = -0x5A5A5A5A5A5A5A5B
N = R.node


def _guarded_i64(size):
    """hiputil.Guarded for int64 (its float sentinel does not fit an integer)."""
    import torch
    import hiputil as U

    class GuardedI64(U.Guarded):
        def __init__(self, size):
            self.size = size
            self.buf = torch.full((size + 2 * U.GUARD,), I64_SENTINEL, dtype=torch.int64, device=U.DEV)
            self.t = self.buf[U.GUARD:U.GUARD + size]

        def guards_ok(self):
            return bool((self.buf[:U.GUARD] == I64_SENTINEL).all() and (self.buf[U.GUARD + self.size:] == I64_SENTINEL).all())

    return GuardedI64(size)


def build(spec):
    """Nodes in depth-first order from a nested spec: ('leaf',) | ('one', child) | ('sw' | 'st', exit index | None, [children])
    -- 'sw' a switch with a router, 'st' a static fork; a child 'leaf' at the exit index is the exit."""
    tree, count = [], dict(leaf=0, sw=0)

    def visit(s):
        me = len(tree)
        tree.append(None)
        if s[0] == 'leaf':
            tree[me] = N(leaf=count['leaf'])
            count['leaf'] += 1
        elif s[0] == 'one':
            tree[me] = N([visit(s[1])])
        else:
            sw = -1
            if s[0] == 'sw':
                sw, count['sw'] = count['sw'], count['sw'] + 1
            nd = tree[me] = N([], sw, exit=-1 if s[1] is None else s[1])
            nd['sinks'] = [visit(c) for c in s[2]]
        return me
    visit(('one', spec))
    return tree


LEAF = ('leaf',)


def chain(k, kind='sw'):
    spec = ('one', LEAF)
    for _ in range(k - 1):
        spec = (kind, 0, [LEAF, spec])
    return spec


def tree15():
    def fork(i):
        kids = [('one', LEAF), ('one', LEAF)] if i == 2 else [fork(i + 1), fork(i + 1)]
        return ('sw', 0, [LEAF] + kids)
    return fork(0)


def mixed():
    """A switch whose exit sits in the middle sink, above: a static chain, and a switch WITHOUT an exit over a gated switch
    and a static fork whose exit is its second sink."""
    return ('sw', 1, [chain(3, 'st'), LEAF, ('sw', None, [('sw', 1, [('one', LEAF), LEAF]), ('st', 1, [('one', LEAF), LEAF])])])


TREES = {'chain2': chain(2), 'chain8': chain(8), 'static4': chain(4, 'st'), 'tree15': tree15(), 'mixed': mixed()}


class Case:
    def __init__(self, spec, n, T, seed, per_leaf=True, extra=0):
        import hiputil as U
        rng = np.random.default_rng(seed)
        self.tree = tree = build(spec)
        self.n, self.T, self.per_leaf = n, T, per_leaf
        NN = len(tree)
        self.nl = nl = sum(1 for nd in tree if not nd['sinks'])
        self.ns = ns = 1 + max(nd['switch'] for nd in tree)
        self.cs, self.ds, self.rs = n + 5 + extra, n + 3 + extra, (n + 2 + extra) * MS          # strides beyond n
        self.node_ops = rng.integers(1, 2 ** 40, NN).astype(np.int64)
        conf = rng.random((nl, self.cs)).astype(np.float32)
        conf[rng.random(conf.shape) < 0.08] = np.float32(NAN)
        d_cor = (rng.random((nl, self.ds)) < 0.5).astype(np.float32)
        r = np.full((max(ns, 1), self.rs // MS, MS), NAN, np.float32)
        for nd in tree:
            if nd['switch'] < 0:
                continue
            S, row = len(nd['sinks']), r[nd['switch']]
            row[:, :S] = rng.standard_normal((row.shape[0], S))
            for s in range(seed % 3, row.shape[0], 3):             # every third row: a planted tie
                how, top = (s // 3) % 4, np.float32(np.abs(row[s, :S]).max() + 1.0)
                if how == 0:
                    row[s, :S] = row[s, 0]
                elif how == 1:
                    row[s, rng.choice(S, size=2, replace=False)] = top
                elif how == 2:
                    row[s, rng.choice(S, size=min(S, 3), replace=False)] = top
                else:
                    row[s, :S] = np.where(rng.random(S) < 0.5, np.float32(0.0), np.float32(-0.0))
        # thresholds: per exit a confidence that occurs among the n images, at a random quantile; specials sprinkled in
        gated = [tree[nd['sinks'][nd['exit']]]['leaf'] for nd in tree if nd['exit'] >= 0]

        def occurring(l):
            c = conf[l, :n]
            c = c[~np.isnan(c)]
            return rng.choice(c) if len(c) else np.float32(0.5)
        if per_leaf:
            taus = np.full((T, nl), NAN, np.float32)               # (leaves no threshold applies to keep NaN)
            for t in range(T):
                for l in gated:
                    u = rng.random()
                    taus[t, l] = -INF if u < 0.08 else INF if u < 0.3 else NAN if u < 0.4 else occurring(l)
            taus[0, gated] = INF                                   # (the first point: everybody refused everywhere)
        else:
            taus = np.array([occurring(gated[t % len(gated)]) for t in range(T)], np.float32)
            taus[::5] = INF
            if T > 2:
                taus[1], taus[2] = -INF, NAN
        self.conf, self.d_cor, self.r, self.taus = conf, d_cor, r, taus
        self.d_conf, self.d_dcor, self.d_r, self.d_taus = U.Guarded(conf.size), U.Guarded(d_cor.size), U.Guarded(r.size), U.Guarded(taus.size)
        self.d_conf.fill(conf); self.d_dcor.fill(d_cor); self.d_r.fill(r); self.d_taus.fill(taus)
        self.host_tree = (_hip.CurveNode * NN)()
        for q, nd in zip(self.host_tree, tree):
            q.n_sinks, q.switch_id, q.leaf_id, q.exit_sink = len(nd['sinks']), nd['switch'], nd['leaf'], nd['exit']
            for i, s in enumerate(nd['sinks']):
                q.sink[i] = s
        self.d_tree = _hip.to_device_table(list(self.host_tree), U.DEV)
        self.d_ops = _guarded_i64(NN)
        self.d_ops.fill(self.node_ops)
        self.acc = _guarded_i64(T * (2 + nl))
        self.acc.t.zero_()

    def record(self, n=None, first=0):
        """The record over images first .. first + n - 1 (pointers shifted by `first` images)."""
        n = self.n if n is None else n
        a = _hip.ExitCurveArgs()
        a.n, a.n_nodes, a.n_leaves, a.n_switches, a.n_points, a.tau_per_leaf = n, len(self.tree), self.nl, self.ns, self.T, int(self.per_leaf)
        a.tree, a.node_ops = self.d_tree.data_ptr(), self.d_ops.ptr()
        a.conf, a.conf_stride = self.d_conf.ptr(first), self.cs
        a.d_cor, a.dcor_stride = self.d_dcor.ptr(first), self.ds
        a.r, a.r_stride, a.r_switch_stride = self.d_r.ptr(first * MS), MS, self.rs
        a.taus = self.d_taus.ptr()
        a.correct, a.ops, a.hist = self.acc.ptr(), self.acc.ptr(self.T), self.acc.ptr(2 * self.T)
        assert _hip.load().mpnn_exit_curve_check(C.byref(a), self.host_tree) == 0
        return a

    def launch(self, *recs):
        import torch
        import hiputil as U
        for a in recs or (self.record(),):
            assert _hip.load().mpnn_exit_curve(C.byref(a), U.stream()) == 0
        torch.cuda.synchronize()

    def got(self):
        out = self.acc.get()
        T = self.T
        return out[:T], out[T:2 * T], out[2 * T:].reshape(T, self.nl)

    def want(self, n=None):
        return R.curve(self.tree, self.node_ops, self.conf, self.d_cor, self.r, self.taus, self.n if n is None else n, self.nl)

    def check(self, want=None):
        want = self.want() if want is None else want
        for name, g, w in zip(('correct', 'ops', 'hist'), self.got(), want):
            assert g.dtype == np.int64 and np.array_equal(g, w), name
        for b in (self.d_conf, self.d_dcor, self.d_r, self.d_taus, self.d_ops, self.acc):
            assert b.guards_ok(), 'a guard changed'
        assert np.array_equal(self.d_conf.get().view(np.uint32), self.conf.reshape(-1).view(np.uint32))
        assert np.array_equal(self.d_r.get().view(np.uint32), self.r.reshape(-1).view(np.uint32))
        return want


@pytest.mark.parametrize('name', list(TREES))
@pytest.mark.parametrize('n', SIZES)
def test_curve_equals_the_reference(name, n):
    for T in POINTS:
        q = Case(TREES[name], n, T, seed=n * 7 + T)
        q.launch()
        q.check()


@pytest.mark.parametrize('name', list(TREES))
def test_every_leaf_is_taken_at_some_point(name):
    """600 images, 33 points: every leaf of every tree has a non-zero histogram entry at some point, the points differ, and
    first point (+inf everywhere: nobody leaves by confidence) is among them."""
    q = Case(TREES[name], 600, 33, seed=5)
    q.launch()
    correct, ops, hist = q.check()
    assert (hist.sum(1) == 600).all() and (hist.max(0) > 0).all(), hist.max(0)
    assert len({tuple(h) for h in hist.tolist()}) >= 10 and len(set(ops.tolist())) >= 10
    assert 0 < correct.min() and correct.max() < 600


@pytest.mark.parametrize('name', ['chain8', 'static4', 'mixed'])
@pytest.mark.parametrize('n,T', [(65, 2), (257, 33)])
def test_broadcast_thresholds(name, n, T):
    q = Case(TREES[name], n, T, seed=n + T, per_leaf=False)
    assert q.taus.shape == (T,)
    q.launch()
    _, _, hist = q.check()
    if T == 33:
        assert (hist.max(0) > 0).sum() >= 3


@pytest.mark.parametrize('name', ['chain8', 'tree15', 'mixed'])
def test_two_launches_add_up_to_one_over_the_concatenation(name):
    q = Case(TREES[name], 600, 5, seed=11)
    q.launch(q.record(257, 0), q.record(343, 257))
    q.check()
    first = R.curve(q.tree, q.node_ops, q.conf, q.d_cor, q.r, q.taus, 257, q.nl)
    assert not np.array_equal(first[2], q.got()[2])                 # (the second launch did add)
    q.launch(q.record(600, 0))                                     # ... and a third keeps adding
    q.check([2 * w for w in q.want()])


def test_nan_confidences_and_special_thresholds():
    """Every confidence NaN: -inf, +inf, an ordinary value and NaN all refuse; the NaN row is the routers' own choice."""
    q = Case(TREES['chain8'], 130, 4, seed=3)
    q.conf[:] = np.float32(NAN)
    q.d_conf.fill(q.conf)
    q.taus[:] = np.array([-INF, INF, 0.5, NAN], np.float32)[:, None]
    q.d_taus.fill(q.taus)
    q.launch()
    _, _, hist = q.check()
    assert hist[0].tolist() == hist[1].tolist() == hist[2].tolist() == [0] * 7 + [130]
    assert (hist[3][:3] > 0).all()
    # the same with finite confidences: -inf takes everybody but the NaNs at exit 0
    p = Case(TREES['chain8'], 130, 4, seed=3)
    p.taus[:] = np.array([-INF, INF, 0.5, NAN], np.float32)[:, None]
    p.d_taus.fill(p.taus)
    p.launch()
    _, _, hist = p.check()
    nan0 = int(np.isnan(p.conf[0, :130]).sum())
    assert nan0 > 0 and hist[0][0] == 130 - nan0 and hist[1].tolist() == [0] * 7 + [130]


def test_more_leaves_than_the_staged_confidences_hold():
    """A chain of 60 exits: 59 switches, 60 leaves -- beyond what a workgroup stages in LDS beside the switch bytes; the
    confidences of the last leaves come from global memory."""
    q = Case(chain(60), 300, 3, seed=2)
    assert q.nl == 60 and q.ns == 59 and len(q.tree) == 121 <= _hip.MAX_NODES
    q.taus[1, :] = -INF
    for t, l in enumerate((58, 50)):                               # leave late: refuse everywhere, accept everything at one deep exit
        q.taus[2 * t] = INF
        q.taus[2 * t, l] = -INF
    q.d_taus.fill(q.taus)
    q.launch()
    _, _, hist = q.check()
    assert hist[0][58] > 200 and hist[2][50] > 200 and hist[0][59] > 0


def test_nothing_to_do_is_no_launch():
    q = Case(TREES['chain2'], 64, 2, seed=1)
    a = q.record()
    a.n = 0
    q.launch(a)
    q.check([np.zeros_like(w) for w in q.want()])
