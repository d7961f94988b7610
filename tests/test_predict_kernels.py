"""GPU: the label-free exit heads and the selection kernel, through the C ABI.

  mpnn_exit_ev / mpnn_exit_ev_gen with y == NULL   cls / conf / p_cls by image, against a float64 numpy softmax
  the same record with labels as well              d_cor == (cls == arg-max y) exactly, cls identical in both launches
  ties                                             first index, also across the threads of a sample (any-width head)
  mpnn_ev_select                                   a hand-made 7-node tree against a numpy gather, exactly

Tolerances: cls is compared wherever the reference's top-two probability gap exceeds 1e-4; conf / p_cls within
2e-4 * (1 + max|ref|), the bound the project uses for exit outputs against the oracle (tests/test_routed_eval.py:
check_vs_oracle).  Rows of images outside the node's list must keep their poison."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lib import _hip
from hiputil import DEV, dev, stream

TOL = 2e-4


class Exit:
    """One exit record (head + router) on random inputs: N images in the buffers, the node's list holds `count` of them.
    dyn: the router's first map has the k_cpt column (extra_col); head / router = False: the record has none (w_head /
    w1 NULL); eps: the epsilons of the two router BatchNorms."""

    def __init__(self, seed, N, count, C_, nc, R, R2, S, HW=16, wh=None, bh=None, dyn=False, head=True, router=True,
                 eps=(1e-6, 1e-6)):
        rng = np.random.default_rng(seed)
        f = np.float32
        K = HW * C_
        self.N, self.count, self.nc, self.K = N, count, nc, K
        self.R, self.R2, self.S, self.dyn, self.head, self.router, self.eps = R, R2, S, dyn, head, router, eps
        self.x = rng.standard_normal((N, HW, C_)).astype(f)
        self.g, self.be = (rng.random(C_) + 0.5).astype(f), (rng.standard_normal(C_) * 0.2).astype(f)
        self.ma, self.va = (rng.standard_normal(C_) * 0.2).astype(f), (rng.random(C_) + 0.5).astype(f)
        self.wh = (rng.standard_normal((K, nc)) / np.sqrt(K) * 4).astype(f) if wh is None else wh.astype(f)
        self.bh = rng.standard_normal(nc).astype(f) if bh is None else bh.astype(f)
        self.y = np.eye(nc, dtype=f)[rng.integers(0, nc, N)]
        self.idx = rng.permutation(N)[:count].astype(np.int32)
        P = dict(w1=rng.standard_normal((K, R)) / np.sqrt(K), b1=rng.standard_normal(R),
                 g1=rng.random(R) + 0.5, be1=rng.standard_normal(R) * 0.3, m1=rng.standard_normal(R) * 0.2, v1=rng.random(R) + 0.5,
                 w2=rng.standard_normal((R, R2)) / 4, bias2=rng.standard_normal(R2) * 0.1,
                 g2=rng.random(R2) + 0.5, be2=rng.standard_normal(R2) * 0.3, m2=rng.standard_normal(R2) * 0.2, v2=rng.random(R2) + 0.5,
                 w3=rng.standard_normal((R2, S)) / 4, bias3=rng.standard_normal(S) * 0.1)
        if dyn:                                           # (drawn last: the records without it keep their inputs)
            P['w1'] = np.concatenate([P['w1'], rng.standard_normal((1, R)) / np.sqrt(K)])
        self.kc = rng.choice([0.0, 1e-9, 6.4e-8], N).astype(f) if dyn else np.full(N, np.nan, f)
        self.P = {k: v.astype(f) for k, v in P.items()}
        self.t = {k: dev(v) for k, v in self.P.items()}
        self.t.update(x=dev(self.x), wh=dev(self.wh), bh=dev(self.bh), y=dev(self.y), idx=dev(self.idx, torch.int32),
                      cnt=dev(np.array([count], np.int32), torch.int32), g=dev(self.g), be=dev(self.be), ma=dev(self.ma),
                      va=dev(self.va), z=torch.zeros((N, nc), device=DEV), h1=torch.zeros((N, R), device=DEV), kc=dev(self.kc))
        self.stride = nc + 3                              # (p_stride > n_cls: the padding must stay untouched)
        e = self.e = _hip.ExitEvArgs()
        t = self.t
        bn = dict(sum=None, gamma=t['g'], beta=t['be'], m_avg=t['ma'], v_avg=t['va'], eps=1e-6)
        e.a = _hip.act(t['x'], C_, _hip.ACT_BN_MOVING, 0, bn, 1)
        e.HW, e.n = HW, N
        e.w_head, e.b_head, e.n_cls, e.eps_ce = (t['wh'].data_ptr() if head else None), t['bh'].data_ptr(), nc, 1e-6
        e.w1, e.b1, e.R, e.R2, e.n_sinks = (t['w1'].data_ptr() if router else None), t['b1'].data_ptr(), R, R2, S
        e.extra_col, e.k_cpt, e.alpha_cpt = (1 if dyn else 0), t['kc'].data_ptr(), 1e7
        for k in ('g1', 'be1', 'm1', 'v1', 'w2', 'bias2', 'g2', 'be2', 'm2', 'v2', 'w3', 'bias3'):
            setattr(e, k, t[k].data_ptr())
        e.bn_eps, e.bn_eps2 = eps
        e.r_stride = 4
        e.idx, e.cnt = t['idx'].data_ptr(), t['cnt'].data_ptr()
        e.z, e.h1 = t['z'].data_ptr(), t['h1'].data_ptr()

    def launch(self, gen, labels, probs=True, lists=()):
        """One launch on poisoned outputs; returns dict(cls, conf, p, c_err, d_cor, r, lists, counts) as host arrays."""
        return launch_table([self], gen, labels, probs, lists)[0]

    def prepare(self, labels, probs, lists, spare_counters=False):
        """Fresh poisoned outputs in the record: NaN (cls, the lists: -1; the lists' counts: 0).  lists: the sinks that
        have a sample list (a child block) and its counter; spare_counters: the other sinks get a counter too, which must stay
        0 (mpnn_exit_ev_check refuses such a record, the any-width form takes it)."""
        e, N = self.e, self.N
        cls = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        conf = torch.full((N,), float('nan'), device=DEV)
        p = torch.full((N, self.stride), float('nan'), device=DEV)
        c_err, d_cor = torch.full((N,), float('nan'), device=DEV), torch.full((N,), float('nan'), device=DEV)
        e.cls, e.conf = cls.data_ptr(), conf.data_ptr()
        e.p_cls, e.p_stride = (p.data_ptr(), self.stride) if probs else (None, 0)
        e.y = self.t['y'].data_ptr() if labels else None
        e.c_err, e.d_cor = (c_err.data_ptr(), d_cor.data_ptr()) if labels else (None, None)
        r = torch.full((N, e.r_stride), float('nan'), device=DEV)
        e.r = r.data_ptr()
        li = torch.full((_hip.MAX_SINKS, N), -1, dtype=torch.int32, device=DEV)
        counts = torch.zeros(_hip.MAX_SINKS, dtype=torch.int32, device=DEV)
        for i in range(_hip.MAX_SINKS):
            e.child_idx[i] = li[i].data_ptr() if i in lists else None
            e.child_cnt[i] = counts[i:].data_ptr() if (i in lists or spare_counters) else None
        return dict(cls=cls, conf=conf, p=p, c_err=c_err, d_cor=d_cor, r=r, lists=li, counts=counts)

    def activated(self):
        """float64 relu(bn(x)) of every image, flattened [N, K]."""
        x = self.x.astype(np.float64)
        return np.maximum(self.g * (x - self.ma) / np.sqrt(self.va.astype(np.float64) + 1e-6) + self.be, 0).reshape(self.N, self.K)

    def router_reference(self):
        """float64 router outputs r of every image [N, S] (moving-average BatchNorms, each with its own epsilon)."""
        P = {k: v.astype(np.float64) for k, v in self.P.items()}
        h1 = self.activated() @ P['w1'][:self.K] + P['b1']
        if self.dyn:
            h1 = h1 + 1e7 * self.kc.astype(np.float64)[:, None] * P['w1'][self.K]
        a1 = np.maximum(P['g1'] * (h1 - P['m1']) / np.sqrt(P['v1'] + self.eps[0]) + P['be1'], 0)
        h2 = a1 @ P['w2'] + P['bias2']
        a2 = np.maximum(P['g2'] * (h2 - P['m2']) / np.sqrt(P['v2'] + self.eps[1]) + P['be2'], 0)
        return a2 @ P['w3'] + P['bias3']

    def reference(self):
        """float64 softmax rows of every image [N, nc]."""
        z = self.activated() @ self.wh.astype(np.float64) + self.bh
        ez = np.exp(z - z.max(1, keepdims=True))
        return ez / ez.sum(1, keepdims=True)


def launch_table(exits, gen, labels, probs=True, lists=()):
    """The records of `exits` as ONE table and one launch (n_max: the largest capacity); every record's outputs.
    mpnn_exit_gen_check runs on every record first, as the engine does: it sizes the any-width forms' grid."""
    lib = _hip.load()
    outs = [ex.prepare(labels, probs, lists, spare_counters=gen) for ex in exits]
    for ex in exits:
        e = ex.e
        if gen:
            assert lib.mpnn_exit_gen_check(e.a.C, ex.K, ex.nc if ex.head else 0, e.R if ex.router else 0, e.R2,
                                           e.n_sinks if ex.router else 0) == 0
        else:
            assert lib.mpnn_exit_ev_check(C.byref(e)) == 0
    tab = _hip.to_device_table([ex.e for ex in exits], DEV)
    _hip.check((lib.mpnn_exit_ev_gen if gen else lib.mpnn_exit_ev)(tab.data_ptr(), len(exits), max(ex.N for ex in exits), stream()),
               'exit_ev')
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in o.items()} for o in outs]


def check_label_free(ex, gen):
    idx, nc = ex.idx, ex.nc
    rest = np.setdiff1d(np.arange(ex.N), idx)
    ref = ex.reference()
    top = np.sort(ref, 1)
    gap = top[:, -1] - top[:, -2]
    free = ex.launch(gen, labels=False)
    sure = idx[gap[idx] > 1e-4]
    assert len(sure) >= 0.9 * len(idx)                    # (the comparison says something)
    assert np.array_equal(free['cls'][sure], ref.argmax(1)[sure])
    assert ((free['cls'][idx] >= 0) & (free['cls'][idx] < nc)).all()
    bound = TOL * (1 + np.abs(ref[idx]).max())
    assert np.abs(free['conf'][idx] - ref[idx].max(1)).max() <= bound
    assert np.abs(free['p'][idx][:, :nc] - ref[idx]).max() <= bound
    # conf is the probability of cls; nothing outside the list, nothing in the rows' padding
    assert np.array_equal(free['conf'][idx], free['p'][idx, free['cls'][idx]])
    assert (free['cls'][rest] == -1).all() and np.isnan(free['conf'][rest]).all() and np.isnan(free['p'][rest]).all()
    assert np.isnan(free['p'][:, nc:]).all()
    # the labelled launch of the same record: the same class, and d_cor is its comparison with the label
    lab = ex.launch(gen, labels=True)
    assert np.array_equal(lab['cls'], free['cls']) and np.array_equal(lab['conf'][idx], free['conf'][idx])
    assert np.array_equal(lab['p'][idx][:, :nc], free['p'][idx][:, :nc])
    assert np.array_equal(lab['d_cor'][idx], (lab['cls'][idx] == ex.y[idx].argmax(1)).astype(np.float32))
    assert np.isfinite(lab['c_err'][idx]).all() and np.isnan(lab['c_err'][rest]).all() and np.isnan(lab['d_cor'][rest]).all()
    # without p_cls: the same class and probability
    bare = ex.launch(gen, labels=False, probs=False)
    assert np.array_equal(bare['cls'], free['cls']) and np.array_equal(bare['conf'][idx], free['conf'][idx])


def test_exit_ev_label_free():
    """The tuned head: 37 images, a list of 29 (two workgroups of 16 samples, the second ragged)."""
    check_label_free(Exit(1, N=37, count=29, C_=16, nc=10, R=16, R2=16, S=2), gen=False)


@pytest.mark.parametrize('nc,count', [(17, 70), (100, 70), (17, 41), (100, 41)])
def test_exit_ev_gen_label_free(nc, count):
    """The any-width head: 17 classes (a ragged second column tile) and 100 (seven column tiles, several classes per
    thread), two workgroups of 64 samples (the second ragged), a full list and one shorter than the capacity."""
    check_label_free(Exit(nc + count, N=70, count=count, C_=32, nc=nc, R=32, R2=24, S=3), gen=True)


def test_ties_take_the_first_index():
    K = 16 * 16
    # all-zero head: every class ties
    ex = Exit(3, N=37, count=29, C_=16, nc=10, R=16, R2=16, S=2, wh=np.zeros((K, 10)), bh=np.zeros(10))
    out = ex.launch(False, labels=False)
    assert (out['cls'][ex.idx] == 0).all() and np.array_equal(out['conf'][ex.idx], np.full(29, 0.1, np.float32))
    # two identical columns made the maximum: the first of them
    rng = np.random.default_rng(4)
    wh = (rng.standard_normal((K, 10)) / 16).astype(np.float32)
    bh = rng.standard_normal(10).astype(np.float32)
    wh[:, 7] = wh[:, 3]
    bh[3] = bh[7] = 50.0
    ex = Exit(5, N=37, count=29, C_=16, nc=10, R=16, R2=16, S=2, wh=wh, bh=bh)
    out = ex.launch(False, labels=False)
    assert (out['cls'][ex.idx] == 3).all()
    assert np.array_equal(out['p'][ex.idx, 3], out['p'][ex.idx, 7])
    # the any-width head, 40 classes: columns 5 and 37 sit on different threads of a sample (5 and 37 % 16 = 5 would share
    # one -- HT = 16 threads take classes part, part + 16, ... -- so also 6 and 37, which do not)
    for a, b in ((5, 37), (6, 37)):
        K = 16 * 32
        wh = (rng.standard_normal((K, 40)) / 16).astype(np.float32)
        bh = rng.standard_normal(40).astype(np.float32)
        wh[:, b] = wh[:, a]
        bh[a] = bh[b] = 50.0
        ex = Exit(6, N=70, count=41, C_=32, nc=40, R=32, R2=24, S=3, wh=wh, bh=bh)
        out = ex.launch(True, labels=False)
        assert (out['cls'][ex.idx] == a).all(), (a, b)
        assert np.array_equal(out['p'][ex.idx, a], out['p'][ex.idx, b])


def test_ev_select_on_a_hand_made_tree():
    """7 nodes, 4 leaves (nodes 2, 4, 5, 6 in leaf order), 70 samples (two waves, a ragged workgroup): every leaf taken,
    sample 11 reaches two leaves (the first in leaf order wins), sample 23 reaches none."""
    lib = _hip.load()
    rng = np.random.default_rng(9)
    n, nn, nl, nc, cap, ps = 70, 7, 4, 10, 80, 12
    leaf_node = np.array([2, 4, 5, 6], np.int32)
    paths = {0: [0, 1, 2], 1: [0, 1, 3, 4], 2: [0, 1, 3, 5], 3: [0, 6]}
    take = rng.integers(0, nl, n)
    take[:4] = [0, 1, 2, 3]
    p_ev = np.zeros((nn, n), np.float32)
    for s in range(n):
        p_ev[paths[take[s]], s] = 1.0
    p_ev[:, 11] = 0.0
    p_ev[[0, 1, 3, 5, 6], 11] = 1.0                       # leaves 2 and 3 (nodes 5 and 6): leaf 2 wins
    p_ev[:, 23] = 0.0
    p_ev[[0, 1, 3], 23] = 1.0                             # no leaf
    ops = np.array([3, 1361664 + 4384, 2560, 2 ** 33 + 5, 7, 11, 13], np.int64)     # (beyond 32 bits, beyond fp32's integers)
    leaf_cls = rng.integers(0, nc, (nl, cap)).astype(np.int32)
    leaf_conf = rng.random((nl, cap)).astype(np.float32)
    leaf_p = rng.random((nl, cap, ps)).astype(np.float32)
    want_leaf = np.full(n, -1, np.int32)
    for l in range(nl - 1, -1, -1):
        want_leaf[p_ev[leaf_node[l]] == 1.0] = l
    assert set(want_leaf) == {-1, 0, 1, 2, 3} and want_leaf[11] == 2 and want_leaf[23] == -1
    ar, lc = np.arange(n), np.maximum(want_leaf, 0)
    none = want_leaf < 0
    want = dict(leaf=want_leaf, cls=np.where(none, -1, leaf_cls[lc, ar]), conf=np.where(none, 0, leaf_conf[lc, ar]).astype(np.float32),
                probs=np.where(none[:, None], 0, leaf_p[lc, ar, :nc]).astype(np.float32),
                ops=((p_ev == 1.0) * ops[:, None]).sum(0))
    d = dict(p_ev=dev(p_ev), ops=dev(ops, torch.int64), leaf_node=dev(leaf_node, torch.int32), leaf_cls=dev(leaf_cls, torch.int32),
             leaf_conf=dev(leaf_conf), leaf_p=dev(leaf_p))
    for with_probs in (True, False):
        out = dict(leaf=torch.full((n + 8,), -7, dtype=torch.int32, device=DEV), cls=torch.full((n + 8,), -7, dtype=torch.int32, device=DEV),
                   conf=torch.full((n + 8,), -7.0, device=DEV), probs=torch.full((n + 8, nc), -7.0, device=DEV),
                   ops=torch.full((n + 8,), -7, dtype=torch.int64, device=DEV))
        a = _hip.EvSelectArgs()
        a.n, a.n_nodes, a.n_leaves, a.n_cls = n, nn, nl, nc
        a.p_ev, a.node_ops, a.leaf_node = d['p_ev'].data_ptr(), d['ops'].data_ptr(), d['leaf_node'].data_ptr()
        a.leaf_cls, a.leaf_conf, a.leaf_stride = d['leaf_cls'].data_ptr(), d['leaf_conf'].data_ptr(), cap
        a.leaf, a.cls, a.conf, a.ops = (out[k].data_ptr() for k in ('leaf', 'cls', 'conf', 'ops'))
        if with_probs:
            a.leaf_p, a.p_stride, a.probs = d['leaf_p'].data_ptr(), ps, out['probs'].data_ptr()
        _hip.check(lib.mpnn_ev_select(C.byref(a), stream()), 'ev_select')
        torch.cuda.synchronize()
        for k in ('leaf', 'cls', 'conf', 'ops') + (('probs',) if with_probs else ()):
            got = out[k].cpu().numpy()
            assert np.array_equal(got[:n], want[k]), k
            assert (got[n:] == -7).all(), k               # nothing behind the n samples
        if not with_probs:
            assert (out['probs'].cpu().numpy() == -7).all()
    # probs without the leaves' rows is refused
    a.probs = out['probs'].data_ptr()
    assert lib.mpnn_ev_select(C.byref(a), stream()) == _hip.E_ARG
