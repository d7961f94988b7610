"""CPU: the float64 references of tests/step_end_ref.py against independent answers, the coverage conditions of the
case tables the GPU tests run (tests/test_step_end_kernels.py, tests/test_route_forms.py), and the refusals of the
step-ending entry points that need no GPU.

  bn_finalize_ref   torch-CPU float64 BatchNorm: batch moments, and autograd's dgamma / dbeta, to 1e-10
  talr_ref          oracle/np_ops.momentum_step; torch.optim.SGD(momentum) over three steps for l2 = 0, talr = 0
  pack_ref          the index formulas of include/mpnn_hip.h, element by element
  seg_path          every path of opt_seg's pack emission is taken by at least 10 work items of the case lists
  mpnn_route        no tree within MPNN_MAX_NODES / MPNN_MAX_SINKS selects 16 samples per workgroup
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_end_ref as R
from oracle import np_ops as O

REL = 1e-10


def same(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want)
    assert (err <= REL * (1 + np.abs(want))).all(), (what, float(err.max()))


# ---------------------------------------------------------------------------------------------------- BatchNorm
def test_bn_finalize_ref_against_torch_batchnorm():
    rng = np.random.default_rng(0)
    n, H, W, Cc = 5, 4, 3, 7
    x, dz = rng.standard_normal((n, H, W, Cc)) * 2 + 0.5, rng.standard_normal((n, H, W, Cc))
    gamma = rng.uniform(0.5, 1.5, Cc)
    m0, v0 = rng.standard_normal(Cc), rng.uniform(0.5, 2, Cc)
    ref = R.bn_finalize_ref(x, dz, gamma, m0, v0, 0.9, 1e-6)
    xt = torch.tensor(x).permute(0, 3, 1, 2)
    g = torch.tensor(gamma, requires_grad=True)
    b = torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.batch_norm(xt, None, None, g, b, True, 0.0, 1e-6)
    (y * torch.tensor(dz).permute(0, 3, 1, 2)).sum().backward()
    same(ref['mean'], xt.mean((0, 2, 3)).numpy(), 'mean')
    same(ref['var'], xt.var((0, 2, 3), unbiased=False).numpy(), 'biased variance')
    same(ref['dgamma'], g.grad.numpy(), 'dgamma')
    same(ref['dbeta'], b.grad.numpy(), 'dbeta')
    same(ref['m_avg'], 0.9 * m0 + 0.1 * xt.mean((0, 2, 3)).numpy(), 'moving mean')
    same(ref['v_avg'], 0.9 * v0 + 0.1 * xt.var((0, 2, 3), unbiased=False).numpy(), 'moving variance')
    # the slot layout: the rows add up to the totals, and no single row does
    for nslot in (1, 3, 16):
        sums, reds = R.spread_slots(x, dz, ref['xhat'], nslot, np.random.default_rng(nslot))
        assert sums.shape == reds.shape == (nslot, 2 * Cc)
        cnt = n * H * W
        same(sums.sum(0)[:Cc] / cnt, ref['mean'], 'sum x')
        same(sums.sum(0)[Cc:] / cnt - ref['mean'] ** 2, ref['var'], 'sum x^2')
        same(reds.sum(0), np.concatenate([ref['dbeta'], ref['dgamma']]), 'reductions')
        if nslot > 1:
            assert (np.abs(sums[0] - sums.sum(0)) > 1e-3).all() and (np.abs(reds[0] - reds.sum(0)) > 1e-6).all()


# ---------------------------------------------------------------------------------------------------- optimizer
def test_talr_ref_against_momentum_step_and_sgd():
    rng = np.random.default_rng(1)
    total, n = 50, 64
    P, A, G = (rng.standard_normal(total) for _ in range(3))
    p = rng.random((3, n)) * 0.9 + 0.01
    stat = np.stack([p.sum(1), (p ** 2).sum(1)], 1)
    eq = rng.standard_normal(20)
    items = [(0, 10, 0, 0, 0.0, -1), (10, 15, 1, 1, 1e-4, -1), (30, 20, 2, 0, 1e-3, 0)]      # [25, 30): no item
    lr, mu, artr = 0.05, 0.9, 1.7
    for talr in (0, 1):
        for gs in (1.0, 0.5):
            wp, wa = R.talr_ref(P, A, G, items, stat, lr, mu, artr, talr, 1.0 / n, gs, eq)
            for off, cnt, node, rt, l2, eo in items:
                sl = slice(off, off + cnt)
                pbar, p2 = p[node].mean(), (p[node] ** 2).mean()
                l2v = np.float64(np.float32(l2))
                grad = gs * G[sl] + 2 * l2v * pbar * (P[sl] - (eq[eo:eo + cnt] if eo >= 0 else 0))
                th, ac = O.momentum_step(P[sl], A[sl], grad, lr, mu, (p2 ** -0.5 if talr else 1.0) * (artr if rt else 1.0))
                same(wp[sl], th, 'parameters')
                same(wa[sl], ac, 'accumulators')
            assert np.array_equal(wp[25:30], P[25:30]) and np.array_equal(wa[25:30], A[25:30])
    # l2 = 0, talr = 0: plain SGD with momentum (torch: buf = mu * buf + g, w -= lr * buf), three steps
    w = torch.tensor(P.copy(), requires_grad=True)
    opt = torch.optim.SGD([w], lr=lr, momentum=mu)
    wp, wa = P.copy(), np.zeros(total)
    for step in range(3):
        g = rng.standard_normal(total)
        w.grad = torch.tensor(g)
        opt.step()
        wp, wa = R.talr_ref(wp, wa, g, [(0, total, 0, 0, 0.0, -1)], stat, lr, mu, artr, 0, 1.0 / n, 1.0)
        same(wp, w.detach().numpy(), 'SGD step %d' % step)


def test_pack_ref_against_the_header_formulas():
    rng = np.random.default_rng(2)
    for ci, co in [(3, 16), (20, 32), (16, 10)]:
        w = rng.standard_normal((3, 3, ci, co)).astype(np.float32)
        fw, bw = R.pack_ref(w)
        assert fw.size == R.pack_sizes(ci, co)[0] and bw.size == R.pack_sizes(ci, co)[1]
        wf = w.reshape(9, ci, co)
        for tap in range(9):
            for ch in range(fw.shape[1]):
                for gb in range(4):
                    for j in range(4):
                        c = ch * 16 + 4 * gb + j
                        assert np.array_equal(fw[tap, ch, gb, :, j], wf[tap, c, :] if c < ci else np.zeros(co))
            for ch in range(bw.shape[1]):
                for gb in range(4):
                    for j in range(4):
                        o = ch * 16 + 4 * gb + j
                        assert np.array_equal(bw[tap, ch, gb, :, j], wf[8 - tap, :, o] if o < co else np.zeros(ci))


def test_opt_case_lists_cover_every_pack_path():
    """A condition on the INPUTS of test_step_end_kernels.py::test_optimizer_emits_the_packs (which asserts it again)."""
    from lib import _hip
    assert (R.BN_SLOTS, R.SEG_INTS) == (_hip.BN_SLOTS, _hip.SEG_INTS)
    tensors, psize, ksize = R.opt_layout()
    assert {(t['cin'], t['cout']) for t in tensors if t['cin']} == {(3, 16), (4, 16), (16, 16), (16, 128), (20, 32), (32, 16), (64, 64), (128, 128)}
    assert all((t['bwd'] >= 0) == (t['cin'] % 16 == 0) for t in tensors if t['cin'])
    total = {'tap': 0, 'taps': 0, 'slow': 0}
    for name, piece in R.OPT_LISTS.items():
        rows = R.opt_rows(piece, tensors)
        assert all(len(r) == R.SEG_INTS and 0 < r[1] <= piece for r in rows)
        covered = np.zeros(psize, int)
        for r in rows:
            covered[r[0]:r[0] + r[1]] += 1
        assert covered.max() == 1 and covered.sum() == sum(t['size'] for t in tensors)
        for k, v in R.path_counts(rows).items():
            total[k] += v
    assert min(total.values()) >= 10, total
    # the shapes the issue names: no whole row (R = 0), a first row off the 4-row grid, a ragged last item
    p64 = R.opt_rows(64, tensors)
    assert any(r[7] and r[1] // r[8] == 0 for r in p64)
    assert any(r[7] and ((r[0] - r[6]) // r[8]) % 4 for r in R.opt_rows(256, tensors))
    assert any(r[7] and r[1] < 64 for r in p64)
    # seg_path itself, on rows written out by hand ([3][3][16][16] at 100: 256 elements per tap)
    row = lambda off, cnt, cin=16, cout=16: [off, cnt, 0, 0, 0, -1, 100, cin, cout, 0, 0, 0]
    assert R.seg_path(row(100, 64)) == 'tap' and R.seg_path(row(100 + 192, 64)) == 'tap'
    assert R.seg_path(row(100 + 192, 128)) == 'slow'                 # four-row groups, but across a tap boundary
    assert R.seg_path(row(100, 512)) == 'taps' and R.seg_path(row(100 + 128, 512)) == 'slow'
    assert R.seg_path(row(100 + 32, 64)) == 'slow'                   # row0 = 2
    assert R.seg_path(row(100, 60)) == 'slow' and R.seg_path(row(100, 8)) == 'slow'
    assert R.seg_path(row(100, 4096)) == 'slow' and R.seg_path(row(100, 48, 3, 16)) == 'slow'
    assert R.seg_path([0, 64, 0, 0, 0, -1, 0, 0, 0, -1, -1, 0]) is None


# ---------------------------------------------------------------------------------------------------- refusals
def test_step_end_entry_points_refuse_bad_arguments():
    """Validated on the host before anything is launched (no GPU needed to be refused)."""
    from lib import _hip
    lib = _hip.load()
    mem = (C.c_char * 64)()
    p = C.addressof(mem)                       # a non-NULL pointer; a refused call never reads it
    fin = lambda ni, nb: lib.mpnn_backward_finish(p, p, p, ni, p, p, p, p, nb, 0.9, 1, None, None)
    assert fin(-1, 0) == fin(0, -1) == fin(-1, 1) == fin(2, -2) == _hip.E_ARG
    assert fin(0, 0) == 0

    def opt(ni, nb, npl, item_seg=p, bn_opt=p, plain_seg=p):
        return lib.mpnn_backward_finish_opt(p, p, ni, item_seg, p, p, p, p, nb, bn_opt, 0.9, 1, None,
                                            p, p, p, p, p, 0, 1.0, 1.0, None, None, plain_seg, npl, None)
    assert opt(-1, 0, 0) == opt(0, -1, 0) == opt(0, 0, -1) == opt(-1, 1, 0) == _hip.E_ARG
    assert opt(0, 0, 0) == 0
    assert opt(1, 0, 0, item_seg=None) == opt(0, 1, 0, bn_opt=None) == opt(0, 0, 1, plain_seg=None) == _hip.E_ARG
    # the multi form checks every net's record the same way
    f = (_hip.FinishNet * 2)()
    for k in range(2):
        for name in ('params', 'accum', 'grads', 'node_stat', 'hyp'):
            setattr(f[k], name, p)
    assert lib.mpnn_backward_finish_opt_multi(f, p, 2, 0.9, None) == 0          # (every count zero)
    f[1].n_plain = 1
    assert lib.mpnn_backward_finish_opt_multi(f, p, 2, 0.9, None) == _hip.E_ARG
    f[1].n_plain = -1
    assert lib.mpnn_backward_finish_opt_multi(f, p, 2, 0.9, None) == _hip.E_ARG
    # mpnn_route / mpnn_route_multi
    def rec(n=64, nn=3, ms=2):
        a = _hip.RouteArgs()
        a.n_nodes, a.n_leaves, a.n_switches, a.max_sinks, a.n, a.n_total = nn, 2, 1, ms, n, n
        a.nodes = a.p_tr = a.p_ev = p
        return a
    a = rec()
    a.stat_part = p
    assert lib.mpnn_route(C.byref(a), None) == _hip.E_ARG                      # stat_part without stat_ticket
    for other in (rec(n=65), rec(nn=4), rec(ms=3)):
        tab = (_hip.RouteArgs * 2)(rec(), other)
        assert lib.mpnn_route_multi(tab, p, 2, None) == _hip.E_ARG
    tab = (_hip.RouteArgs * 2)(rec(), a)
    assert lib.mpnn_route_multi(tab, p, 2, None) == _hip.E_ARG


# ---------------------------------------------------------------------------------------------------- route
def test_no_tree_selects_sixteen_samples_per_workgroup():
    """mpnn_route's RB=16 instantiation is unreachable: over every (n_switches, n_leaves, n_nodes) a tree within
    MPNN_MAX_NODES and MPNN_MAX_SINKS can have -- each switch has 2..4 sinks, so n_leaves - 1 = sum (sinks - 1) lies in
    [n_switches, 3 * n_switches], and n_nodes >= n_switches + n_leaves (the rest are one-sink nodes) -- declared with
    max_sinks = 4, the tables fit 160 KB at 32 samples."""
    from lib import _hip
    worst = (0, None)
    for ns in range(0, _hip.MAX_NODES):
        for nl in range(ns + 1 if ns else 1, 3 * ns + 2):
            if ns + nl > _hip.MAX_NODES:
                break
            for nn in range(ns + nl, _hip.MAX_NODES + 1):
                per, fix = R.route_lds_floats(nn, ns, nl, _hip.MAX_SINKS)
                assert R.route_rb(nn, ns, nl, _hip.MAX_SINKS) in (64, 32), (ns, nl, nn)
                worst = max(worst, ((per * 32 + fix) * 4, (ns, nl, nn)))
    # the largest: 63 switches (62 two-way, one three-way), 65 leaves, no one-sink node: 1209 floats per sample
    assert worst == ((1209 * 32 + 128 * 5 + 8 + 63) * 4, (63, 65, 128)) and worst[0] <= 160 * 1024
    assert R.route_lds_floats(128, 63, 64, 4)[0] == 1207                       # a static root over a full binary tree
    assert R.route_rb(122, 40, 81, 3) == 32 and R.route_lds_floats(122, 40, 81, 3)[0] == 930
