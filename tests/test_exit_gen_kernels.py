"""GPU: the any-width exit kernels (csrc/exit_gen.hip), each entry point alone through the C ABI against the explicit
float64 reference of tests/exit_ref.py:

  mpnn_lin_fwd_gen / mpnn_lin_bwd_gen              the cases of exit_ref.LIN_CASES, and three records in one table
  mpnn_exit_tail_fwd_gen / mpnn_exit_tail_bwd_gen  the cases of exit_ref.TAIL_CASES: the backward runs on the forward's
                                                   own h2 and bn_save
  mpnn_exit_ev_gen                                 router tail, r and the children's sample lists (the head alone:
                                                   tests/test_predict_kernels.py)

The contract every launch here keeps, as the engine does: mpnn_exit_gen_check runs on EVERY record before its table is
launched.  The records live in device memory, so the launchers cannot read their widths; the check keeps the widest
column-tile count of the process, and that count sizes the grid of mpnn_lin_fwd_gen and mpnn_exit_ev_gen for every
record of every table.  A record launched without it can lose its last column tiles.

Every output lives in a hiputil.Guarded buffer filled with NaN: after a launch the guards are intact, every element
that must be written is finite and every other element is still NaN (rows beyond a record's own n, the padding columns
of r, images outside an evaluation list, the k_cpt row of dW without extra_col).  Every case runs twice on fresh
buffers and must give the same bits: none of these kernels adds floats atomically.

Tolerances, element by element, against `bound` = the sum of the absolute values of the element's own terms in the
reference (tests/test_conv_gen.py::_close); never a max-norm, never taken from the kernel's output:
  2e-6 * bound + 1e-6        forward MFMA sums (y)
  4e-6 * bound + 1e-6        gradient sums (dW, db, dx of the affine maps; dbias3, dw3)
  2e-5 * (1 + |ref|)         statistics, moving averages, c_err, h2, r
  2e-5 * bound + 1e-9        dz (a softmax gradient: expf's error, no BatchNorm behind it)
  1e-4 * bound + 1e-6        gradients that pass a BatchNorm backward (dh2, dh1, dg*, db*, dbias2, dw2)
These are the project's constants.  The same reference evaluated in numpy float32 stays below 0.2 of every limit
over both case tables, K = 4112 and 1024 classes included (worst error / limit: dw3 0.16, y 0.13, dz 0.03, r 0.015;
error / bound at most 1e-6 for every sum), so none of them had to be widened.
d_cor is exact wherever the reference's top-two probability gap exceeds 1e-4 (check_label_free's rule).

ReLU masks: every tail case carries a seed for which both router BatchNorms' outputs lie at least 1e-4 from zero in
float64 (asserted on the CPU: tests/test_exit_ref_cpu.py); before any gradient is compared, the masks recomputed in
float64 from the device's own h2 and bn_save must equal the reference's -- no element is excluded from a comparison.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lib import _hip
from hiputil import DEV, Guarded, bn_dict, dev, stream
import exit_ref as X
from test_predict_kernels import Exit, check_label_free, launch_table

MODES = {'identity': _hip.ACT_IDENTITY, 'batch': _hip.ACT_BN_BATCH, 'moving': _hip.ACT_BN_MOVING}
fwd_lim = lambda ref, bound: 2e-6 * bound + 1e-6
grad_lim = lambda ref, bound: 4e-6 * bound + 1e-6
stat_lim = lambda ref, bound=None: 2e-5 * (1 + np.abs(ref))
dz_lim = lambda ref, bound: 2e-5 * bound + 1e-9
bn_lim = lambda ref, bound: 1e-4 * bound + 1e-6


def nan_buf(size, dtype=torch.float32):
    g = Guarded(size, dtype)
    g.fill(np.nan)
    return g


def written(g, must, what):
    """The buffer's contents shaped like `must`: guards intact, finite exactly where `must`, NaN everywhere else."""
    assert g.guards_ok(), what + ': written outside the buffer'
    a = g.get().reshape(must.shape)
    assert np.isfinite(a[must]).all(), what + ': an element that must be written is not finite'
    assert np.isnan(a[~must]).all(), what + ': an element that must not be written was'
    return a


def rows(n, n_max, width):
    must = np.zeros((n_max, width), bool)
    must[:n] = True
    return must


def close(got, ref, lim, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / lim).max()) if err.size else 0.0
    print('%-40s worst error / limit %.3g' % (what, ratio))
    assert (err <= lim).all(), '%s: %d of %d elements beyond the limit, worst error / limit %.3g' % (what, int((err > lim).sum()), err.size, ratio)


def same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), '%s: %s differs between two launches' % (what, k)


# ---------------------------------------------------------------------------------------------------- affine maps
_lin_ref = {}


class Lin:
    """One record of mpnn_lin_fwd_gen / mpnn_lin_bwd_gen on the inputs of exit_ref.lin_inputs(case)."""

    def __init__(self, case):
        d = self.d = X.lin_inputs(case)
        if case not in _lin_ref:
            _lin_ref[case] = X.lin_ref(d)
        self.ref = _lin_ref[case]
        self.xd = dev(d['x'])
        bn, cnt = (None, 1) if d['mode'] == 'identity' else bn_dict(d['x'], d['gamma'], d['beta'], d['m_avg'], d['v_avg'])
        self.bn = bn
        self.act = _hip.act(self.xd, d['C'], MODES[d['mode']], 0, bn, cnt)
        self.t = {k: [dev(v) for v in d[k]] for k in ('w', 'b', 'dy')}
        self.kc = dev(d['kc'])

    def records(self, n_max, with_dx):
        """(mpnn_lin_fwd_args, mpnn_lin_bwd_args, outputs) on fresh NaN buffers: y [n_max, M], dw [K + 1, M], db [M], dx
        [n_max, K]."""
        d, t = self.d, self.t
        K = d['K']
        o = dict(y=[None, None], dw=[None, None], db=[None, None], dx=nan_buf(n_max * K) if with_dx else None)
        lf, lb = _hip.LinFwdArgs(), _hip.LinBwdArgs()
        for a in (lf, lb):
            a.a, a.HW, a.n, a.k_cpt, a.alpha_cpt = self.act, d['HW'], d['n'], self.kc.data_ptr(), X.ALPHA_CPT
        for s, M in enumerate(d['M']):
            lf.M[s] = lb.M[s] = M
            lf.extra_col[s] = lb.extra_col[s] = int(d['extra'][s])
            if not M:
                continue
            o['y'][s], o['dw'][s], o['db'][s] = nan_buf(n_max * M), nan_buf((K + 1) * M), nan_buf(M)
            lf.w[s], lf.b[s], lf.y[s] = t['w'][s].data_ptr(), t['b'][s].data_ptr(), o['y'][s].ptr()
            lb.w[s], lb.dy[s], lb.dw[s], lb.db[s] = t['w'][s].data_ptr(), t['dy'][s].data_ptr(), o['dw'][s].ptr(), o['db'][s].ptr()
        lb.dx = o['dx'].ptr() if with_dx else None
        return lf, lb, o

    def collect(self, o, n_max):
        """The outputs as host arrays, after the written / not written checks."""
        d = self.d
        n, K = d['n'], d['K']
        out = {}
        for s, M in enumerate(d['M']):
            if not M:
                continue
            out['y%d' % s] = written(o['y'][s], rows(n, n_max, M), 'y[%d]' % s)[:n]
            dw = written(o['dw'][s], rows(K + 1 if d['extra'][s] else K, K + 1, M), 'dW[%d]' % s)
            out['dw%d' % s] = dw[:K + 1 if d['extra'][s] else K]
            out['db%d' % s] = written(o['db'][s], np.ones(M, bool), 'db[%d]' % s)
        if o['dx'] is not None:
            out['dx'] = written(o['dx'], rows(n, n_max, K), 'dx')[:n]
        return out

    def compare(self, out):
        ref = self.ref
        for s, M in enumerate(self.d['M']):
            if M:
                close(out['y%d' % s], ref['y'][s][0], fwd_lim(*ref['y'][s]), 'y[%d]' % s)
                close(out['dw%d' % s], ref['dw'][s][0], grad_lim(*ref['dw'][s]), 'dW[%d]' % s)
                close(out['db%d' % s], ref['db'][s][0], grad_lim(*ref['db'][s]), 'db[%d]' % s)
        if 'dx' in out:
            close(out['dx'], ref['dx'][0], grad_lim(*ref['dx']), 'dx')


def run_lin(lins, with_dx):
    """One mpnn_lin_fwd_gen and one mpnn_lin_bwd_gen launch over the records of `lins` (n_max / k_max: the maxima)."""
    lib = _hip.load()
    n_max, k_max = max(l.d['n'] for l in lins), max(l.d['K'] for l in lins)
    recs = [l.records(n_max, with_dx) for l in lins]
    for l in lins:
        M0, M1 = l.d['M']
        assert lib.mpnn_exit_gen_check(l.d['C'], l.d['K'], M0, M1, M1, 2 if M1 else 0) == 0
    tf, tb = _hip.to_device_table([r[0] for r in recs], DEV), _hip.to_device_table([r[1] for r in recs], DEV)
    _hip.check(lib.mpnn_lin_fwd_gen(tf.data_ptr(), len(lins), n_max, stream()), 'lin_fwd_gen')
    _hip.check(lib.mpnn_lin_bwd_gen(tb.data_ptr(), len(lins), n_max, k_max, stream()), 'lin_bwd_gen')
    torch.cuda.synchronize()
    return [l.collect(r[2], n_max) for l, r in zip(lins, recs)]


def check_lin(lins):
    first, again, bare = run_lin(lins, True), run_lin(lins, True), run_lin(lins, False)
    for l, a, b, c in zip(lins, first, again, bare):
        same_bits(a, b, 'affine maps')
        l.compare(a)
        assert 'dx' in a and 'dx' not in c
        same_bits(c, {k: a[k] for k in c}, 'affine maps without dx')           # dx == NULL: dW, db (and y) bit for bit


@pytest.mark.parametrize('case', X.LIN_CASES, ids=lambda c: 'n%d-hw%d-c%d-%s-m%d-%d%s' % c)
def test_lin_gen(case):
    """mpnn_lin_fwd_gen / mpnn_lin_bwd_gen alone (mpnn_exit_gen_check first: it sizes the forward grid), with dx and
    without."""
    check_lin([Lin(case)])


def test_lin_gen_table():
    """Three records of different n, K and widths in one table, one without a head and one without a router: n_max and
    k_max are the maxima, rows at or beyond a record's own n stay untouched."""
    check_lin([Lin(c) for c in X.LIN_MULTI])


# ---------------------------------------------------------------------------------------------------- exit tail
_tail_ref = {}
GRADS = ('dg1', 'db1', 'dw2', 'dbias2', 'dg2', 'db2', 'dw3', 'dbias3')


class Tail:
    """One record of mpnn_exit_tail_fwd_gen / _bwd_gen on the inputs of exit_ref.tail_inputs(name).  clear: the sizes
    (floats, doubles) of the accumulators the record's head workgroup clears, with a schedule row to copy.  table: the
    case table `name` is from (None: exit_ref.TAIL_CASES).  DH2: the backward writes dh2 (the tuned form, tests/
    test_exit_tuned_kernels.py, never does: its buffer must stay NaN)."""
    DH2 = True

    def __init__(self, name, clear=None, table=None):
        d = self.d = X.tail_inputs(name, table=table)
        if name not in _tail_ref:
            f = X.tail_fwd(d)
            g = X.tail_bwd(d, f.get('h2'), X.split_save(f['bn_save'], d['R'], d['R2']) if d['router'] else None) \
                if d['mode'] == 'batch' else None
            _tail_ref[name] = (f, g)
        self.ref, self.gref = _tail_ref[name]
        self.t = {k: dev(d[k]) for k in ('z', 'y', 'w_cerr', 'h1', 'g1', 'b1', 'w2', 'bias2', 'g2', 'b2', 'w3', 'bias3') if k in d}
        self.clear = clear
        if clear:
            self.hyp = np.random.default_rng(5).standard_normal(_hip.HYP_N).astype(np.float32)
            self.hyp_d = dev(self.hyp)

    def records(self, n_max):
        d, t = self.d, self.t
        n, nc, R, R2, S, st = d['n'], d['nc'], d['R'], d['R2'], d['S'], d['stride']
        o = {}
        tf, tb = _hip.ExitTailArgs(), _hip.ExitTailBwdArgs()
        tf.n, tf.mode, tf.n_cls, tf.eps_ce = n, MODES[d['mode']], nc, d['eps_ce']
        tf.R, tf.R2, tf.n_sinks, tf.r_stride = R, R2, S, st
        tf.bn_eps, tf.bn_eps2, tf.bn_decay, tf.bn_decay2 = d['bn_eps'], d['bn_eps2'], d['bn_decay'], d['bn_decay2']
        if d['head']:
            o.update(c_err=nan_buf(n_max), d_cor=nan_buf(n_max), dz=nan_buf(n_max * nc))
            tf.z, tf.y, tf.c_err, tf.d_cor = t['z'].data_ptr(), t['y'].data_ptr(), o['c_err'].ptr(), o['d_cor'].ptr()
            tb.w_cerr, tb.dz = t['w_cerr'].data_ptr(), o['dz'].ptr()
        if d['router']:
            o.update(h2=nan_buf(n_max * R2), r=nan_buf(n_max * st), bn_save=nan_buf(2 * R + 2 * R2), dh1=nan_buf(n_max * R),
                     dh2=nan_buf(n_max * R2), dg1=nan_buf(R), db1=nan_buf(R), dw2=nan_buf(R * R2), dbias2=nan_buf(R2),
                     dg2=nan_buf(R2), db2=nan_buf(R2), dw3=nan_buf(R2 * S), dbias3=nan_buf(S))
            for k, w in (('m1', R), ('v1', R), ('m2', R2), ('v2', R2)):       # (read and written: the averages start from the inputs)
                o[k] = Guarded(w)
                o[k].fill(d[k])
                setattr(tf, k, o[k].ptr())
            for k in ('h1', 'g1', 'b1', 'w2', 'bias2', 'g2', 'b2', 'w3', 'bias3'):
                setattr(tf, k, t[k].data_ptr())
            tf.h2, tf.r, tf.bn_save = o['h2'].ptr(), o['r'].ptr(), o['bn_save'].ptr()
            drp = np.zeros((n_max, st), np.float32)
            drp[:n, :S] = d['dr']
            self.dr_d = dev(drp)
            tb.dr, tb.dh1, tb.dh2 = self.dr_d.data_ptr(), o['dh1'].ptr(), o['dh2'].ptr()
            for k in GRADS:
                setattr(tb, k, o[k].ptr())
        if self.clear:
            nf, nd = self.clear
            o.update(clear_f=Guarded(nf + 16), clear_d=Guarded(nd + 4, torch.float64), hyp=Guarded(_hip.HYP_N + 8))
            for k in ('clear_f', 'clear_d', 'hyp'):
                o[k].fill(5.0)
            tf.clear_f, tf.n_clear_f, tf.clear_d, tf.n_clear_d = o['clear_f'].ptr(), nf, o['clear_d'].ptr(), nd
            tf.hyp_src, tf.hyp_dst = self.hyp_d.data_ptr(), o['hyp'].ptr()
        return tf, tb, o

    def collect(self, o, n_max):
        d = self.d
        n, nc, R, R2, S, st = d['n'], d['nc'], d['R'], d['R2'], d['S'], d['stride']
        bwd = d['mode'] == 'batch'
        out = {}
        if d['head']:
            for k in ('c_err', 'd_cor'):
                out[k] = written(o[k], rows(n, n_max, 1), k)[:n, 0]
            out['dz'] = written(o['dz'], rows(n if bwd else 0, n_max, nc), 'dz')[:n]
        if d['router']:
            out['h2'] = written(o['h2'], rows(n, n_max, R2), 'h2')[:n]
            must = rows(n, n_max, st)
            must[:, S:] = False
            out['r'] = written(o['r'], must, 'r')[:n, :S]
            out['bn_save'] = written(o['bn_save'], np.ones(2 * R + 2 * R2, bool), 'bn_save')
            for k in ('m1', 'v1', 'm2', 'v2'):
                assert o[k].guards_ok(), k
                out[k] = o[k].get()
            for k, w in (('dh1', R), ('dh2', R2)):
                out[k] = written(o[k], rows(n if bwd and (k != 'dh2' or self.DH2) else 0, n_max, w), k)[:n]
            for k in GRADS:
                out[k] = written(o[k], np.full(o[k].size, bwd), k)
        if self.clear:
            nf, nd = self.clear
            for k, m, want in (('clear_f', nf, 0.0), ('clear_d', nd, 0.0), ('hyp', _hip.HYP_N, self.hyp)):
                a = o[k].get()
                assert o[k].guards_ok() and np.array_equal(a[:m], np.zeros(m) + want), k + ': its range was not cleared / copied'
                assert (a[m:] == 5.0).all(), k + ': written beside its range'
        return out

    def compare(self, out):
        d, ref, g = self.d, self.ref, self.gref
        name, R, R2, S = d['name'], d['R'], d['R2'], d['S']
        if d['head']:
            close(out['c_err'], ref['c_err'], stat_lim(ref['c_err']), name + ' c_err')
            sure = ref['gap'] > 1e-4
            assert sure.sum() >= 0.9 * d['n']
            assert np.array_equal(out['d_cor'][sure], ref['d_cor'][sure]), name + ' d_cor'
            assert np.isin(out['d_cor'], (0.0, 1.0)).all()
        if d['router']:
            for k in ('h2', 'r', 'bn_save'):
                close(out[k], ref[k], stat_lim(ref[k]), '%s %s' % (name, k))
            for k, want in zip(('m1', 'v1', 'm2', 'v2'), ref['avg']):
                if d['mode'] == 'moving':
                    assert np.array_equal(out[k], d[k]), name + ': evaluation mode changed a moving average'
                else:
                    close(out[k], want, stat_lim(want), '%s moving %s' % (name, k))
        if g is None:
            return
        if d['router']:
            # the ReLU masks of the device's own h2 and statistics, in float64: a difference is a failure of this seed
            on = X.masks(d, out['h2'], X.split_save(out['bn_save'], R, R2))
            want = (ref['pre1'] > 0, ref['pre2'] > 0)
            assert all(np.array_equal(a, b) for a, b in zip(on, want)), \
                '%s, seed %d: a ReLU mask of the device differs from the reference\'s' % (name, d['seed'])
            for k in ('dbias3', 'dw3'):
                close(out[k].reshape(g[k][0].shape), g[k][0], grad_lim(*g[k]), '%s %s' % (name, k))
            for k in ('dh2', 'dh1', 'dg1', 'db1', 'dw2', 'dbias2', 'dg2', 'db2')[0 if self.DH2 else 1:]:
                close(out[k].reshape(g[k][0].shape), g[k][0], bn_lim(*g[k]), '%s %s' % (name, k))
        if d['head']:
            close(out['dz'], g['dz'][0], dz_lim(*g['dz']), name + ' dz')


def run_tail(tails):
    """mpnn_exit_tail_fwd_gen over the records, then (batch-statistics mode) mpnn_exit_tail_bwd_gen on the forward's own
    h2 and bn_save."""
    lib = _hip.load()
    n_max = max(t.d['n'] for t in tails)
    recs = [t.records(n_max) for t in tails]
    for t in tails:
        d = t.d
        assert lib.mpnn_exit_gen_check(16, 256, d['nc'] if d['head'] else 0, d['R'], d['R2'], d['S']) == 0
    tf = _hip.to_device_table([r[0] for r in recs], DEV)
    _hip.check(lib.mpnn_exit_tail_fwd_gen(tf.data_ptr(), len(tails), n_max, stream()), 'exit_tail_fwd_gen')
    torch.cuda.synchronize()
    if all(t.d['mode'] == 'batch' for t in tails):
        for r in recs:
            r[1].f = r[0]
        tb = _hip.to_device_table([r[1] for r in recs], DEV)
        _hip.check(lib.mpnn_exit_tail_bwd_gen(tb.data_ptr(), len(tails), n_max, stream()), 'exit_tail_bwd_gen')
        torch.cuda.synchronize()
    return [t.collect(r[2], n_max) for t, r in zip(tails, recs)]


def check_tail(tails):
    first, again = run_tail(tails), run_tail(tails)
    for t, a, b in zip(tails, first, again):
        same_bits(a, b, t.d['name'])
        t.compare(a)
    return first


@pytest.mark.parametrize('name', [k for k in X.TAIL_CASES if not k.startswith('table')])
def test_exit_tail_gen(name):
    """mpnn_exit_tail_fwd_gen, then mpnn_exit_tail_bwd_gen on its h2 and bn_save (mpnn_exit_gen_check on the record
    first, as for every launch of the any-width forms).  'moving': evaluation mode, forward only."""
    out = check_tail([Tail(name)])[0]
    if name == 'one':                                      # zero variance: both input gradients are exactly zero
        assert not out['dh1'].any() and not out['dh2'].any()


def test_exit_tail_gen_table():
    """Two records of different n and widths in one table, each with accumulators to clear (37 floats and 5 doubles;
    21 and 3) and a schedule row to copy, as the records of a co-trained group carry them (lib/_co.py: one per net):
    exactly those ranges are cleared / copied, for every record, nothing beside them."""
    check_tail([Tail('table0', clear=(37, 5)), Tail('table1', clear=(21, 3))])


# ---------------------------------------------------------------------------------------------------- evaluation router
# (seed, N, count, C, nc, R, R2, S, dyn, head, router, sinks with a list)
EV_CASES = {
    'full-200':   (11, 200, 200, 32, 10, 32, 24, 3, True, True, True, (1, 2)),       # three tail workgroups of 64, the last ragged
    'wide-150':   (12, 200, 150, 32, 17, 256, 256, 4, False, True, True, (0, 1, 3)), # both router limits; a sink without a list
    'wide-dyn':   (13, 70, 41, 16, 10, 256, 256, 4, True, True, True, (1, 2, 3)),
    'no-head':    (14, 70, 41, 32, 10, 32, 24, 3, True, False, True, (1, 2)),
    'no-router':  (15, 70, 41, 32, 100, 32, 24, 3, False, True, False, ()),
}


def make_ev(name):
    seed, N, count, C_, nc, R, R2, S, dyn, head, router, lists = EV_CASES[name]
    return Exit(seed, N=N, count=count, C_=C_, nc=nc, R=R, R2=R2, S=S, dyn=dyn, head=head, router=router, eps=(1e-6, 1e-3)), lists


def check_ev(ex, lists, out, what):
    idx, S, N = ex.idx, ex.S, ex.N
    rest = np.setdiff1d(np.arange(N), idx)
    cn = out['counts']
    if ex.router:
        ref = ex.router_reference()
        assert np.isfinite(out['r'][idx][:, :S]).all() and np.isnan(out['r'][idx][:, S:]).all(), what + ': r of the listed images'
        close(out['r'][idx][:, :S], ref[idx], stat_lim(ref[idx]), what + ' r')
        arg = np.argmax(out['r'][idx][:, :S], 1)                               # (first index on ties)
        top = np.sort(ref[idx], 1)
        sure = top[:, -1] - top[:, -2] > 1e-4
        assert sure.sum() >= 0.9 * len(idx) and np.array_equal(arg[sure], ref[idx].argmax(1)[sure]), what + ': arg-max sink'
        for i in range(_hip.MAX_SINKS):
            want = np.sort(idx[arg == i]) if i in lists else np.zeros(0, np.int32)
            assert cn[i] == len(want), '%s: sink %d holds %d samples, not %d' % (what, i, cn[i], len(want))
            assert np.array_equal(np.sort(out['lists'][i][:cn[i]]), want), '%s: list of sink %d' % (what, i)
            assert (out['lists'][i][cn[i]:] == -1).all(), '%s: written behind the list of sink %d' % (what, i)
        assert len(lists) < S or sum(cn) == len(idx)
    else:
        assert np.isnan(out['r']).all() and not cn.any() and (out['lists'] == -1).all(), what + ': a record without a router routed'
    assert np.isnan(out['r'][rest]).all(), what + ': r outside the list'
    assert np.isnan(out['c_err'][rest]).all() and np.isnan(out['d_cor'][rest]).all(), what + ': head outputs outside the list'
    if ex.head:
        z = np.log(ex.reference()[idx])                                        # (log-softmax: the same cross-entropy)
        f = X.head_fwd(z, ex.y[idx], 1e-6)
        close(out['c_err'][idx], f['c_err'], stat_lim(f['c_err']), what + ' c_err')
        sure = f['gap'] > 1e-4
        assert np.array_equal(out['d_cor'][idx][sure], f['d_cor'][sure]), what + ' d_cor'
    else:
        assert np.isnan(out['c_err']).all() and np.isnan(out['d_cor']).all() and (out['cls'] == -1).all(), what + ': a record without a head classified'


@pytest.mark.parametrize('name', sorted(EV_CASES))
def test_exit_ev_gen_router(name):
    """mpnn_exit_ev_gen with a router tail: r on the listed images against float64, untouched elsewhere; each child's
    count exact and its list the images whose arg-max is that sink, in any order; nothing for a sink without a list; the
    head as check_label_free holds it.  Two launches give the same r, c_err and d_cor bits and the same lists as sets."""
    ex, lists = make_ev(name)
    a, b = ex.launch(True, labels=True, lists=lists), ex.launch(True, labels=True, lists=lists)
    check_ev(ex, lists, a, name)
    same_bits({k: a[k] for k in ('r', 'c_err', 'd_cor', 'cls', 'conf', 'p', 'counts')},
              {k: b[k] for k in ('r', 'c_err', 'd_cor', 'cls', 'conf', 'p', 'counts')}, name)
    assert np.array_equal(np.sort(a['lists'], 1), np.sort(b['lists'], 1))
    if ex.head:
        check_label_free(ex, gen=True)


def test_exit_ev_gen_table():
    """The five records in ONE table (capacities 200 and 70, lists of 200, 150 and 41): every record's outputs as above."""
    made = [make_ev(k) for k in sorted(EV_CASES)]
    lists = (1, 2)                                         # (one choice for the table: sinks 1 and 2 have a child)
    outs = launch_table([m[0] for m in made], True, labels=True, lists=lists)
    for k, (ex, _), out in zip(sorted(EV_CASES), made, outs):
        check_ev(ex, tuple(i for i in lists if i < ex.S) if ex.router else (), out, 'table/' + k)
