"""GPU: the TUNED exit kernels (csrc/lin.hip, csrc/exit_tail.hip, the router half of csrc/exit_ev.hip), each entry point
alone through the C ABI against the explicit float64 reference of tests/exit_ref.py, on the shapes their dispatch
admits and tests/test_exit_kernels.py never draws.

The tuned domain (lib/_eng_alloc.py, `tuned = ...`; restated and asserted for every case on the CPU,
tests/test_exit_ref_cpu.py): C <= 128 in multiples of 16, K = H W C a multiple of 16, <= 16 classes, two equal router
layers of <= 16 units, <= 4 sinks.  Rectangular maps and the any-channel convs put 3x5, 1x1 and 2x3 maps of 48, 80,
96 and 112 channels into it.

  mpnn_lin_fwd / mpnn_lin_fwd_ks     exit_ref.TUNED_LIN_CASES (uneven K-slices: S = 2, 3, 5 with 22 / 23, 16 / 16 / 17,
  mpnn_lin_bwd / mpnn_lin_bwd_rs     18 x 4 + 19 blocks; channel counts that are no power of two; partly live feature
                                     blocks; the k_cpt row inside the last block and in one of its own; the fused
                                     reductions' wrap and slot choice; row groups Z = 3, 4, 7 < gridDim.z), and
                                     TUNED_LIN_MULTI as one table of records with different n, K and slice counts
  mpnn_exit_tail_fwd / _bwd          exit_ref.TUNED_TAIL_CASES and the four any-width cases inside the limits: R in
                                     {1, 3, 5, 8, 12, 16}, 2 / 3 / 10 / 16 classes, head-only, router-only, moving
                                     averages, n on both sides of 128; one table that runs the LDS-resident and the
                                     any-size kernels in one call, with per-record clearing and the schedule copy
  mpnn_exit_ev                       exit_ref.TUNED_EV_CASES (mpnn_exit_ev_check on every record first), each with its
                                     own list, an empty one and a full one, and the five in one table

Every output lives in a NaN-filled hiputil.Guarded buffer: guards intact, finite exactly where it must be written (rows
>= n, the k_cpt row of dW without extra_col, the padding of r, slots >= red_nslot, dh2 -- which the tuned backward
never writes -- all stay NaN).  The K-slice / row-split scratch is NaN-filled and its ticket counters are zero before
and after every launch.  Every launch runs twice on fresh buffers and gives the same bits, except the fused
reductions: they are float64 atomicAdds of several workgroups into a slot, so their last bits depend on the arrival
order, and they are held to their limit in both runs instead.  dW / db of the fused launch (dx == NULL) are the
unfused launch's bit for bit.  A record of a table equals itself launched alone with the same n_max bit for bit.

Limits: the constants of tests/test_exit_gen_kernels.py, per element against `bound`, none widened:
  2e-6 * bound + 1e-6     y
  4e-6 * bound + 1e-6     dW, db, dx, dz of the fused form, the fused reductions, dw3, dbias3
  2e-5 * (1 + |ref|)      statistics, moving averages, c_err, h2, r
  2e-5 * bound + 1e-9     dz of the head
  1e-4 * bound + 1e-6     what passes a BatchNorm backward
The float32 evaluation of the reference stays below 0.2 of each (asserted on the CPU; worst: dW 0.14, y 0.11).
A fused dz is compared with the reference's masked dx; where the float64 pre-activation lies within exit_ref.NEAR =
1e-5 of zero (at most 0.1 % of a case, asserted; the cases have at most 1.4e-5) either 0 or that element's dx passes,
and the reductions are compared for the mask so resolved.

Worst error / limit by quantity, measured on an MI355X (printed by `close`; none above 0.08, so no limit had to be
re-derived from a restated summation form):
  affine maps   y 0.073, dW 0.078, db 0.018, dx 0.047, fused dz 0.047, fused reductions 0.011
  exit tail     c_err 0.011, h2 0.030, r 0.037, bn_save 0.016, moving averages 0.003, dz 0.026, dw3 0.068, dbias3 0.006,
                dh1 0.0018, dw2 0.0027, dg2 0.0010, db2 0.0005, dbias2 0.0003, dg1 0.0002, db1 0.0001
  evaluation    r 0.011, c_err 0.022

What these tests catch and tests/test_exit_kernels.py does not: four mutated libraries (built aside, not kept), each
through both files once on an MI355X.  tests/test_exit_kernels.py passed (35 of 35) under all four.
  (a) lin_fwd_k, slice bounds slice * (nkb_all / S): the three cases with uneven slices (K = 720, 784, 1456) and the
      table fail on y of mpnn_lin_fwd_ks, error / limit ~1e4
  (b) lin_fwd_k, channel k & (C - 1): the five cases with C = 48, 80, 96, 112, the launch without scratch and the table
      fail on y
  (c) lin_bwd_k, channel (k0 + tid) & (C - 1) in both places: the same five cases and the table fail on dW
  (d) exit_tail_fwd_k, clearing and schedule copy only in workgroup 1: test_exit_tail_tuned_table fails (the second
      record's accumulators are not cleared)
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lib import _hip
from hiputil import DEV, Guarded, stream
import exit_ref as X
from test_exit_gen_kernels import Lin, Tail, check_ev, close, fwd_lim, grad_lim, nan_buf, rows, same_bits, written
from test_predict_kernels import Exit, check_label_free, launch_table

IGUARD = 16


def counters(size):
    """Zeroed int32 ticket counters between two guard regions."""
    t = torch.full((size + 2 * IGUARD,), 12345, dtype=torch.int32, device=DEV)
    t[IGUARD:IGUARD + size] = 0
    return t


def counters_ok(t, what):
    a = t.cpu().numpy()
    assert (a[:IGUARD] == 12345).all() and (a[-IGUARD:] == 12345).all(), what + ': written beside the ticket counters'
    assert not a[IGUARD:-IGUARD].any(), what + ': a ticket counter is not back at zero'


# ---------------------------------------------------------------------------------------------------- affine maps
ENTRIES = ('fwd', 'fwd_ks', 'bwd', 'bwd_rs')
_fused_ref = {}


class TunedLin(Lin):
    """One record of mpnn_lin_fwd(_ks) / mpnn_lin_bwd(_rs) on the inputs of exit_ref.lin_inputs(case)."""

    def __init__(self, case):
        super().__init__(case)
        if self.d['mode'] == 'batch':
            if case not in _fused_ref:
                _fused_ref[case] = X.lin_fused(self.d, self.ref)
            self.fz = _fused_ref[case]

    def tuned_records(self, n_max, entry, fused=0, scratch=True):
        """The record of `entry` on fresh buffers.  fused: 0, or red_nslot of the fused form (dx == NULL, dz_out and
        red_out given).  scratch: fwd_ks -- where the engine gives it (K >= 512); bwd_rs -- always."""
        d = self.d
        n, K, C_ = d['n'], d['K'], d['C']
        lf, lb, o = self.records(n_max, with_dx=not fused)
        if entry == 'fwd_ks' and scratch and K >= 512:
            rg = (n + 15) // 16
            o['kpart'], o['kcnt'] = nan_buf(rg * _hip.LIN_KSLICES * 512), counters(rg)
            lf.kpart, lf.kcnt = o['kpart'].ptr(), o['kcnt'][IGUARD:].data_ptr()
        if entry == 'bwd_rs':
            nblk = (K + 1 + 63) // 64
            o['kpart'], o['kcnt'] = nan_buf(nblk * _hip.LIN_RSPLIT * _hip.LIN_RS_TILE), counters(nblk)
            lb.kpart, lb.kcnt = o['kpart'].ptr(), o['kcnt'][IGUARD:].data_ptr()
        if fused:
            o['dz'] = nan_buf(n_max * K)
            o['red'] = Guarded(_hip.BN_SLOTS * 2 * C_, torch.float64)
            o['red'].fill(np.nan)
            o['red'].t[:fused * 2 * C_] = 0.0
            lb.dz_out, lb.red_out, lb.red_nslot = o['dz'].ptr(), o['red'].ptr(), fused
        return (lf if entry.startswith('fwd') else lb), o

    def tuned_collect(self, o, n_max, entry, fused=0):
        """The outputs of `entry` as host arrays, after the written / not written checks."""
        d = self.d
        n, K, C_ = d['n'], d['K'], d['C']
        out = {}
        if 'kcnt' in o:
            counters_ok(o['kcnt'], entry)
            assert o['kpart'].guards_ok(), entry + ': written outside the scratch tiles'
        for s, M in enumerate(d['M']):
            if not M:
                continue
            if entry.startswith('fwd'):
                out['y%d' % s] = written(o['y'][s], rows(n, n_max, M), 'y[%d]' % s)[:n]
            else:
                kr = K + 1 if d['extra'][s] else K
                out['dw%d' % s] = written(o['dw'][s], rows(kr, K + 1, M), 'dW[%d]' % s)[:kr]
                out['db%d' % s] = written(o['db'][s], np.ones(M, bool), 'db[%d]' % s)
        if entry.startswith('bwd'):
            if fused:
                assert o['dx'] is None
                out['dz'] = written(o['dz'], rows(n, n_max, K), 'dz')[:n]
                out['red'] = written(o['red'], rows(fused, _hip.BN_SLOTS, 2 * C_), 'red')[:fused].sum(0)
            else:
                out['dx'] = written(o['dx'], rows(n, n_max, K), 'dx')[:n]
        return out

    def tuned_compare(self, out, what):
        d, ref = self.d, self.ref
        for s, M in enumerate(d['M']):
            if M and 'y%d' % s in out:
                close(out['y%d' % s], ref['y'][s][0], fwd_lim(*ref['y'][s]), '%s y[%d]' % (what, s))
            if M and 'dw%d' % s in out:
                close(out['dw%d' % s], ref['dw'][s][0], grad_lim(*ref['dw'][s]), '%s dW[%d]' % (what, s))
                close(out['db%d' % s], ref['db'][s][0], grad_lim(*ref['db'][s]), '%s db[%d]' % (what, s))
        if 'dx' in out:
            close(out['dx'], ref['dx'][0], grad_lim(*ref['dx']), what + ' dx')
        if 'dz' in out:
            fz = self.fz
            on, share = X.dz_resolve(out['dz'], fz)
            assert share <= 1e-3, '%s: %.3g of dz within %g of a ReLU edge' % (what, share, X.NEAR)
            close(out['dz'], on * fz['dx'], grad_lim(None, on * fz['dxb']), what + ' dz')
            red, bound = X.fused_red(fz, on, d['C'])
            close(out['red'], red, grad_lim(red, bound), what + ' reductions')


def launch_lin(lins, entry, n_max=None, k_max=None, fused=0, scratch=True):
    """One launch of `entry` over the records of `lins` on fresh buffers (n_max / k_max: the maxima unless given)."""
    lib = _hip.load()
    n_max = max(l.d['n'] for l in lins) if n_max is None else n_max
    k_max = max(l.d['K'] for l in lins) if k_max is None else k_max
    recs = [l.tuned_records(n_max, entry, fused if l.d['mode'] == 'batch' else 0, scratch) for l in lins]
    tab = _hip.to_device_table([r[0] for r in recs], DEV)
    if entry == 'fwd':
        rc = lib.mpnn_lin_fwd(tab.data_ptr(), len(lins), n_max, stream())
    elif entry == 'fwd_ks':
        rc = lib.mpnn_lin_fwd_ks(tab.data_ptr(), len(lins), n_max, k_max, stream())
    else:
        rc = (lib.mpnn_lin_bwd_rs if entry == 'bwd_rs' else lib.mpnn_lin_bwd)(tab.data_ptr(), len(lins), n_max, k_max, stream())
    _hip.check(rc, 'lin ' + entry)
    torch.cuda.synchronize()
    return [l.tuned_collect(r[1], n_max, entry, fused if l.d['mode'] == 'batch' else 0) for l, r in zip(lins, recs)]


def twice(lins, entry, what, **kw):
    """Two launches on fresh buffers: the same bits (but for the float64 atomic reductions), every record compared."""
    a, b = launch_lin(lins, entry, **kw), launch_lin(lins, entry, **kw)
    for l, u, v in zip(lins, a, b):
        w = '%s n%d-hw%d-c%d' % ((what,) + l.case[:3])
        same_bits({k: u[k] for k in u if k != 'red'}, v, w)
        l.tuned_compare(u, w)
        if 'red' in v:
            l.tuned_compare({k: v[k] for k in ('dz', 'red')}, w + ' again')
    return a


def check_tuned_lin(lins, **kw):
    """The four entry points over `lins`; returns entry -> the unfused outputs of every record."""
    res = {}
    any_batch = any(l.d['mode'] == 'batch' for l in lins)
    for entry in ENTRIES:
        res[entry] = twice(lins, entry, entry, **kw)
        if entry.startswith('bwd') and any_batch:
            for nslot in (1, 8, 16):
                fu = twice(lins, entry, '%s fused/%d' % (entry, nslot), fused=nslot, **kw)
                for l, f, u in zip(lins, fu, res[entry]):          # the same contraction: dW, db bit for bit
                    same_bits({k: f[k] for k in f if k[:2] in ('dw', 'db')}, u, entry + ': fused against unfused')
    return res


LIN_ID = lambda c: 'n%d-hw%d-c%d-%s-m%d-%d%s' % c


def tuned_lin(case):
    l = TunedLin(case)
    l.case = case
    return l


@pytest.mark.parametrize('case', X.TUNED_LIN_CASES, ids=LIN_ID)
def test_lin_tuned(case):
    """mpnn_lin_fwd, mpnn_lin_fwd_ks (k_max = K; scratch where the engine gives it), mpnn_lin_bwd and mpnn_lin_bwd_rs
    (scratch always) with dx, and for the batch-statistics cases fused with red_nslot = 1, 8, 16."""
    check_tuned_lin([tuned_lin(case)])


def test_lin_fwd_ks_without_scratch():
    """K = 784 without scratch: S = 1 inside the sliced kernel, whose grid still has three slices."""
    twice([tuned_lin(X.TUNED_LIN_CASES[4])], 'fwd_ks', 'fwd_ks bare', scratch=False)


def test_lin_tuned_table():
    """Four records of different n, K, modes and slice counts (S = 1, 1, 3, 2 under a grid of 4 x 3) in one table, one
    without a head and one without a router; n_max = 130, k_max = 784.  Every record equals, bit for bit, itself
    launched alone through the same entry point with the same n_max (the row split depends on it)."""
    lins = [tuned_lin(c) for c in X.TUNED_LIN_MULTI]
    res = check_tuned_lin(lins)
    for entry in ENTRIES:
        for l, t in zip(lins, res[entry]):
            alone = launch_lin([l], entry, n_max=130)[0]
            same_bits(alone, t, '%s: alone against the table' % entry)
            assert set(alone) == set(t)


# ---------------------------------------------------------------------------------------------------- exit tail
class TunedTail(Tail):
    """One record of mpnn_exit_tail_fwd / _bwd.  The record is the any-width one (bn_save is [4 R] with R2 == R); the
    tuned backward does not write dh2."""
    DH2 = False

    def __init__(self, name, clear=None):
        super().__init__(name, clear, X.TUNED_TAIL_CASES if name in X.TUNED_TAIL_CASES else None)
        d = self.d
        assert d['R'] == d['R2'] <= 16 and d['S'] <= 4 and (not d['head'] or d['nc'] <= 16)


def run_tuned_tail(tails, n_max=None):
    """mpnn_exit_tail_fwd over the records, then (batch-statistics mode) mpnn_exit_tail_bwd on the forward's own h2 and
    bn_save."""
    lib = _hip.load()
    n_max = max(t.d['n'] for t in tails) if n_max is None else n_max
    recs = [t.records(n_max) for t in tails]
    tf = _hip.to_device_table([r[0] for r in recs], DEV)
    _hip.check(lib.mpnn_exit_tail_fwd(tf.data_ptr(), len(tails), n_max, stream()), 'exit_tail_fwd')
    torch.cuda.synchronize()
    if all(t.d['mode'] == 'batch' for t in tails):
        for r in recs:
            r[1].f = r[0]
        tb = _hip.to_device_table([r[1] for r in recs], DEV)
        _hip.check(lib.mpnn_exit_tail_bwd(tb.data_ptr(), len(tails), n_max, stream()), 'exit_tail_bwd')
        torch.cuda.synchronize()
    return [t.collect(r[2], n_max) for t, r in zip(tails, recs)]


def check_tuned_tail(tails):
    first, again = run_tuned_tail(tails), run_tuned_tail(tails)
    for t, a, b in zip(tails, first, again):
        same_bits(a, b, t.d['name'])
        t.compare(a)
    return first


@pytest.mark.parametrize('name', list(X.TUNED_TAIL_CASES) + ['ship129', 'ship300', 'rows1100', 'headonly'])
def test_exit_tail_tuned(name):
    """mpnn_exit_tail_fwd, then mpnn_exit_tail_bwd on its h2 and bn_save.  Moving-average mode: the forward alone, the
    averages bit-unchanged (Tail.compare)."""
    out = check_tuned_tail([TunedTail(name)])[0]
    if name == 't_one':                                    # zero variance: the input gradient is exactly zero
        assert not out['dh1'].any()


def test_exit_tail_tuned_table():
    """Four records in one table with n_max = 129: the call launches the LDS-resident kernels (n = 37, 70, 70) and the
    any-size ones (n = 129).  Two records carry accumulators to clear and a schedule row to copy (exactly those ranges
    are written: Tail.collect); one has no router, one no head.  Every record equals itself launched alone with its own
    n_max bit for bit."""
    make = lambda: [TunedTail('t_r5', clear=(37, 5)), TunedTail('ship129', clear=(21, 3)), TunedTail('t_head'), TunedTail('t_router')]
    tails = make()
    assert max(t.d['n'] for t in tails) == 129
    outs = check_tuned_tail(tails)
    for t, o in zip(make(), outs):
        alone = run_tuned_tail([t])[0]
        same_bits(alone, o, t.d['name'] + ': alone against the table')
        assert set(alone) == set(o)


# ---------------------------------------------------------------------------------------------------- evaluation exit
EV_BITS = ('r', 'c_err', 'd_cor', 'cls', 'conf', 'p', 'counts')


def make_tuned_ev(name, count=None):
    seed, N, cnt, HW, C_, nc, R, S, dyn, head, router, lists = X.TUNED_EV_CASES[name]
    ex = Exit(seed, N=N, count=cnt if count is None else count, C_=C_, nc=nc, R=R, R2=R, S=S, HW=HW, dyn=dyn, head=head,
              router=router, eps=(1e-6, 1e-3))
    return ex, lists


@pytest.mark.parametrize('name', sorted(X.TUNED_EV_CASES))
def test_exit_ev_tuned(name):
    """mpnn_exit_ev (mpnn_exit_ev_check first: launch_table) on the record's own list, an empty list and a full one: r
    against float64 on the listed images and untouched elsewhere, the children's counts exact and their lists the
    arg-max sinks' images, the head as check_ev / check_label_free hold it.  Two launches: the same bits, the same
    lists as sets."""
    N = X.TUNED_EV_CASES[name][1]
    for count in (None, 0, N):
        ex, lists = make_tuned_ev(name, count)
        what = '%s/%s' % (name, 'own' if count is None else count)
        a, b = ex.launch(False, labels=True, lists=lists), ex.launch(False, labels=True, lists=lists)
        check_ev(ex, lists, a, what)
        same_bits({k: a[k] for k in EV_BITS}, {k: b[k] for k in EV_BITS}, what)
        assert np.array_equal(np.sort(a['lists'], 1), np.sort(b['lists'], 1))
        if ex.head and ex.count:
            check_label_free(ex, gen=False)


def test_exit_ev_tuned_table():
    """The five records in ONE table (capacities 70 and 37): every record's outputs as above, twice."""
    made = [make_tuned_ev(k) for k in sorted(X.TUNED_EV_CASES)]
    lists = (1, 2)                                         # (one choice for the table: sinks 1 and 2 have a child)
    first = launch_table([m[0] for m in made], False, labels=True, lists=lists)
    again = launch_table([m[0] for m in made], False, labels=True, lists=lists)
    for k, (ex, _), a, b in zip(sorted(X.TUNED_EV_CASES), made, first, again):
        check_ev(ex, tuple(i for i in lists if i < ex.S) if ex.router else (), a, 'table/' + k)
        same_bits({q: a[q] for q in EV_BITS}, {q: b[q] for q in EV_BITS}, 'table/' + k)
        assert np.array_equal(np.sort(a['lists'], 1), np.sort(b['lists'], 1))
