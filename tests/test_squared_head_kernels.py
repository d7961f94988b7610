"""GPU: the SquaredError heads of the exit kernels (the records' `loss`: MPNN_LOSS_SQ on the softmax, MPNN_LOSS_SQ_LIN on
the LinTrans output), each entry point alone through the C ABI against tests/squared_error_ref.py in float64, with the
machinery of tests/test_exit_gen_kernels.py and tests/test_predict_kernels.py:

  mpnn_exit_tail_fwd / _bwd            squared_error_ref.TAIL_SHAPES['tuned'], ties, rows below -1, a mixed table
  mpnn_exit_tail_fwd_gen / _bwd_gen    squared_error_ref.TAIL_SHAPES['gen'], ties, rows below -1, a mixed table
  mpnn_exit_ev / mpnn_exit_ev_gen      labelled and label-free, with and without a sample list, with p_cls, ties, rows below
                                       -1; mpnn_exit_ev_check refuses a loss it does not know

Every output lives in a NaN-filled guarded buffer (written exactly where it must be), every case runs twice and must
give the same bits.  Limits, element by element -- the project's constants, none widened:
  c_err   2e-5 * (1 + |ref|)
  dz      2e-5 * bound + 1e-9, bound = the sum of the absolute values of the element's own terms in the float64 reference
          (squared_error_ref.head_bwd)
  d_cor, cls   exact on EVERY row: the inputs keep a top-two gap of 0.5 in z and in y (asserted above 1e-4 in x and y on the
          CPU), and the tie rows tie exactly
  conf, p_cls  2e-4 * (1 + max |ref|), as tests/test_predict_kernels.py: check_label_free holds them
The same reference in numpy float32 stays below 0.05 of every limit on these inputs (tests/test_squared_error_ref_cpu.py
asserts half).  The mixed tables hold a cross-entropy record with a router beside the squared ones: it and the router
outputs are held to tests/exit_ref.py, unchanged.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lib import _hip
from hiputil import dev
import squared_error_ref as R
from test_exit_gen_kernels import Tail, check_tail, close, same_bits
from test_exit_tuned_kernels import TunedTail, check_tuned_tail
from test_predict_kernels import Exit

CHECK = {'tuned': check_tuned_tail, 'gen': check_tail}


class SqTail(Tail):
    """One head-only record of the exit-tail launches with a SquaredError head on the inputs (z, y, w_cerr) of a case."""

    def __init__(self, cid, family, form, inputs):
        z, y, w = inputs
        name = 'squared/' + cid
        super().__init__(name, None, {name: dict(n=len(z), nc=z.shape[1], R=0, R2=0, S=0, stride=4, seed=0, router=False)})
        self.form = form
        self.d.update(z=z, y=y, w_cerr=w)
        self.t = {k: dev(self.d[k]) for k in ('z', 'y', 'w_cerr')}
        self.fref, self.dzref = R.head_fwd(z, y, form), R.head_bwd(z, y, w, form)

    def records(self, n_max):
        tf, tb, o = super().records(n_max)
        tf.loss = R.LOSS[self.form]
        tf.eps_ce = float('nan')                           # (not read by these heads)
        return tf, tb, o

    def compare(self, out):
        name, f = self.d['name'], self.fref
        close(out['c_err'], f['c_err'], R.c_err_lim(f['c_err']), name + ' c_err')
        assert np.array_equal(out['d_cor'], f['d_cor']), name + ' d_cor'
        close(out['dz'], self.dzref[0], R.dz_lim(*self.dzref), name + ' dz')


TAIL = R.tail_cases()


@pytest.mark.parametrize('case', TAIL, ids=[c[0] for c in TAIL])
def test_squared_exit_tail(case):
    """Forward, then backward, of one record (the any-width forms after mpnn_exit_gen_check, as every launch of theirs)."""
    cid, family, form, inputs = case
    out = CHECK[family]([SqTail(cid, family, form, inputs)])[0]
    if cid.endswith('ties') or cid.endswith('sentinel'):
        assert 0 < out['d_cor'].sum() < len(out['d_cor'])             # (both answers occur)


@pytest.mark.parametrize('family', ['tuned', 'gen'])
def test_mixed_table(family):
    """Three records with losses 0, 1 and 2 side by side, the cross-entropy one with a router: it and the router outputs
    against tests/exit_ref.py as they always were, the squared ones against their own reference."""
    plain = TunedTail('t_r5') if family == 'tuned' else Tail('table0')
    assert plain.d['router'] and plain.d['head']
    sq, lin = (SqTail('table/' + cid, fam, form, inputs) for cid, fam, form, inputs in R.mixed_cases(family))
    tails = [sq, plain, lin]
    assert max(t.d['n'] for t in tails) == R.MIXED_N
    recs = [t.records(R.MIXED_N)[0] for t in tails]
    assert [r.loss for r in recs] == [_hip.LOSS_SQ, _hip.LOSS_CE, _hip.LOSS_SQ_LIN]
    outs = CHECK[family](tails)
    # every record equals itself launched alone, bit for bit
    for t, o in zip(tails, outs):
        same_bits(CHECK[family]([t])[0], o, t.d['name'] + ': alone against the table')


# ---------------------------------------------------------------------------------------------------- evaluation heads
def make_exit(d, form, listed):
    N = d['N']
    ex = Exit(d['seed'], N=N, count=max(1, 3 * N // 4) if listed else N, C_=d['C_'], nc=d['nc'], R=16, R2=16, S=2, HW=d['HW'],
              wh=d['wh'], bh=d['bh'], router=False)
    for k in ('x', 'g', 'be', 'ma', 'va'):                 # (the inputs the CPU test judged)
        assert np.array_equal(getattr(ex, k), d[k]), k
    ex.y = d['y']
    ex.t['y'] = dev(d['y'])
    ex.e.loss = R.LOSS[form]
    ex.e.eps_ce = float('nan')
    if not listed:
        ex.e.idx, ex.e.cnt, ex.idx = None, None, np.arange(N, dtype=np.int32)
    return ex


def check_squared_ev(d, form, gen, listed):
    ex = make_exit(d, form, listed)
    idx, nc = ex.idx, ex.nc
    rest = np.setdiff1d(np.arange(ex.N), idx)
    f = R.head_fwd(R.ev_logits(d), d['y'], form)
    ref = f['x']
    free = ex.launch(gen, labels=False)
    assert np.array_equal(free['cls'][idx], f['cls'][idx])
    bound = R.OUT_TOL * (1 + np.abs(ref[idx]).max())
    assert np.abs(free['conf'][idx] - ref[idx, f['cls'][idx]]).max() <= bound
    assert np.abs(free['p'][idx][:, :nc] - ref[idx]).max() <= bound
    # conf is the output of cls; nothing outside the list, nothing in the rows' padding, c_err / d_cor untouched
    assert np.array_equal(free['conf'][idx], free['p'][idx, free['cls'][idx]])
    assert (free['cls'][rest] == -1).all() and np.isnan(free['conf'][rest]).all() and np.isnan(free['p'][rest]).all()
    assert np.isnan(free['p'][:, nc:]).all() and np.isnan(free['c_err']).all() and np.isnan(free['d_cor']).all()
    # the labelled launch of the same record: the same class, and d_cor is its comparison with the label
    lab = ex.launch(gen, labels=True)
    assert np.array_equal(lab['cls'], free['cls']) and np.array_equal(lab['conf'][idx], free['conf'][idx])
    assert np.array_equal(lab['p'][idx][:, :nc], free['p'][idx][:, :nc])
    assert np.array_equal(lab['d_cor'][idx], (lab['cls'][idx] == d['y'][idx].argmax(1)).astype(np.float32))
    assert np.array_equal(lab['d_cor'][idx], f['d_cor'][idx])
    close(lab['c_err'][idx], f['c_err'][idx], R.c_err_lim(f['c_err'][idx]), 'c_err')
    assert np.isnan(lab['c_err'][rest]).all() and np.isnan(lab['d_cor'][rest]).all()
    same_bits(lab, ex.launch(gen, labels=True), 'evaluation head')
    # without p_cls: the same class and output
    bare = ex.launch(gen, labels=False, probs=False)
    assert np.array_equal(bare['cls'], free['cls']) and np.array_equal(bare['conf'][idx], free['conf'][idx]) and np.isnan(bare['p']).all()
    return free, lab


@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('family,nc', R.ev_cases())
def test_squared_exit_ev(family, nc, form):
    """mpnn_exit_ev (tuned) / mpnn_exit_ev_gen: 1, 64 and 65 images, every image or a list of three quarters, one-hot and
    real-valued targets."""
    for N in R.EV_N:
        for target in R.TARGETS:
            d = R.ev_input(family, nc, N, 'plain', target)
            for listed in (False, True):
                free, _ = check_squared_ev(d, form, family == 'gen', listed)
    if form == 'lin':
        assert (free['conf'] < 0).any() or (free['p'] < 0).any()       # raw outputs, not probabilities


@pytest.mark.parametrize('family', ['tuned', 'gen'])
def test_linear_head_below_the_probability_sentinel(family):
    """Every output below -1, three classes: thirteen of a sample's sixteen threads own no class and must not win."""
    d = R.ev_input(family, 3, 65, 'sentinel')
    free, lab = check_squared_ev(d, 'lin', family == 'gen', listed=False)
    assert free['conf'].max() < -2 and 0 < lab['d_cor'].sum() < 65 and len(set(free['cls'].tolist())) == 3


@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('family', ['tuned', 'gen'])
def test_evaluation_ties_take_the_first_index(family, form):
    d = R.ev_input(family, R.TIE_CLS[family], 65, 'ties')
    pz, py = R.TIES[family][0]
    free, lab = check_squared_ev(d, form, family == 'gen', listed=True)
    ex_idx = np.flatnonzero(free['cls'] >= 0)
    assert (free['cls'][ex_idx] == pz[0]).all() and np.array_equal(free['p'][ex_idx, pz[0]], free['p'][ex_idx, pz[1]])
    assert (lab['d_cor'][ex_idx] == float(pz[0] == py[0])).all()


def test_exit_ev_check_refuses_an_unknown_loss():
    lib = _hip.load()
    ex = make_exit(R.ev_input('tuned', 16, 1), 'sq', listed=True)
    ex.prepare(labels=True, probs=True, lists=())
    for loss, want in ((0, 0), (1, 0), (2, 0), (3, _hip.E_SHAPE), (-1, _hip.E_SHAPE)):
        ex.e.loss = loss
        assert lib.mpnn_exit_ev_check(C.byref(ex.e)) == want, loss
