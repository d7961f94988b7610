"""GPU: the ActivityError terms of the exit backward kernels, each entry point alone through the C ABI against the float64
reference of tests/activity_error_ref.py, on the inputs of the tables in tests/exit_ref.py and with the machinery of
tests/test_exit_tuned_kernels.py and tests/test_exit_gen_kernels.py (NaN-filled guarded outputs, every launch twice with the
same bits):

  mpnn_lin_bwd / mpnn_lin_bwd_rs   act_alpha / act_w on five of exit_ref.TUNED_LIN_CASES: raw (identity) activations; the
                                   k_cpt row inside the last feature block (its dW row is the launch's without the layer, bit
                                   for bit); a batch of one; three row groups, the last ragged; two supers -- with dx, and the
                                   batch-statistics ones fused (dx == NULL: dz_out, red_out) under exit_ref.dz_resolve's rule;
                                   TUNED_LIN_MULTI with the layer on records 0 and 2: the other two equal, bit for bit, the
                                   table launched with the fields zeroed and act_w NULL
  mpnn_lin_bwd_gen                 four of exit_ref.LIN_CASES
  mpnn_exit_tail_bwd               act_z / act_p on five of exit_ref.TUNED_TAIL_CASES x the three loss kinds x the (α_z, α_p)
  mpnn_exit_tail_bwd_gen           combinations of activity_error_ref.ALPHAS (a head without Softmax has no α_p); any-width:
                                   20 classes at n = 129, 100 classes, and n = 37.  Everything but dz -- the router's
                                   outputs, the forward's -- has the bits of the launch with both α zero, and that launch is
                                   held to the references those files hold it to

Limits: the constants of those two files, per element, with `bound` extended by the bound of the layer's own term:
  4e-6 * bound + 1e-6     dx, the fused dz and the fused reductions
  2e-5 * bound + 1e-9     dz of the head
dW and db do not see the layer: they keep their references and limits.  tests/test_activity_error_ref_cpu.py shows on the CPU
that numpy float32 meets every limit and that every case's α moves the result far beyond it.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hiputil import dev
import activity_error_ref as R
import exit_ref as X
from test_exit_gen_kernels import Lin, Tail, check_lin, check_tail, close, run_lin, run_tail, same_bits
from test_exit_tuned_kernels import TunedLin, TunedTail, check_tuned_tail, launch_lin, run_tuned_tail, twice


# ---------------------------------------------------------------------------------------------------- affine maps
class _ActLin:
    """The layer on a record of the affine-map backward: act_alpha = α, act_w = weights drawn for the case."""

    def set_activity(self, α, seed):
        self.α = α
        self.w = R.act_w(self.d['n'], seed)
        self.w_d = dev(self.w) if α else None
        if α:
            self.ref = R.lin_ref_with(self.d, self.ref, self.w, α)              # (a new dict: the shared reference stays)
            if self.d['mode'] == 'batch':
                self.fz = X.lin_fused(self.d, self.ref)
        return self

    def stamp(self, lb):
        if self.α:
            lb.act_alpha, lb.act_w = self.α, self.w_d.data_ptr()


class ActTunedLin(_ActLin, TunedLin):
    def tuned_records(self, n_max, entry, fused=0, scratch=True):
        rec, o = super().tuned_records(n_max, entry, fused, scratch)
        if entry.startswith('bwd'):
            self.stamp(rec)
        return rec, o


class ActGenLin(_ActLin, Lin):
    def records(self, n_max, with_dx):
        lf, lb, o = super().records(n_max, with_dx)
        self.stamp(lb)
        return lf, lb, o


def tuned_lin(k, α, cls=ActTunedLin, table=X.TUNED_LIN_CASES):
    l = cls(table[k])
    l.case = table[k]
    return l.set_activity(α, k)


LIN_ID = lambda k: 'n%d-hw%d-c%d-%s' % X.TUNED_LIN_CASES[k][:4]


@pytest.mark.parametrize('k', sorted(R.TUNED_LIN), ids=LIN_ID)
def test_lin_bwd_tuned_with_the_map_term(k):
    """mpnn_lin_bwd and mpnn_lin_bwd_rs with dx and (batch statistics) fused: dx, dz and the reductions against the reference
    with the term; dW and db -- the k_cpt row of the router's included -- bit for bit those of the same launch without the
    layer."""
    with_α, plain = tuned_lin(k, R.TUNED_LIN[k]), tuned_lin(k, 0.0)
    for entry in ('bwd', 'bwd_rs'):
        a = twice([with_α], entry, entry + ' activity')[0]
        b = launch_lin([plain], entry)[0]
        same_bits({q: a[q] for q in a if q != 'dx'}, b, entry + ': dW / db with the layer against without')
        assert not np.array_equal(a['dx'], b['dx'])
        if with_α.d['mode'] == 'batch':
            f = twice([with_α], entry, entry + ' activity fused/8', fused=8)[0]
            same_bits({q: f[q] for q in f if q[:2] in ('dw', 'db')}, b, entry + ': fused dW / db')


def test_lin_bwd_tuned_table_with_the_layer_on_two_records():
    """TUNED_LIN_MULTI, α on records 0 and 2: every record against its reference; records 1 and 3 equal, bit for bit, the
    same table launched with the new fields zeroed and act_w NULL (a table of TunedLin records, which never set them)."""
    ks = [X.TUNED_LIN_CASES.index(c) for c in X.TUNED_LIN_MULTI]
    lins = [tuned_lin(k, α) for k, α in zip(ks, R.TUNED_LIN_MULTI_α)]
    bare = [tuned_lin(k, 0.0) for k in ks]
    assert [bool(l.α) for l in lins] == [True, False, True, False]
    for entry in ('bwd', 'bwd_rs'):
        a = twice(lins, entry, entry + ' activity table')
        b = launch_lin(bare, entry)
        for i in (1, 3):
            same_bits(a[i], b[i], '%s: record %d without the layer beside records with it' % (entry, i))
        for i in (0, 2):
            assert not np.array_equal(a[i]['dx'], b[i]['dx'])
            same_bits({q: a[i][q] for q in a[i] if q != 'dx'}, b[i], '%s: dW / db of record %d' % (entry, i))
        twice(lins, entry, entry + ' activity table fused/8', fused=8)


@pytest.mark.parametrize('k', sorted(R.GEN_LIN), ids=lambda k: 'n%d-hw%d-c%d-%s' % X.LIN_CASES[k][:4])
def test_lin_bwd_gen_with_the_map_term(k):
    """mpnn_lin_bwd_gen (mpnn_exit_gen_check first, as every launch of the any-width forms): dx with the term; y, dW, db
    bit for bit those of the launch without the layer."""
    l = tuned_lin(k, R.GEN_LIN[k], ActGenLin, X.LIN_CASES)
    check_lin([l])
    a, b = run_lin([l], True)[0], run_lin([Lin(X.LIN_CASES[k])], True)[0]
    same_bits({q: a[q] for q in a if q != 'dx'}, b, 'any-width: y / dW / db with the layer against without')
    assert not np.array_equal(a['dx'], b['dx'])


# ---------------------------------------------------------------------------------------------------- exit tail
class _ActTail:
    """A tail record with loss kind `form` and the layer's act_z / act_p."""

    def set_activity(self, form, α_z, α_p):
        self.form, self.α_z, self.α_p = form, α_z, α_p
        self.dz_ref = R.tail_dz(self.d, form, α_z, α_p) if self.d['head'] else None
        return self

    def records(self, n_max):
        tf, tb, o = super().records(n_max)
        tf.loss, tb.act_z, tb.act_p = R.LOSS[self.form], self.α_z, self.α_p
        return tf, tb, o

    def compare(self, out):
        if self.form == 'ce' and not (self.α_z or self.α_p):
            return super().compare(out)                    # (the record those files test: every output against exit_ref)
        if self.d['head']:
            close(out['dz'], self.dz_ref[0], R.dz_lim(self.dz_ref[1]), '%s %s (%g, %g) dz' % (self.d['name'], self.form, self.α_z, self.α_p))


class ActTunedTail(_ActTail, TunedTail):
    pass


class ActGenTail(_ActTail, Tail):
    def __init__(self, name, clear=None):
        Tail.__init__(self, name, clear, R.tail_table(name))


def check_tail_case(cls, check, run, name, form):
    base = check([cls(name).set_activity(form, 0.0, 0.0)])[0]
    for α_z, α_p in R.ALPHAS[form]:
        out = check([cls(name).set_activity(form, α_z, α_p)])[0]
        # the router's outputs, the forward's: the bits of the launch without α
        same_bits({k: out[k] for k in out if k != 'dz'}, base, '%s %s: outputs beside dz' % (name, form))
        assert not np.array_equal(out['dz'], base['dz'])
    # (0, 0): the bits of a record that never heard of the fields
    t = cls(name).set_activity(form, 0.0, 0.0)
    t.records = lambda n_max, t=t: _without_fields(t, n_max)
    same_bits(run([t])[0], base, '%s %s: (0, 0) against a record without the fields' % (name, form))


def _without_fields(t, n_max):
    tf, tb, o = super(_ActTail, t).records(n_max)
    tf.loss = R.LOSS[t.form]
    assert tb.act_z == 0 and tb.act_p == 0
    return tf, tb, o


@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('name', R.TUNED_TAIL)
def test_exit_tail_bwd_tuned_with_the_head_terms(name, form):
    check_tail_case(ActTunedTail, check_tuned_tail, run_tuned_tail, name, form)


@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('name', R.GEN_TAIL)
def test_exit_tail_bwd_gen_with_the_head_terms(name, form):
    check_tail_case(ActGenTail, check_tail, run_tail, name, form)
