"""GPU: the exit kernels on the inputs of a TRAINED net (csrc/lin.hip, exit_tail.hip, exit_gen.hip, exit_ev.hip), each
entry point alone through the C ABI against the explicit float64 reference of tests/exit_ref.py.

What the older files never vary is the values: tests/test_exit_kernels.py, test_exit_gen_kernels.py and
test_exit_tuned_kernels.py draw a net at initialisation (logits 2 N(0, 1), hidden units N(0, 1), scales and variances in
[0.5, 1.5]).  Here the same records run in the regimes of exit_ref.REGIMES, on the smallest case that reaches each code
path (exit_ref.TUNED_REGIME_RUNS / GEN_REGIME_RUNS / BOTH_REGIME_RUNS):

  head     confident   logits 10 to 40 apart, rows confidently wrong, a softmax output exactly 0 in fp32, two rows whose
                       top two logits tie bitwise (first index on both sides), w_cerr = 0 / 1e-8 / 1
           offset      the same with a common +-1e4 per row: the max-subtraction matters
  router   shifted     channel means in +-50, spreads from 1e-3 to 10
           pivot       row 0 six to a hundred standard deviations out -- the row the tuned kernels pivoted their one-pass
                       sums on before this file came
           dead        a constant channel, sigma far below sqrt(eps), gamma 1e-4 / 20 / negative, a dead unit, a unit
                       always on
           moving      v_avg in {0, 1e-8, 1e-3, 1, 1e4}, m_avg up to 30 sqrt(v) from the batch's mean
  lin      trained     channel scales and v_avg over four to eight decades, gamma of both signs, 70 % of the
                       pre-activations off, a channel off everywhere (its dW rows exactly 0.0) and one on everywhere

  mpnn_exit_tail_fwd / _bwd             the tuned kernels (bn_stats, router_fwd_big with fewer and more rows than
                                        threads), CE and the softmax SquaredError head
  mpnn_exit_tail_fwd_gen / _bwd_gen     the any-width kernels; ship300 and t_r8_1100 through BOTH families on one record,
                                        each against the reference, their mutual difference printed
  mpnn_exit_ev                          ev_c48, ev_hw1 in moving + confident, their own list and an empty one
  mpnn_lin_fwd / _fwd_ks / _bwd / _bwd_rs and mpnn_lin_fwd_gen / _bwd_gen      trained, batch and moving mode

Everything the older files hold stays held: NaN-filled guarded outputs written exactly where they must be, two launches
with the same bits (the float64-atomic fused reductions excepted, as there), every record after its check.  Beyond
`close`: c_err <= -log(eps_ce / nc) (1 + 1e-6); dz rows with w_cerr = 0 exactly 0; d_cor exact on the tie rows; dh1
exactly 0 in every channel where the reference's is (the constant channel, the dead unit); the moving averages bit-
unchanged in moving mode; the dead channel's dW rows exactly 0.0.

Limits.  The constants of tests/test_exit_gen_kernels.py.  For every compared quantity of every (case, regime) the
reference is also evaluated in numpy float32, as written and with the batch rows reversed (exit_ref.f32_errors).  Where
that error stays within 0.2 of the constant -- the rule tests/test_exit_ref_cpu.py asserts for the older draws -- the
constant holds unchanged.  Where it does not, the input is ill-conditioned for ANY fp32 evaluation and the limit is
max(constant, 5 x the float32 reference's worst error) (exit_ref.widened): computed from the reference at run time,
never read off a kernel.  tests/test_exit_ref_cpu.py prints the widened (case, regime, quantity) triples and asserts
that no statistic of a `pivot` case, and no statistic, c_err, dz or bias gradient of any case, is among them.  They are
(float32 reference / constant): h2, r and dw3 of every `shifted` and `pivot` case (h2 1.2 to 48, r 0.7 to 28, dw3 0.4 to
3.3; t_full/confident+shifted h2 396, r 177, dw3 165, and there also dh2, dw2 1.8, dg2 0.84, dg1 0.39, dh1 0.29) -- a
mean stored in fp32 is uncertain by 1e-4 of a spread that is 1e-3 of it, and w2, w3 carry that times 8 into sums whose
limit knows only their result --; dh2 0.3 to 0.4 at n = 1100; h2 of `dead` (0.6 to 13: rstd = 1000 behind sigma = 1e-5);
h2 and r of `moving` (0.6 to 6.3); of the affine maps dW (0.22 to 3.8) and in moving mode y (0.21 to 0.27): relu(bn(x))
is formed from gamma xhat + beta, which a trained beta makes cancel, and the sums' bounds know only the result.
The SECOND BatchNorm's statistics (bn_save's second half, m2, v2) are held to exit_ref.bn2_given of the kernel's OWN h2
(and its h2 to the reference): what h2 inherits from an ill-conditioned first layer is not charged to the statistics,
which therefore keep the unwidened limit in every regime.
ReLU masks: every seed keeps both BatchNorms' float64 pre-activations 1e-4 from zero.  Where the float32 reference's own
pre-activation error, times 5, exceeds that distance, the element is ambiguous (exit_ref.ambiguous; at most 0.1 % of a
case, asserted on the CPU): the device's mask may differ there and only there, and the reference then differentiates
through the device's masks.

The finding this file came with: bn_stats and router_fwd_big + stats_finish (csrc/exit_tail.hip) pivoted their one-pass
float sums on row 0, and lost up to log2(n) bits when that row was the extreme of its channel.  The pass now judges
itself and, where it lost more than five bits in any channel, runs once more around the mean it found (the comment above
bn_stats; exit_ref.pivoted_stats_f32 restates both forms).  A batch that never trips that -- every batch of the older
tests and of bench.py -- computes bit for bit what it did.

MEASURED on an MI355X.  The 32 tests take 2.9 s together (the slowest 0.1 s); every launch gave the same bits twice, and
no ReLU mask of a device differed from the reference's.
The parent's kernels (row-0 pivot) on the tuned `pivot` cases, worst error / limit, statistics limit unwidened:
  n = 1100 (t_r8_1100)   rstd1 1.88, v2 1.86, h2 1.16          n = 300 (ship300)   rstd1 1.04, h2 1.74, r 1.01, v2 0.65
  n = 300, R = 3         rstd1 0.61                             n = 128 (t_full)    rstd1 0.47, v1 0.42, v2 0.44, h2 1.85
  n = 37 (t_r5)          rstd1 0.30, v2 0.30
-- beyond the limit in router_fwd_big, a third to a half of it in bn_stats, where the draws at initialisation use 0.016;
the any-width kernels (float64 sums) 0.004 on the same records.  With the repeated pass the same five cases read bn_save
<= 0.0043 and v2 <= 0.020; worst over the file:
  tuned tail   bn_save (BatchNorm 1) 0.011, (BatchNorm 2) 0.0096, m1 0.013, v1 0.022, m2 0.003, v2 0.020, h2 0.20, r 0.061,
               c_err 0.013, dz 0.038, dw3 0.037, dbias3 0.007, dh1 0.044, dw2 0.039, dg2 0.037, dg1 0.037, db1 0.011
  any-width    bn_save 0.0036 / 0.002, m1 0.005, v1 0.008, m2 0.004, v2 0.021, h2 0.16, r 0.23, c_err 0.014, dz 0.038,
               dw3 0.098, dbias3 0.004, dh2 0.009, dh1 0.003, dw2 0.038, dg2 0.014, dg1 0.002
  tuned against any-width on one record, in limits: dz 0.014, c_err 0.012, h2 0.008, r 0.005, v2 0.003, every gradient <= 0.004
  squared head c_err 0.003, dz 0.005        evaluation  r 0.069, c_err 0.071
  affine maps  y 0.15, dW 0.067, db 0.015, dx 0.055, fused dz 0.027, fused reductions 0.006
What this file catches and the older files do not: four mutated libraries, arithmetic only, built aside and not kept, each
once through this file and once through tests/test_exit_tuned_kernels.py, test_exit_gen_kernels.py and test_exit_kernels.py
(96 tests), which passed under all four:
  1  head_softmax without the max-subtraction: caught -- t_full/offset+pivot, t_head/offset and the squared head on
     `offset` (c_err not finite); NOT by `confident` alone (exp(40) is finite)
  2  fmaxf(var, 0) dropped in stats_finish: NOT caught, by no file.  The pivot is a sample of the batch, so the variance
     is at least ~1/n of E[d^2] unless every d is 0 -- and then both terms are exactly 0: the clamp is unreachable below
     n ~ 1e6 (and a negative variance would repeat the pass).  It stays as a guard
  3  exit_ev.hip k1 = g1 / (sqrt(v1) + eps): caught -- both evaluation cases (r 1e8 limits off at v_avg = 0)
  4  the heads' dot summed over y_k > 0 only: caught in the squared head (both regimes); in the cross-entropy head the
     mutant is equivalent -- its g_k is 0 wherever y_k is
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lib import _hip
from hiputil import DEV, bn_dict, dev
import exit_ref as X
from test_exit_gen_kernels import (MODES, Tail, bn_lim, close, dz_lim, fwd_lim, grad_lim, run_lin, run_tail, same_bits, stat_lim)
from test_exit_tuned_kernels import EV_BITS, TunedLin, check_tuned_lin, check_tuned_tail, make_tuned_ev, run_tuned_tail
from test_predict_kernels import TOL
from test_squared_head_kernels import SqTail


# ---------------------------------------------------------------------------------------------------- limits
BN2 = ('bn_save2', 'm2', 'v2')


def tail_limits(d, f64, g64, on=None):
    """quantity -> (limit, the float32 reference's worst error / the existing limit, the floor the limit was raised to or
    0): exit_ref.widened of the project's constant and exit_ref.f32_errors, for every quantity a tail test compares (g64:
    tail_bwd's result for the masks `on`)."""
    out = {}
    for k, e in X.f32_errors(d, f64, g64, on).items():
        if g64 is not None and k in g64:
            lim = (dz_lim if k == 'dz' else grad_lim if k in ('dw3', 'dbias3') else bn_lim)(*g64[k])
        elif k in BN2:                                      # (of the kernel's own h2: the base limit is set at the comparison)
            lim = stat_lim(X.bn2_given(d, X.tail_fwd(d, np.float32)['h2'])[k])
        else:                                               # (m1, v1: the moving averages after the update)
            lim = stat_lim(f64['avg'][('m1', 'v1').index(k)] if k in ('m1', 'v1') else f64['bn_save'][:2 * d['R']] if k == 'bn_save1' else f64[k])
        out[k] = X.widened(lim, e)
    return out


_ref = {}


def reference(name, regime):
    """(inputs, forward, backward, limits, ambiguous mask elements) of one (case, regime), computed once."""
    if (name, regime) not in _ref:
        d = X.tail_inputs(name, table=X.tail_table(name), regime=regime)
        f = X.tail_fwd(d)
        g = X.tail_bwd(d, f.get('h2'), X.split_save(f['bn_save'], d['R'], d['R2']) if d['router'] else None) \
            if d['mode'] == 'batch' else None
        _ref[name, regime] = (d, f, g, tail_limits(d, f, g), X.ambiguous(d, f)[0] if d['router'] else None)
    return _ref[name, regime]


# ---------------------------------------------------------------------------------------------------- exit tail
class RegimeTail(Tail):
    """One record of the exit-tail launches on exit_ref.tail_inputs(name, regime=regime); tuned: the record goes to
    mpnn_exit_tail_fwd / _bwd, which never write dh2."""

    def __init__(self, name, regime, tuned):
        d, self.ref, self.gref, self.lims, self.amb = reference(name, regime)
        self.d, self.DH2, self.clear = d, not tuned, None
        self.what = '%s/%s/%s' % (name, regime, 'tuned' if tuned else 'gen')
        if tuned:
            assert d['R'] == d['R2'] <= 16 and d['S'] <= 4 and (not d['head'] or d['nc'] <= 16)
        self.t = {k: dev(d[k]) for k in ('z', 'y', 'w_cerr', 'h1', 'g1', 'b1', 'w2', 'bias2', 'g2', 'b2', 'w3', 'bias3') if k in d}

    def hold(self, k, got, want, L):
        close(got, want, L[k][0], '%s %s' % (self.what, k))

    def compare(self, out):
        d, ref, g, L = self.d, self.ref, self.gref, self.lims
        R, R2 = d['R'], d['R2']
        if d['head']:
            self.hold('c_err', out['c_err'], ref['c_err'], L)
            assert (out['c_err'] <= -np.log(np.float64(d['eps_ce']) / d['nc']) * (1 + 1e-6)).all(), self.what + ': c_err above its bound'
            sure, tie = ref['gap'] > 1e-4, ref['gap'] == 0
            assert sure.sum() >= 0.9 * d['n']
            assert np.array_equal(out['d_cor'][sure], ref['d_cor'][sure]), self.what + ' d_cor'
            assert np.array_equal(out['d_cor'][tie], ref['d_cor'][tie]), self.what + ': d_cor of a bitwise tie (first index)'
            assert np.isin(out['d_cor'], (0.0, 1.0)).all()
        if d['router']:
            self.hold('bn_save1', out['bn_save'][:2 * R], ref['bn_save'][:2 * R], L)      # (the statistics first: they say most)
            for k in ('h2', 'r'):
                self.hold(k, out[k], ref[k], L)
            own = X.bn2_given(d, out['h2'])                 # the second BatchNorm's statistics: of the kernel's own h2
            got = dict(out, bn_save2=out['bn_save'][2 * R:])
            for k, want in (('m1', ref['avg'][0]), ('v1', ref['avg'][1])) + tuple(own.items()):
                if d['mode'] == 'moving' and k in ('m1', 'v1', 'm2', 'v2'):
                    assert np.array_equal(out[k], d[k]), self.what + ': evaluation mode changed a moving average'
                else:
                    close(got[k], want, np.maximum(stat_lim(want), L[k][2]), '%s %s' % (self.what, k))
        if g is None:
            return
        if d['router']:
            on = X.masks(d, out['h2'], X.split_save(out['bn_save'], R, R2))
            diff = [a != (ref[k] > 0) for a, k in zip(on, ('pre1', 'pre2'))]
            if any(x.any() for x in diff):                  # only where fp32 cannot tell: then through the device's masks
                assert not any((x & ~a).any() for x, a in zip(diff, self.amb)), \
                    '%s, seed %d: a ReLU mask of the device differs from the reference\'s where it is unambiguous' % (self.what, d['seed'])
                print('%-40s %d mask elements resolved the device\'s way' % (self.what, sum(int(x.sum()) for x in diff)))
                g = X.tail_bwd(d, ref['h2'], X.split_save(ref['bn_save'], R, R2), on=on)
                L = tail_limits(d, ref, g, on)
            for k in ('dbias3', 'dw3', 'dh2', 'dh1', 'dg1', 'db1', 'dw2', 'dbias2', 'dg2', 'db2'):
                if k != 'dh2' or self.DH2:
                    self.hold(k, out[k].reshape(g[k][0].shape), g[k][0], L)
            zero = ~g['dh1'][0].any(0)
            assert not out['dh1'][:, zero].any(), self.what + ': dh1 of a channel whose gradient is exactly zero'
        if d['head']:
            self.hold('dz', out['dz'], g['dz'][0], L)
            assert not out['dz'][d['w_cerr'] == 0].any(), self.what + ': dz of a row with w_cerr = 0'


def check_regime_tail(name, regime, tuned):
    run = run_tuned_tail if tuned else run_tail
    t = RegimeTail(name, regime, tuned)
    a, b = run([t])[0], run([t])[0]
    same_bits(a, b, t.what)
    t.compare(a)
    return t, a


@pytest.mark.parametrize('name,regime', X.TUNED_REGIME_RUNS, ids=['%s-%s' % c for c in X.TUNED_REGIME_RUNS])
def test_tuned_tail_in_regime(name, regime):
    """mpnn_exit_tail_fwd, then mpnn_exit_tail_bwd on its h2 and bn_save (moving mode: the forward alone)."""
    t, out = check_regime_tail(name, regime, True)
    if name == 't_one':                                    # n = 1: every variance 0, the input gradient exactly zero
        assert not out['dh1'].any() and not t.ref['v1'].any()


@pytest.mark.parametrize('name,regime', X.GEN_REGIME_RUNS, ids=['%s-%s' % c for c in X.GEN_REGIME_RUNS])
def test_gen_tail_in_regime(name, regime):
    """mpnn_exit_tail_fwd_gen, then mpnn_exit_tail_bwd_gen (mpnn_exit_gen_check on the record first: run_tail)."""
    check_regime_tail(name, regime, False)


@pytest.mark.parametrize('name,regime', X.BOTH_REGIME_RUNS, ids=['%s-%s' % c for c in X.BOTH_REGIME_RUNS])
def test_both_families_on_one_record(name, regime):
    """The tuned and the any-width kernels on identical inputs: each meets the reference; their mutual difference, in
    units of the quantity's limit, is printed."""
    (t, a), (_, b) = check_regime_tail(name, regime, True), check_regime_tail(name, regime, False)
    for k in sorted(set(a) & set(b) & set(t.lims)):
        if np.isfinite(a[k]).all() and np.isfinite(b[k]).all():
            diff = np.abs(a[k].astype(np.float64) - b[k]).reshape(np.shape(t.lims[k][0]) or -1)
            print('%-40s tuned - any-width / limit %.3g' % ('%s/%s %s' % (name, regime, k), float((diff / t.lims[k][0]).max())))


@pytest.mark.parametrize('regime', ['confident', 'offset'])
def test_squared_head_in_regime(regime):
    """The softmax SquaredError head of mpnn_exit_tail_fwd / _bwd on t_head's logits: c_err, d_cor on EVERY row (the tie
    rows included) and dz at the limits of tests/test_squared_head_kernels.py, none widened."""
    d = X.tail_inputs('t_head', table=X.TUNED_TAIL_CASES, regime=regime)
    out = check_tuned_tail([SqTail('trained/' + regime, 'tuned', 'sq', (d['z'], d['y'], d['w_cerr']))])[0]
    assert not out['dz'][d['w_cerr'] == 0].any() and 0 < out['d_cor'].sum() < d['n']


# ---------------------------------------------------------------------------------------------------- evaluation exit
def ev_record(ex):
    """The evaluation exit `ex` as a tail record of exit_ref (moving mode), with the float64 activations."""
    P = ex.P
    d = dict(head=ex.head, router=True, mode='moving', n=ex.N, nc=ex.nc, R=ex.R, R2=ex.R2, S=ex.S, y=ex.y, eps_ce=1e-6,
             bn_eps=ex.eps[0], bn_eps2=ex.eps[1], bn_decay=0.0, bn_decay2=0.0, b1=P['be1'], b2=P['be2'])
    d.update({k: P[k] for k in ('g1', 'g2', 'w2', 'bias2', 'w3', 'bias3', 'm1', 'v1', 'm2', 'v2')})
    return d


def ev_maps(ex, dt):
    """(z, h1) of every image: relu(bn(x)) through the two affine maps in precision dt."""
    a = X.act(ex.x, 'moving', ex.g, ex.be, ex.ma, ex.va, dt=dt).reshape(ex.N, ex.K)
    z = X.lin_fwd(a, ex.wh, ex.bh, False, None, dt=dt)[0]
    return z, X.lin_fwd(a, ex.P['w1'], ex.P['b1'], ex.dyn, ex.kc, dt=dt)[0]


def trained_ev(name, count):
    """One TUNED_EV_CASES record in `confident` + `moving`: the head's map times 8 (logits tens apart), every other image
    labelled with its own arg-max (confidently right; the random labels of the rest are mostly confidently wrong), the
    router's moving statistics and scales by exit_ref's `moving` regime on the record's own float64 h1."""
    ex, lists = make_tuned_ev(name, count)
    rng = np.random.default_rng([X.TUNED_EV_CASES[name][0], 7])
    f = np.float32
    ex.wh, ex.bh = ex.wh * f(8), ex.bh * f(8)
    z, h1 = ev_maps(ex, np.float64)
    ex.y = ex.y.copy()
    ex.y[::2] = np.eye(ex.nc, dtype=f)[z.argmax(1)[::2]]
    d = ev_record(ex)
    d['z'], d['h1'] = z, h1
    X.REGIMES['moving'](d, rng)
    for k in ('g1', 'g2', 'm1', 'v1', 'm2', 'v2'):
        ex.P[k] = d[k]
        ex.t[k].copy_(dev(d[k]))
    for k, v in (('wh', ex.wh), ('bh', ex.bh), ('y', ex.y)):
        ex.t[k].copy_(dev(v))
    return ex, lists


@pytest.mark.parametrize('name', ['ev_c48', 'ev_hw1'])
def test_exit_ev_in_regime(name):
    """mpnn_exit_ev (mpnn_exit_ev_check first: launch_table) on the record's own list and on an empty one: r, c_err, d_cor
    and p_cls on the listed images, nothing anywhere else, the children's lists the arg-max sinks' images; twice, the
    same bits.  The float32 reference runs the whole chain (activation, both affine maps, the tail): no batch sums here,
    so one summation order."""
    for count in (None, 0):
        ex, lists = trained_ev(name, count)
        what = '%s/%s' % (name, 'own' if count is None else count)
        a, b = ex.launch(False, labels=True, lists=lists), ex.launch(False, labels=True, lists=lists)
        same_bits({k: a[k] for k in EV_BITS}, {k: b[k] for k in EV_BITS}, what)
        assert np.array_equal(np.sort(a['lists'], 1), np.sort(b['lists'], 1))
        idx, S, nc = ex.idx, ex.S, ex.nc
        rest = np.setdiff1d(np.arange(ex.N), idx)
        for k in ('r', 'c_err', 'd_cor', 'conf', 'p'):
            assert np.isnan(a[k][rest]).all(), '%s: %s outside the list' % (what, k)
        assert (a['cls'][rest] == -1).all() and np.isnan(a['r'][:, S:]).all() and np.isnan(a['p'][:, nc:]).all()
        if not len(idx):
            assert not a['counts'].any() and (a['lists'] == -1).all()
            continue
        ref, f32 = [], None
        for dt in (np.float64, np.float32):
            d = ev_record(ex)
            d['z'], d['h1'] = ev_maps(ex, dt)
            ref.append(X.tail_fwd(d, dt))
        f64, f32 = ref
        for k in ('r', 'c_err'):
            lim, ratio, _ = X.widened(stat_lim(f64[k][idx]), np.abs(f32[k][idx].astype(np.float64) - f64[k][idx]))
            print('%-40s float32 reference / existing limit %.3g' % ('%s %s' % (what, k), ratio))
            got = a[k][idx][:, :S] if k == 'r' else a[k][idx]
            assert np.isfinite(got).all()
            close(got, f64[k][idx], lim, '%s %s' % (what, k))
        assert (a['c_err'][idx] <= -np.log(1e-6 / nc) * (1 + 1e-6)).all()
        sure = f64['gap'][idx] > 1e-4
        assert sure.sum() >= 0.9 * len(idx) and np.array_equal(a['d_cor'][idx][sure], f64['d_cor'][idx][sure]), what + ' d_cor'
        assert 0 < a['d_cor'][idx].sum() < len(idx)                            # (confidently right and confidently wrong)
        assert np.abs(a['p'][idx][:, :nc] - f64['p'][idx]).max() <= TOL * (1 + f64['p'][idx].max()), what + ' p_cls'
        assert (f64['p'][idx].max(1) > 0.99).mean() > 0.5                      # (the regime: most outputs saturate)
        arg = np.argmax(a['r'][idx][:, :S], 1)
        for i in range(_hip.MAX_SINKS):
            want = np.sort(idx[arg == i]) if i in lists else np.zeros(0, np.int32)
            assert a['counts'][i] == len(want) and np.array_equal(np.sort(a['lists'][i][:len(want)]), want), '%s: list of sink %d' % (what, i)
            assert (a['lists'][i][len(want):] == -1).all()


# ---------------------------------------------------------------------------------------------------- affine maps
_lin_ref = {}


def lin_floors(d, ref, fz):
    """key -> (the float32 reference's worst error / the existing limit, the floor its limit is raised to or 0) for y, dW,
    db of both sets, dx, and the fused dz and reductions: exit_ref.widened on exit_ref.lin_ref in float32, as written and
    with the batch rows reversed.  relu(bn(x)) is formed from gamma xhat + beta, and the sums' bounds know only its
    result: where the two cancel, as a trained beta makes them, ANY fp32 evaluation loses that much of a."""
    n, C_ = d['n'], d['C']
    err = {}
    up = lambda k, a, b: err.__setitem__(k, np.maximum(err.get(k, 0), np.abs(np.asarray(a, np.float64) - b)))
    lims = {}
    for rev in (False, True):
        e = dict(d)
        if rev:
            e.update(x=d['x'][::-1], kc=d['kc'][::-1], dy=[None if v is None else v[::-1] for v in d['dy']])
        back = (lambda a: a[::-1]) if rev else (lambda a: a)
        r32 = X.lin_ref(e, np.float32)
        for s in range(2):
            if d['w'][s] is not None:
                for k, v, lim in (('y', back(r32['y'][s][0]), fwd_lim), ('dw', r32['dw'][s][0], grad_lim), ('db', r32['db'][s][0], grad_lim)):
                    up('%s%d' % (k, s), v, ref[k][s][0])
                    lims['%s%d' % (k, s)] = lim(*ref[k][s])
        up('dx', back(r32['dx'][0]), ref['dx'][0])
        lims['dx'] = grad_lim(*ref['dx'])
        if fz is not None:
            f32 = X.lin_fused(e, r32, np.float32)
            dz = back(f32['dz'][0])
            on = X.dz_resolve(dz, fz)[0]
            up('dz', dz, on * fz['dx'])
            lims['dz'] = grad_lim(None, on * fz['dxb'])
            red, bound = X.fused_red(fz, on, C_)
            up('red', X.fused_red(f32, f32['on'], C_)[0], red)
            lims['red'] = grad_lim(red, bound)
    return {k: X.widened(lims[k], err[k])[1:] for k in err}


class RegimeLin(TunedLin):
    """One record of the affine-map launches on exit_ref.lin_inputs(case, regime='trained'); every quantity held to
    max(the existing limit, its floor of lin_floors)."""

    def __init__(self, case):
        d = self.d = X.lin_inputs(case, regime='trained')
        if case not in _lin_ref:
            ref = X.lin_ref(d)
            fz = X.lin_fused(d, ref) if d['mode'] == 'batch' else None
            _lin_ref[case] = (ref, fz, lin_floors(d, ref, fz))
        self.ref, self.fz, self.floors = _lin_ref[case]
        self.case = case
        self.xd = dev(d['x'])
        self.bn, cnt = bn_dict(d['x'], d['gamma'], d['beta'], d['m_avg'], d['v_avg'])
        self.act = _hip.act(self.xd, d['C'], MODES[d['mode']], 0, self.bn, cnt)
        self.t = {k: [dev(v) for v in d[k]] for k in ('w', 'b', 'dy')}
        self.kc = dev(d['kc'])

    def tuned_compare(self, out, what=''):
        """TunedLin.tuned_compare (and, for the any-width launches, Lin.compare) with the floors."""
        d, ref = self.d, self.ref
        hold = lambda k, want, lim: close(out[k], want, np.maximum(lim, self.floors[k][1]), '%s %s %s' % (LIN_ID(self.case), what, k))
        for s, M in enumerate(d['M']):
            for k, q, lim in (('y%d' % s, 'y', fwd_lim), ('dw%d' % s, 'dw', grad_lim), ('db%d' % s, 'db', grad_lim)):
                if M and k in out:
                    hold(k, ref[q][s][0], lim(*ref[q][s]))
        if 'dx' in out:
            hold('dx', ref['dx'][0], grad_lim(*ref['dx']))
        if 'dz' in out:
            fz = self.fz
            on, share = X.dz_resolve(out['dz'], fz)
            assert share <= 1e-3, '%s: %.3g of dz within %g of a ReLU edge' % (what, share, X.NEAR)
            hold('dz', on * fz['dx'], grad_lim(None, on * fz['dxb']))
            red, bound = X.fused_red(fz, on, d['C'])
            hold('red', red, grad_lim(red, bound))

    compare = tuned_compare

    def dead_rows(self, out):
        """The dW rows of channel 0 -- off everywhere, a zero column of a -- are exactly 0.0."""
        for s, M in enumerate(self.d['M']):
            if M and 'dw%d' % s in out:
                rows = out['dw%d' % s][:self.d['K']][0::self.d['C']]
                assert rows.shape[0] == self.d['HW'] and not rows.any(), 'dW[%d] of the dead channel is not exactly zero' % s


# two tuned cases (K = 720: the K-slice scratch; K = 240: none) and an any-width one (K = 512, 100 classes), each in both modes
mode = lambda case, m: case[:3] + (m,) + case[4:]
TUNED_LINS = [mode(c, m) for c in (X.TUNED_LIN_CASES[1], X.TUNED_LIN_CASES[2]) for m in ('batch', 'moving')]
GEN_LINS = [mode(X.LIN_CASES[5], m) for m in ('batch', 'moving')]
LIN_ID = lambda c: 'n%d-hw%d-c%d-%s-m%d-%d%s' % c


@pytest.mark.parametrize('case', TUNED_LINS, ids=LIN_ID)
def test_tuned_lin_in_regime(case):
    """mpnn_lin_fwd, _fwd_ks, _bwd and _bwd_rs, and in batch mode the fused forms, as tests/test_exit_tuned_kernels.py
    runs them."""
    l = RegimeLin(case)
    for entry, outs in check_tuned_lin([l]).items():
        l.dead_rows(outs[0])


@pytest.mark.parametrize('case', GEN_LINS, ids=LIN_ID)
def test_gen_lin_in_regime(case):
    """mpnn_lin_fwd_gen / mpnn_lin_bwd_gen (mpnn_exit_gen_check first: run_lin), twice."""
    l = RegimeLin(case)
    a, b = run_lin([l], True)[0], run_lin([l], True)[0]
    same_bits(a, b, 'affine maps')
    l.compare(a)
    l.dead_rows(a)
