"""CPU: the explicit float64 reference of the any-width exit path (tests/exit_ref.py) against torch-CPU float64
autograd of the forward pass, and the ReLU-mask margin of every committed case.

The GPU tests (tests/test_exit_gen_kernels.py) compare the kernels with exit_ref; here exit_ref's hand-written
backward -- the formulas of exit_tail_bwd_gen_k, from h1, h2 and the saved statistics -- is held to autograd of
`tail_ref` (tests/test_exit_kernels.py) within 1e-10 of every element's sum of absolute terms, on every tail case.

The tuned-domain tables (TUNED_LIN_CASES, TUNED_TAIL_CASES, TUNED_EV_CASES; GPU: tests/test_exit_tuned_kernels.py):
every seed has its margin, every case satisfies the predicate by which the engine sends an exit to the tuned kernels,
the reference evaluated in float32 stays below 0.2 of every limit the GPU test applies, at most 0.1 % of a fused dz
lies within exit_ref.NEAR of a ReLU edge, and the tables' arrival changed no draw of an existing case.

The trained-net regimes (exit_ref.REGIMES; GPU: tests/test_exit_trained_regime.py): `regime=None` leaves every draw of
every table bit-identical; every (case, regime) has the property its regime is named for, its committed seed, and at
most 0.1 % of ReLU-mask elements that fp32 cannot tell; which limits the float32 reference itself cannot keep a fifth
of -- those the GPU file widens, printed here, no BatchNorm statistic of a `pivot` case among them; and the tuned
kernels' one-pass statistics restated in numpy float32 (exit_ref.pivoted_stats_f32): pivoted on row 0, as they were,
they miss the statistics limit on `pivot`; as shipped -- the pass repeated around the mean where it finds itself ill-
conditioned -- they use at most half of it at n = 128, 300, 1100 and 4096, also on the worst batch that is NOT repeated.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exit_ref as X
from test_exit_kernels import tail_ref
from test_exit_gen_kernels import bn_lim, dz_lim, fwd_lim, grad_lim, stat_lim

REL = 1e-10


def same(got, want, bound, what):
    err = np.abs(np.asarray(got) - np.asarray(want))
    lim = REL * np.maximum(np.asarray(bound), np.abs(want))
    assert got.shape == np.asarray(want).shape, what
    assert (err <= lim).all(), '%s: worst %.3g over the limit' % (what, float((err - lim).max()))


def autograd_inputs(d):
    """tail_ref wants a head and a router: a record without one gets an inert stand-in (zero gradient weights)."""
    n = d['n']
    z, y, wc = (d['z'], d['y'], d['w_cerr']) if d['head'] else (np.zeros((n, 2)), np.eye(2)[np.zeros(n, int)], np.zeros(n))
    if d['router']:
        h1, dr = d['h1'], d['dr']
        P = {k: d[k] for k in ('g1', 'b1', 'w2', 'bias2', 'g2', 'b2', 'w3', 'bias3')}
        mov = [d['m1'], d['v1'], d['m2'], d['v2']]
    else:
        h1, dr = np.zeros((n, 1)), np.zeros((n, 2))
        P = dict(g1=np.ones(1), b1=np.ones(1), w2=np.ones((1, 1)), bias2=np.zeros(1), g2=np.ones(1), b2=np.ones(1),
                 w3=np.ones((1, 2)), bias3=np.zeros(2))
        mov = [np.zeros(1), np.ones(1)] * 2
    return z, y, h1, P, wc, dr, mov


TUNED_TAILS = [(k, X.TUNED_TAIL_CASES) for k in sorted(X.TUNED_TAIL_CASES)]
ALL_TAILS = [(k, None) for k in sorted(X.TAIL_CASES)] + TUNED_TAILS


@pytest.mark.parametrize('name', sorted(X.TAIL_CASES))
def test_explicit_tail_matches_autograd(name, table=None):
    d = X.tail_inputs(name, table=table)
    z, y, h1, P, wc, dr, mov = autograd_inputs(d)
    moving = d['mode'] == 'moving'
    ref = tail_ref(z, y, h1, P, d['eps_ce'], d['bn_eps'], None if moving else wc, dr, max(d['S'], 2),
                   moving=mov if moving else None, bn_eps2=d['bn_eps2'])
    f = X.tail_fwd(d)
    if d['head']:
        same(f['c_err'], ref['c_err'], np.abs(ref['c_err']), 'c_err')
        assert np.array_equal(f['d_cor'], ref['d_cor'])
    if d['router']:
        same(f['h2'], ref['h2'], f['h2_bound'], 'h2')
        same(f['r'], ref['r'], f['r_bound'], 'r')
        (m1, v1), (m2, v2) = ref['stats']
        for k, want in (('m1', m1), ('v1', v1), ('m2', m2), ('v2', v2)):
            same(f[k], want, np.abs(want), k)
        same(f['bn_save'], np.concatenate([m1, 1 / np.sqrt(v1 + d['bn_eps']), m2, 1 / np.sqrt(v2 + d['bn_eps2'])]),
             np.abs(f['bn_save']), 'bn_save')
        for k, dec, new in (('m1', d['bn_decay'], m1), ('v1', d['bn_decay'], v1), ('m2', d['bn_decay2'], m2), ('v2', d['bn_decay2'], v2)):
            want = d[k].astype(np.float64) if moving else dec * d[k].astype(np.float64) + (1 - dec) * new
            same(f['avg'][('m1', 'v1', 'm2', 'v2').index(k)], want, np.abs(want), 'moving ' + k)
    if moving:
        return
    g = X.tail_bwd(d, f.get('h2'), X.split_save(f['bn_save'], d['R'], d['R2']) if d['router'] else None)
    if d['head']:
        same(g['dz'][0], ref['dz'], g['dz'][1], 'dz')
    if d['router']:
        same(g['dh1'][0], ref['dh1'], g['dh1'][1], 'dh1')
        for k in P:
            same(g['d' + k][0], ref['d' + k], g['d' + k][1], 'd' + k)
        assert set(g) == {'dh2', 'dh1'} | {'d' + k for k in P} | ({'dz'} if d['head'] else set())


@pytest.mark.parametrize('name', sorted(X.TUNED_TAIL_CASES))
def test_explicit_tuned_tail_matches_autograd(name):
    test_explicit_tail_matches_autograd(name, X.TUNED_TAIL_CASES)


def test_batch_of_one_has_zero_input_gradients(name='one', table=None):
    d = X.tail_inputs(name, table=table)
    f = X.tail_fwd(d)
    g = X.tail_bwd(d, f['h2'], X.split_save(f['bn_save'], d['R'], d['R2']))
    assert not g['dh1'][0].any() and not g['dh2'][0].any() and not f['v1'].any() and not f['v2'].any()


def test_tuned_batch_of_one_has_zero_input_gradients():
    test_batch_of_one_has_zero_input_gradients('t_one', X.TUNED_TAIL_CASES)


@pytest.mark.parametrize('name', sorted(X.TUNED_TAIL_CASES))
def test_tuned_relu_masks_are_unambiguous(name):
    test_relu_masks_are_unambiguous(name, X.TUNED_TAIL_CASES)


@pytest.mark.parametrize('name', sorted(X.TAIL_CASES))
def test_relu_masks_are_unambiguous(name, table=None):
    """The committed seed of every case keeps both router BatchNorms' outputs at least MARGIN from zero, so the fp32
    kernel and the float64 reference cannot disagree on a ReLU mask; and it is the first such seed of the draw."""
    d = X.tail_inputs(name, table=table)
    if not d['router']:
        return
    assert X.min_margin(d) >= X.MARGIN, (name, d['seed'], X.min_margin(d))
    assert X.scan_seed(name, table=table) == d['seed']


def test_the_two_batchnorms_differ_in_every_case():
    for name, table in ALL_TAILS:
        d = X.tail_inputs(name, table=table)
        assert d['bn_eps'] != d['bn_eps2'] and d['bn_decay'] != d['bn_decay2']
    assert sum(X.tail_inputs(k)['eps_ce'] == 0.1 and X.tail_inputs(k)['head'] for k in X.TAIL_CASES) >= 2


@pytest.mark.parametrize('case', X.LIN_CASES + X.LIN_MULTI + [c for c in X.TUNED_LIN_CASES if c not in X.LIN_CASES], ids=lambda c: 'n%d-K%d-M%d-%d' % (c[0], c[1] * c[2], c[4], c[5]))
def test_explicit_affine_maps_match_autograd(case):
    d = X.lin_inputs(case)
    ref = X.lin_ref(d)
    n, K = d['n'], d['K']
    T = lambda a, g=False: torch.tensor(np.nan_to_num(np.asarray(a, np.float64)), requires_grad=g)
    a = T(X.act(d['x'], d['mode'], d['gamma'], d['beta'], d['m_avg'], d['v_avg']).reshape(n, K), True)
    kc = T(d['kc'])
    loss, ws, bs = 0, [None, None], [None, None]
    for s in range(2):
        if d['w'][s] is None:
            continue
        ws[s], bs[s] = T(d['w'][s], True), T(d['b'][s], True)
        y = a @ ws[s][:K] + bs[s]
        if d['extra'][s]:
            y = y + X.ALPHA_CPT * kc[:, None] * ws[s][K]
        same(ref['y'][s][0], y.detach().numpy(), ref['y'][s][1], 'y')
        loss = loss + (T(d['dy'][s]) * y).sum()
    loss.backward()
    same(ref['dx'][0], a.grad.numpy(), ref['dx'][1], 'dx')
    for s in range(2):
        if ws[s] is None:
            assert ref['dw'][s] is None and ref['y'][s] is None
            continue
        rows = K + 1 if d['extra'][s] else K
        assert ref['dw'][s][0].shape == (rows, d['M'][s])
        same(ref['dw'][s][0], ws[s].grad.numpy()[:rows], ref['dw'][s][1], 'dW')
        same(ref['db'][s][0], bs[s].grad.numpy(), ref['db'][s][1], 'db')


# ---------------------------------------------------------------------------------------------------- the tuned tables
# sha256 (first 16 hex digits) of every existing case's inputs, taken before the TUNED_* tables and the `table`
# argument of tail_inputs / scan_seed came: a draw depends on the case's position in ITS table, and the scanned seeds
# on the draw.
TAIL_DRAWS = {
    'one': 'c4e15ce824c27477', 'unit': '3e87e19342060232', 'class17': '54e72e7e51c94fdf', 'limits': 'd6955ceb499d6cd4',
    'w2lds': '3db5a2180f2b2c59', 'w2glob': '5adece6d14a75161', 'ship129': '7135b8a06a81274d', 'ship300': 'c5643c09bbab897c',
    'rows1100': '6bc72c974dae6a6b', 'odd': 'cbe4127ba0e60008', 'headonly': '5ba966f6955ed1e5', 'routeronly': 'e1ded68971a4bbc0',
    'moving': '44dad647e5890d8b', 'table0': '506f3a4c8c970dbe', 'table1': '8662f9708675c216',
}
LIN_DRAWS = {
    (5, 1, 3, 'identity', 2, 1, ''): '45581151b0323577', (17, 5, 3, 'batch', 17, 33, 'r'): '9afc73b0bdf897fa',
    (1, 16, 16, 'batch', 10, 16, 'r'): '3ac3fb859022ebf6', (16, 4, 24, 'moving', 0, 40, ''): '59859430f2584a43',
    (33, 16, 16, 'batch', 10, 0, ''): '7f4776164ed0a9bd', (37, 16, 32, 'batch', 100, 32, 'r'): '9c29d3ae0b6de4e7',
    (129, 4, 16, 'batch', 130, 256, 'hr'): '0904e487361041fa', (5, 257, 16, 'batch', 16, 16, ''): '6acb63a14e0e7b59',
    (200, 1, 256, 'batch', 1024, 16, 'r'): '56bd8921ec99c453', (5, 4, 24, 'moving', 0, 40, ''): '6caa80bcb9964937',
    (129, 1, 16, 'batch', 130, 0, 'h'): 'bdc7be63840d245c',
}


def digest(d):
    h = hashlib.sha256()
    for k in sorted(d):
        v = d[k]
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            h.update(k.encode())
            h.update(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else repr(a).encode())
    return h.hexdigest()[:16]


# ... and of the tuned tables, taken before the `regime` argument came
TUNED_TAIL_DRAWS = {
    't_one': '489fa5cd6963495d', 't_r5': 'eddde8c3d8d2218f', 't_full': '0e88e83f00c43e82', 't_stride': '1e78866b49932934',
    't_router': '177bd580b24655f5', 't_head': '94ad84e463b30009', 't_moving': 'f087bffe51107d87',
    't_moving_big': '0b6ec9329ef82436', 't_r3_big': '70a104288cee5301',
}
TUNED_LIN_DRAWS = {
    (5, 1, 16, 'identity', 2, 1, ''): 'f061b2728336e0a8', (17, 15, 48, 'batch', 16, 5, 'r'): '4db5b064e7f79e04',
    (33, 3, 80, 'moving', 10, 0, ''): 'd32bd181677d7a34', (1, 16, 16, 'batch', 10, 16, 'r'): '3ac3fb859022ebf6',
    (37, 7, 112, 'batch', 0, 16, 'r'): '75d592cf8d1b1f5c', (130, 6, 96, 'batch', 16, 16, 'hr'): 'bf56e1afbd044918',
    (9, 13, 112, 'batch', 10, 16, 'r'): '5d2bb971561cf89b', (200, 4, 128, 'batch', 10, 16, ''): '9a16737f310f78fc',
    (520, 1, 32, 'batch', 3, 8, 'r'): 'edb8d699e97bdf96',
}


def test_existing_draws_are_unchanged():
    assert set(TAIL_DRAWS) == set(X.TAIL_CASES) and set(LIN_DRAWS) == set(X.LIN_CASES + X.LIN_MULTI)
    assert set(TUNED_TAIL_DRAWS) == set(X.TUNED_TAIL_CASES) and set(TUNED_LIN_DRAWS) == set(X.TUNED_LIN_CASES)
    for name, want in TAIL_DRAWS.items():
        assert digest(X.tail_inputs(name)) == want, name
        assert digest(X.tail_inputs(name, table=X.TAIL_CASES)) == want, name
        assert digest(X.tail_inputs(name, regime=None)) == want, name
    for name, want in TUNED_TAIL_DRAWS.items():
        assert digest(X.tail_inputs(name, table=X.TUNED_TAIL_CASES, regime=None)) == want, name
    for case, want in list(LIN_DRAWS.items()) + list(TUNED_LIN_DRAWS.items()):
        assert digest(X.lin_inputs(case)) == want, case
        assert digest(X.lin_inputs(case, regime=None)) == want, case


def tuned_exit(C_, K, n_cls, R, R2, n_sinks):
    """lib/_eng_alloc.py, `tuned = ...`: the exits the engine sends to lin.hip / exit_tail.hip / exit_ev.hip (n_cls = 0:
    no head; R = R2 = 0: no router), and its limit of MAX_SINKS = 4 sinks under a switch."""
    return C_ <= 128 and C_ % 16 == 0 and K % 16 == 0 and n_cls <= 16 and R == R2 and R <= 16 and n_sinks <= 4


def ev_host_record(case):
    """A HOST mpnn_exit_ev_args of one TUNED_EV_CASES row for mpnn_exit_ev_check, which looks at sizes and at which
    pointers are NULL and follows none: every pointer the launch would carry is the same non-NULL stand-in."""
    from lib import _hip
    seed, N, count, HW, C_, nc, R, S, dyn, head, router, lists = case
    some = 4096
    e = _hip.ExitEvArgs()
    e.a.x, e.a.C, e.a.mode = some, C_, _hip.ACT_BN_MOVING
    e.HW, e.n, e.n_cls, e.R, e.R2, e.n_sinks, e.r_stride, e.extra_col = HW, N, nc, R, R, S, 4, int(dyn)
    for k in ('b_head', 'y', 'c_err', 'd_cor', 'b1', 'k_cpt', 'g1', 'be1', 'm1', 'v1', 'w2', 'bias2', 'g2', 'be2', 'm2', 'v2',
              'w3', 'bias3', 'r', 'idx', 'cnt'):
        setattr(e, k, some)
    e.w_head, e.w1 = (some if head else None), (some if router else None)
    for i in lists:
        e.child_idx[i] = e.child_cnt[i] = some
    return e


def test_every_tuned_case_lies_in_the_tuned_domain():
    from lib import _hip
    for n, HW, C_, mode, M0, M1, ex in X.TUNED_LIN_CASES + X.TUNED_LIN_MULTI:
        assert tuned_exit(C_, HW * C_, M0, M1, M1, 2), (n, HW, C_)
    assert max(c[0] for c in X.TUNED_LIN_MULTI) == 130 and max(c[1] * c[2] for c in X.TUNED_LIN_MULTI) == 784
    for name, table in TUNED_TAILS + [(k, None) for k in ('ship129', 'ship300', 'rows1100', 'headonly')]:
        d = X.tail_inputs(name, table=table)
        assert tuned_exit(16, 256, d['nc'] if d['head'] else 0, d['R'], d['R2'], d['S']), name
        assert d['n'] != 2 and d['S'] <= d['stride']
    lib = _hip.load()
    for name, case in X.TUNED_EV_CASES.items():
        seed, N, count, HW, C_, nc, R, S, dyn, head, router, lists = case
        assert lib.mpnn_exit_ev_check(ctypes.byref(ev_host_record(case))) == 0, name
        if name != 'ev_c20':                               # (the one record the check admits and the engine never sends)
            assert tuned_exit(C_, HW * C_, nc if head else 0, R if router else 0, R if router else 0, S if router else 0), name
    assert not tuned_exit(*(lambda c: (c[4], c[3] * c[4], c[5], c[6], c[6], c[7]))(X.TUNED_EV_CASES['ev_c20']))


worst = lambda got, ref, lim: float((np.abs(np.asarray(got, np.float64) - ref) / lim).max()) if np.size(ref) else 0.0


def lin_ratios(case, regime=None):
    """Worst error / limit of the float32 evaluation of one affine case, by quantity, and the share of its fused dz
    within NEAR of a ReLU edge."""
    d = X.lin_inputs(case, regime=regime)
    r64, r32 = X.lin_ref(d), X.lin_ref(d, np.float32)
    out, share = {}, 0.0
    up = lambda k, v: out.__setitem__(k, max(out.get(k, 0.0), v))
    for s in range(2):
        if d['w'][s] is not None:
            up('y', worst(r32['y'][s][0], r64['y'][s][0], fwd_lim(*r64['y'][s])))
            up('dW', worst(r32['dw'][s][0], r64['dw'][s][0], grad_lim(*r64['dw'][s])))
            up('db', worst(r32['db'][s][0], r64['db'][s][0], grad_lim(*r64['db'][s])))
    up('dx', worst(r32['dx'][0], r64['dx'][0], grad_lim(*r64['dx'])))
    if d['mode'] == 'batch':
        f64, f32 = X.lin_fused(d, r64), X.lin_fused(d, r32, np.float32)
        on, share = X.dz_resolve(f32['dz'][0], f64)
        up('dz', worst(f32['dz'][0], on * f64['dx'], grad_lim(None, on * f64['dxb'])))
        red, bound = X.fused_red(f64, on, d['C'])
        up('red', worst(X.fused_red(f32, f32['on'], d['C'])[0], red, grad_lim(red, bound)))
    return out, share


def tail_ratios(name, table):
    d = X.tail_inputs(name, table=table)
    f64, f32 = X.tail_fwd(d), X.tail_fwd(d, np.float32)
    out = {}
    if d['head']:
        out['c_err'] = worst(f32['c_err'], f64['c_err'], stat_lim(f64['c_err']))
    if d['router']:
        for k in ('h2', 'r', 'bn_save'):
            out[k] = worst(f32[k], f64[k], stat_lim(f64[k]))
        out['avg'] = max(worst(a, b, stat_lim(b)) for a, b in zip(f32['avg'], f64['avg']))
    if d['mode'] != 'batch':
        return out
    sv = lambda f: X.split_save(f['bn_save'], d['R'], d['R2']) if d['router'] else None
    g64, g32 = X.tail_bwd(d, f64.get('h2'), sv(f64)), X.tail_bwd(d, f32.get('h2'), sv(f32), np.float32)
    for k in g64:
        lim = dz_lim if k == 'dz' else grad_lim if k in ('dw3', 'dbias3') else bn_lim
        out[k] = worst(g32[k][0], g64[k][0], lim(*g64[k]))
    return out


def test_float32_reference_keeps_a_fifth_of_every_tuned_limit():
    """The rule tests/test_exit_gen_kernels.py states for its tables, asserted for the tuned ones: a correct float32
    evaluation of the same arithmetic uses at most 0.2 of each limit, so the limits are not set by the kernels."""
    top = {}
    for case in X.TUNED_LIN_CASES:
        out, share = lin_ratios(case)
        assert share <= 1e-3, (case, share)
        for k, v in out.items():
            top[k] = max(top.get(k, 0.0), v)
    for name, table in TUNED_TAILS + [(k, None) for k in ('ship129', 'ship300', 'rows1100', 'headonly')]:
        for k, v in tail_ratios(name, table).items():
            top['tail ' + k] = max(top.get('tail ' + k, 0.0), v)
    print(' '.join('%s %.3g' % kv for kv in sorted(top.items())))
    assert max(top.values()) <= 0.2, top


# ---------------------------------------------------------------------------------------------------- trained-net regimes
import test_exit_trained_regime as T

ALL_RUNS = X.REGIME_RUNS + [c for c in X.BOTH_REGIME_RUNS if c not in X.REGIME_RUNS]
RUN_ID = ['%s-%s' % c for c in ALL_RUNS]


def regime_inputs(name, regime):
    return X.tail_inputs(name, table=X.tail_table(name), regime=regime)


def test_regime_runs_are_the_planned_ones():
    assert len(set(ALL_RUNS)) == len(ALL_RUNS) == 20 and set(X.REGIME_SEEDS) == set(ALL_RUNS)
    for name, regime in X.TUNED_REGIME_RUNS + X.BOTH_REGIME_RUNS:
        d = regime_inputs(name, regime)
        assert tuned_exit(16, 256, d['nc'] if d['head'] else 0, d['R'], d['R2'], d['S']), name
    for name, regime in ALL_RUNS:
        d = regime_inputs(name, regime)
        assert set(regime.split('+')) <= set(X.REGIMES) and (d['mode'] == 'moving') == (regime == 'moving')
        assert all(v.dtype == np.float32 for v in d.values() if isinstance(v, np.ndarray)), (name, regime)
        assert digest(d) == digest(regime_inputs(name, regime)) != digest(X.tail_inputs(name, d['seed'], X.tail_table(name)))


@pytest.mark.parametrize('name,regime', ALL_RUNS, ids=RUN_ID)
def test_regime_seed_and_masks(name, regime):
    """The committed seed is the first whose float64 pre-activations all lie MARGIN from zero and of whose mask elements
    at most 0.1 % are ambiguous in fp32 -- conditions on the inputs, met by the float64 reference alone."""
    d = regime_inputs(name, regime)
    assert d['seed'] == X.REGIME_SEEDS[name, regime]
    if d['router']:
        assert X.min_margin(d) >= X.MARGIN and X.ambiguous(d)[1] <= 1e-3, (name, regime, X.min_margin(d), X.ambiguous(d)[1])
        assert X.scan_seed(name, table=X.tail_table(name), regime=regime) == d['seed']


@pytest.mark.parametrize('name,regime', ALL_RUNS, ids=RUN_ID)
def test_regime_has_the_property_it_is_named_for(name, regime):
    d = regime_inputs(name, regime)
    f = X.tail_fwd(d)
    parts = regime.split('+')
    if d['head'] and ('confident' in parts or 'offset' in parts):
        p32 = X.tail_fwd(d, np.float32)['p']
        assert (p32 == 0).any() and (f['p'][p32 == 0] < 1e-45).all()                      # exactly 0 in fp32
        top = np.sort(d['z'], 1)
        tie = np.flatnonzero(top[:, -1] == top[:, -2])
        assert list(tie) == [2, 3] and list(f['d_cor'][tie]) == [1.0, 0.0]                # the label first, then second
        assert all(np.flatnonzero(d['z'][r] == top[r, -1]).tolist()[i] == d['y'][r].argmax() for r, i in ((2, 0), (3, 1)))
        gap = top[:, -1] - top[:, -2]
        assert np.median(gap) >= 10 and gap.max() <= 60
        assert (f['d_cor'] == 0).sum() >= 2 and (f['p'].max(1)[f['d_cor'] == 0] > 0.99).sum() >= 1     # confidently wrong
        w = d['w_cerr']
        assert (w == 0).sum() == d['n'] // 4 and (w == np.float32(1e-8)).sum() == 3 and (w == 1).sum() == 1 and w[:5].all()
        if 'offset' in parts:
            assert (np.abs(d['z']).min(1) > 9e3).all() and {-1.0, 1.0} == set(np.sign(d['z'][:, 0]))
    if 'pivot' in parts:
        rest = d['h1'][1:].astype(np.float64)               # (of the rest of the batch: WITH row 0 in them, one outlier
        k = np.abs(d['h1'][0] - rest.mean(0)) / rest.std(0)  # can lie at most sqrt(n - 1) standard deviations out)
        assert k.max() >= 6 and (d['R'] < 3 or k.max() >= 50), k
        h2 = f['h2'][1:]
        assert (np.abs(f['h2'][0] - h2.mean(0)) / h2.std(0)).max() >= 6                   # the second pivot row too
    if 'shifted' in parts:
        sd = d['h1'].astype(np.float64).std(0)
        assert np.abs(d['h1'].mean(0)).max() > 20 and sd.min() < 0.1 and sd.max() > 1 and np.ptp(f['r']) > 10
    if 'dead' in parts:
        assert f['v1'][0] == 0 and f['v2'][0] == 0                                         # exactly constant channels
        for pre, W in ((f['pre1'], d['R']), (f['pre2'], d['R2'])):
            assert (pre[:, 0] < 0).all()                                                   # a fully masked column
            assert W < 3 or (pre[:, 2] > 0).all()                                          # a fully live one
            assert W < 6 or (pre[:, 5] < -0.9).all()
            assert W < 7 or (pre[:, 6] > 0.9).all()
        if d['R'] > 1 and d['n'] > 1:
            assert 0 < f['v1'][1] < 1e-9
        if d['R'] > 4:
            assert d['g1'][2] == np.float32(1e-4) and d['g1'][3] == 20 and d['g1'][4] < 0 and d['g2'][4] < 0
    if 'moving' in parts:
        for k in ('1', '2'):
            assert set(d['v' + k]) == set(np.float32([0, 1e-8, 1e-3, 1, 1e4])) and d['g' + k][4] < 0
        assert np.abs(d['m1'] - d['h1'].mean(0)).max() > 100


def test_float32_reference_in_the_regimes():
    """Which limits hold in the regimes.  For every quantity the GPU file compares, the float32 evaluation of the
    reference (as written and with the batch rows reversed: exit_ref.f32_errors) against the existing limit: at most 0.2
    -- the limit stands; above -- the GPU file holds the quantity to max(limit, 5 x that error) (exit_ref.widened).  The
    widened triples are printed.  No BatchNorm statistic of a `pivot` case is among them: there the two-pass float32
    form stays at or below 0.1."""
    wide = []
    for name, regime in ALL_RUNS:
        d, f, g, L, amb = T.reference(name, regime)
        for k, (lim, ratio, floor) in sorted(L.items()):
            assert np.isfinite(ratio) and (floor > 0) == (ratio > 0.2)
            if ratio > 0.2:
                wide.append('%s/%s %s %.3g' % (name, regime, k, ratio))
            if 'pivot' in regime and k in ('bn_save1', 'bn_save2', 'm1', 'v1', 'm2', 'v2'):
                assert ratio <= 0.1, (name, regime, k, ratio)
            if k in ('bn_save1', 'bn_save2', 'm1', 'v1', 'm2', 'v2', 'c_err', 'dz', 'dbias3', 'db1', 'db2', 'dbias2'):
                assert ratio <= 0.2, (name, regime, k, ratio)                              # (never widened anywhere)
    print('widened: ' + '; '.join(wide))
    assert wide and all(q.split()[1] in ('h2', 'r', 'dw3', 'dh2', 'dh1', 'dw2', 'dg1', 'dg2') for q in wide)


STAT_N = (128, 300, 1100, 4096)


def pivot_batch(n, R=16):
    """h1 of the `pivot` regime at any batch size (the regime's own draw, from a generator of the size's own)."""
    d = dict(n=n, R=R, router=True, w2=np.ones((R, R), np.float32), w3=np.ones((R, 2), np.float32))
    X.REGIMES['pivot'](d, np.random.default_rng([n, R]))
    return d['h1']


def stat_ratios(h, eps, form):
    h64 = np.asarray(h, np.float64)
    m = h64.mean(0)
    v = ((h64 - m) ** 2).mean(0)
    got = X.pivoted_stats_f32(h, len(h), eps, form)
    return [worst(a, b, stat_lim(b)) for a, b in zip(got, (m, v, 1 / np.sqrt(v + eps)))]


def test_restated_pivoted_statistics():
    """exit_ref.pivoted_stats_f32 -- bn_stats (n <= 128) and router_fwd_big + block_sums + stats_finish (n > 128) of
    csrc/exit_tail.hip restated in numpy float32 -- on the `pivot` regime against the statistics limit 2e-5 (1 + |ref|):
    the form pivoted on row 0 exceeds it (mean, variance or rstd) at every size, the shipped form (the pass repeated
    around the mean where (mean - pivot)^2 > REDO var) uses at most half of it, also where row 0 lies just inside that
    threshold in EVERY channel, so that nothing is repeated; both BatchNorms of every `pivot` case of the GPU file as well.  On
    the draws at initialisation both forms keep well inside it."""
    for n in STAT_N:
        h = pivot_batch(n)
        old, new = stat_ratios(h, 1e-6, 'row0'), stat_ratios(h, 1e-6, 'shipped')
        print('n %4d   row 0: mean %.3g var %.3g rstd %.3g   shipped: mean %.3g var %.3g rstd %.3g' % (n, *old, *new))
        assert max(old) > 1, (n, old)
        assert max(new) <= 0.5, (n, new)
        edge = np.random.default_rng(n + 1).standard_normal((n, 16))       # row 0 at 5.3 sd of the batch: (mean - pivot)^2 = 28 var
        edge = (3 + edge / edge[1:].std(0)).astype(np.float32)
        edge[0] = 3 + 5.3 / np.sqrt(1 - 28 / n)
        m, v = edge.astype(np.float64).mean(0), edge.astype(np.float64).var(0)
        assert 25 < ((edge[0] - m) ** 2 / v).min() and ((edge[0] - m) ** 2 / v).max() < X.REDO
        assert stat_ratios(edge, 1e-6, 'shipped') == stat_ratios(edge, 1e-6, 'row0') and max(stat_ratios(edge, 1e-6, 'shipped')) <= 0.5
        plain = np.random.default_rng(n).standard_normal((n, 16)).astype(np.float32)
        assert max(stat_ratios(plain, 1e-6, 'row0') + stat_ratios(plain, 1e-6, 'shipped')) <= 0.2
    for name, regime in ALL_RUNS:
        d = regime_inputs(name, regime)
        if 'pivot' in regime and d['R'] <= 16:
            h2 = X.tail_fwd(d, np.float32)['h2']
            for h, eps in ((d['h1'], d['bn_eps']), (h2, d['bn_eps2'])):
                new = stat_ratios(h, eps, 'shipped')
                print('%s/%s   shipped: mean %.3g var %.3g rstd %.3g   row 0: %s' % (name, regime, *new, ' '.join('%.3g' % v for v in stat_ratios(h, eps, 'row0'))))
                assert max(new) <= 0.5, (name, regime, new)


@pytest.mark.parametrize('case', T.TUNED_LINS + T.GEN_LINS, ids=T.LIN_ID)
def test_trained_affine_maps(case):
    """The `trained` regime of the affine maps: its properties, and which limits the float32 reference keeps a fifth of
    (test_exit_trained_regime.lin_floors; the others are printed: the GPU file raises them to 5 x that error)."""
    d = X.lin_inputs(case, regime='trained')
    assert all(v.dtype == np.float32 for v in (d['x'], d['gamma'], d['beta'], d['v_avg']))
    x = d['x'].astype(np.float64).reshape(-1, d['C'])
    m, v = (x.mean(0), x.var(0)) if d['mode'] == 'batch' else (d['m_avg'], d['v_avg'].astype(np.float64))
    pre = d['gamma'] * (x - m) / np.sqrt(v + 1e-6) + d['beta']
    assert (pre[:, 0] < 0).all() and (pre[:, 1] > 0).all() and 0.6 < (pre < 0).mean() < 0.8
    assert (d['gamma'] < 0).any() and (d['gamma'] > 0).any() and (np.isnan(d['kc']).all() or (0 <= d['kc'].min() and d['kc'].max() <= 1))
    assert x.std(0).max() / x.std(0).min() > 100 and d['v_avg'].max() / d['v_avg'].min() > 1e4
    ref = X.lin_ref(d)
    for s in range(2):
        if d['w'][s] is not None:
            assert not ref['dw'][s][0][:d['K']][0::d['C']].any()                           # the dead channel's dW rows: exactly 0
    out, share = lin_ratios(case, 'trained')
    assert share <= 1e-3, share
    floors = T.lin_floors(d, ref, X.lin_fused(d, ref) if d['mode'] == 'batch' else None)
    assert all((floor > 0) == (ratio > 0.2) and np.isfinite(ratio) for ratio, floor in floors.values()), floors
    assert all(floors[k][0] <= 0.2 for k in floors if k[:2] == 'db' or k == 'dx')
    print('widened: ' + ' '.join('%s %.3g' % (k, v[0]) for k, v in sorted(floors.items()) if v[1]))
