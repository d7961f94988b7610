"""CPU: the explicit float64 reference of the any-width exit path (tests/exit_ref.py) against torch-CPU float64
autograd of the forward pass, and the ReLU-mask margin of every committed case.

The GPU tests (tests/test_exit_gen_kernels.py) compare the kernels with exit_ref; here exit_ref's hand-written
backward -- the formulas of exit_tail_bwd_gen_k, from h1, h2 and the saved statistics -- is held to autograd of
`tail_ref` (tests/test_exit_kernels.py) within 1e-10 of every element's sum of absolute terms, on every tail case.

The tuned-domain tables (TUNED_LIN_CASES, TUNED_TAIL_CASES, TUNED_EV_CASES; GPU: tests/test_exit_tuned_kernels.py):
every seed has its margin, every case satisfies the predicate by which the engine sends an exit to the tuned kernels,
the reference evaluated in float32 stays below 0.2 of every limit the GPU test applies, at most 0.1 % of a fused dz
lies within exit_ref.NEAR of a ReLU edge, and the tables' arrival changed no draw of an existing case.
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


def test_existing_draws_are_unchanged():
    assert set(TAIL_DRAWS) == set(X.TAIL_CASES) and set(LIN_DRAWS) == set(X.LIN_CASES + X.LIN_MULTI)
    for name, want in TAIL_DRAWS.items():
        assert digest(X.tail_inputs(name)) == want, name
        assert digest(X.tail_inputs(name, table=X.TAIL_CASES)) == want, name
    for case, want in LIN_DRAWS.items():
        assert digest(X.lin_inputs(case)) == want, case


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


def lin_ratios(case):
    """Worst error / limit of the float32 evaluation of one affine case, by quantity, and the share of its fused dz
    within NEAR of a ReLU edge."""
    d = X.lin_inputs(case)
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
