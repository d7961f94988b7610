"""CPU: the explicit float64 reference of the any-width exit path (tests/exit_ref.py) against torch-CPU float64
autograd of the forward pass, and the ReLU-mask margin of every committed case.

The GPU tests (tests/test_exit_gen_kernels.py) compare the kernels with exit_ref; here exit_ref's hand-written
backward -- the formulas of exit_tail_bwd_gen_k, from h1, h2 and the saved statistics -- is held to autograd of
`tail_ref` (tests/test_exit_kernels.py) within 1e-10 of every element's sum of absolute terms, on every tail case.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exit_ref as X
from test_exit_kernels import tail_ref

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


@pytest.mark.parametrize('name', sorted(X.TAIL_CASES))
def test_explicit_tail_matches_autograd(name):
    d = X.tail_inputs(name)
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


def test_batch_of_one_has_zero_input_gradients():
    d = X.tail_inputs('one')
    f = X.tail_fwd(d)
    g = X.tail_bwd(d, f['h2'], X.split_save(f['bn_save'], d['R'], d['R2']))
    assert not g['dh1'][0].any() and not g['dh2'][0].any() and not f['v1'].any() and not f['v2'].any()


@pytest.mark.parametrize('name', sorted(X.TAIL_CASES))
def test_relu_masks_are_unambiguous(name):
    """The committed seed of every case keeps both router BatchNorms' outputs at least MARGIN from zero, so the fp32
    kernel and the float64 reference cannot disagree on a ReLU mask; and it is the first such seed of the draw."""
    d = X.tail_inputs(name)
    if not d['router']:
        return
    assert X.min_margin(d) >= X.MARGIN, (name, d['seed'], X.min_margin(d))
    assert X.scan_seed(name) == d['seed']


def test_the_two_batchnorms_differ_in_every_case():
    for name in X.TAIL_CASES:
        d = X.tail_inputs(name)
        assert d['bn_eps'] != d['bn_eps2'] and d['bn_decay'] != d['bn_decay2']
    assert sum(X.tail_inputs(k)['eps_ce'] == 0.1 and X.tail_inputs(k)['head'] for k in X.TAIL_CASES) >= 2


@pytest.mark.parametrize('case', X.LIN_CASES + X.LIN_MULTI, ids=lambda c: 'n%d-K%d-M%d-%d' % (c[0], c[1] * c[2], c[4], c[5]))
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
