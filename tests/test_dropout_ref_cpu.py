"""CPU: the reference of Dropout (tests/dropout_ref.py), the layer's host side and the exit planner with the layer.

* Philox4x32-10: three known answers -- by the numpy generator, by the plain-Python-int one and by the kernels' own routine
  compiled for the host (mpnn_philox4x32_10) --, the two restatements against each other on random counters;
* thresh: λ = 1 keeps everything, λ = 0.5 is 2^31, a word equal to thresh keeps, a tiny λ clips to 2^32 - 1; the planner's
  lib._eng_common.dropout_thresh is the same function;
* statistics with fixed seeds: the kept fraction of 262 144 draws at λ = 0.1, 0.5, 0.9 within 5 σ of λ; two step counters,
  and two leaves, give masks that differ in 2 λ (1 - λ) of the elements within 5 σ;
* the float64 layer and its backward against torch autograd on x m / λ; the float32 stand-ins keep dropped elements exact;
* link: x passes through, λ out of range and a bad seed are ValueErrors; every position but the one in front of a head's
  LinTrans is refused with a NotImplementedError that names it (router and block chains, Conv nets, beside a 'map'
  ActivityError, twice in one head); reg / exit_dropout / dropout_seed build the chains; parse_exit_dropout; the seed per
  net and per data-parallel rank; the record's layout as gcc sees the header;
* the exit planner, run on the host over CPU tensors: with the layer the two launches and the extra lin records appear
  exactly for the exits that carry it; with λ = 1, or without the layer, the launch list and every record field are what
  they are without it.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dropout_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'dropout_ref_graph.npz')
sys.path.insert(0, os.path.join(HERE, 'golden'))
KNOWN = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
hexes = lambda w: ' '.join('%08x' % int(v) for v in w)


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize('ctr,key,want', KNOWN)
def test_known_answers(ctr, key, want):
    from lib import _hip
    assert hexes(R.philox(np.array(ctr, np.uint32), np.array(key, np.uint32))) == want
    assert hexes(R.philox_int(ctr, key)) == want
    out = (C.c_uint * 4)()
    assert _hip.load().mpnn_philox4x32_10((C.c_uint * 4)(*ctr), (C.c_uint * 2)(*key), out) == 0
    assert hexes(out) == want


def test_the_two_restatements_agree_on_random_counters():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, (200, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, (200, 2), dtype=np.uint64).astype(np.uint32)
    got = R.philox(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (200, 4)
    for c, k, g in zip(ctr, key, got):
        assert tuple(int(v) for v in g) == R.philox_int(c, k)
    # one key for many counters (the launch's form), and the words of a map: word k & 3 of counter (k >> 2, s, leaf, t)
    assert np.array_equal(R.philox(ctr, key[0]), np.stack([R.philox(c, key[0]) for c in ctr]))
    seed, t, leaf = 2 ** 40 + 7, 9, 3
    w = R.words(seed, t, leaf, 3, 10)
    assert w.shape == (3, 10)
    for s in range(3):
        for k in range(10):
            assert int(w[s, k]) == R.philox_int((k >> 2, s, leaf, t), (seed & 0xffffffff, seed >> 32))[k & 3]


def test_thresh():
    from lib._eng_common import dropout_thresh
    assert R.thresh(1) == R.thresh(1.0) == 0 and R.mask(0, 0, 0, 7, 13, 1.0).all()
    assert R.thresh(0.5) == 1 << 31
    assert R.thresh(0.25) == 3 << 30 and R.thresh(0.9) == int(np.ceil((1.0 - 0.9) * 2.0 ** 32))
    assert R.thresh(1e-300) == R.thresh(2.0 ** -60) == 2 ** 32 - 1            # ((1 - λ) 2^32 rounds to 2^32: clipped)
    assert R.thresh(2.0 ** -32) == 2 ** 32 - 1 and R.thresh(2.0 ** -31) == 2 ** 32 - 2
    for λ in (1, 0.9, 0.5, 0.1, 1e-3, 2.0 ** -40):
        assert dropout_thresh(λ) == R.thresh(λ)
    # the boundary: a word equal to thresh keeps, one below it drops
    w = R.words(5, 1, 2, 4, 8)
    th = int(w[1, 3])
    keep = w >= np.uint32(th)
    assert keep[1, 3] and not (w[~keep] >= th).any() and (w[keep] >= th).all()
    assert not (w >= np.uint32(min(th + 1, 2 ** 32 - 1)))[1, 3] or th == 2 ** 32 - 1


@pytest.mark.parametrize('λ', [0.1, 0.5, 0.9])
def test_kept_fraction_and_the_distance_between_masks(λ):
    n, K = 512, 512                                        # 262 144 draws
    N = n * K
    σ = np.sqrt(λ * (1 - λ) / N)
    m = R.mask(1234, 0, 0, n, K, λ)
    assert abs(m.mean() - λ) <= 5 * σ, (m.mean(), λ, σ)
    # another step counter, another leaf, another seed: independent masks, which differ where exactly one keeps
    q = 2 * λ * (1 - λ)
    σq = np.sqrt(q * (1 - q) / N)
    for other in (R.mask(1234, 1, 0, n, K, λ), R.mask(1234, 0, 1, n, K, λ), R.mask(1235, 0, 0, n, K, λ), R.mask(1234 + 2 ** 32, 0, 0, n, K, λ)):
        assert abs(other.mean() - λ) <= 5 * σ
        assert abs((m != other).mean() - q) <= 5 * σq, ((m != other).mean(), q)
    # ... and depends on nothing else: a row is the same row in a smaller batch, a column the same column in a narrower map
    assert np.array_equal(R.mask(1234, 0, 0, 3, K, λ), m[:3]) and np.array_equal(R.mask(1234, 0, 0, n, 10, λ), m[:, :10])
    # rows and columns are independent too (a counter that ignored s or k would repeat)
    assert abs((m[0::2] != m[1::2]).mean() - q) <= 5 * np.sqrt(q * (1 - q) / (N / 2))
    assert abs((m[:, 0::2] != m[:, 1::2]).mean() - q) <= 5 * np.sqrt(q * (1 - q) / (N / 2))


# ------------------------------------------------------------------ the reference against the reference's own layer
def test_golden_vectors_of_the_reference_layer():
    """The reference's own Dropout.link over the stand-in's tf.nn.dropout (x / keep_prob * floor(keep_prob + u), u injected from
    the same words): the literal lines of tests/dropout_ref.py give its output, and the zero pattern is the mask."""
    import dropout_ref_graph as G
    assert os.path.getsize(GOLDEN) < 200 * 1024
    with np.load(GOLDEN) as gold:
        for key, case in G.LAYER_CASES.items():
            x = G.layer_input(case)
            n, K = x.shape[0], int(np.prod(x.shape[1:]))
            m = R.mask(case['seed'], 0, case['leaf'], n, K, case['λ'])
            g = gold['layer/%s/x' % key]
            assert g.shape == x.shape and np.array_equal(g.reshape(n, K) != 0, m), key
            assert np.abs(R.layer(x.reshape(n, K), m, case['λ']) - g.reshape(n, K)).max() <= 1e-12 * (1 + np.abs(g).max()), key
    assert {len(c['shape']) for c in G.LAYER_CASES.values()} == {2, 4}


@pytest.mark.parametrize('key', ['sr', 'actor'])
def test_refnet_dropout_reproduces_the_reference_net_in_tr_and_departs_from_it_in_ev(key):
    import arch_and_hypers as A
    import lib.net_types as NT
    import dropout_ref_graph as G
    import make_ref_graph_golden as M
    from lib._eng_common import _kind, head_dropout
    from test_ref_graph_golden import ordered
    spec = G.NETS[key]
    net = G.dropout_chain(A, NT, spec)((32, 32, 3), (10,))
    params = ordered(net)
    rng = np.random.RandomState(spec['seed'])
    vals = {id(p): M.param_value(n, p.shape, rng) for n, p in params}
    leaves = [ℓ for ℓ in net.layers if not ℓ.sinks]
    assert all([type(c).__name__ for c in ℓ.comps] == ['Select', 'Dropout', 'LinTrans', 'Softmax', 'CrossEntropyError'] and _kind(ℓ) == 'head'
               for ℓ in leaves)
    blocks = [2] if key == 'sr' else [0, 1, 2]
    assert [(head_dropout(ℓ).hypers.λ, head_dropout(ℓ).hypers.seed) for ℓ in leaves] == [(G.DROP[i]['λ'], G.DROP[i]['seed']) for i in blocks]
    x0, y = G.net_inputs(spec)
    layers = list(net.layers)
    num = lambda v: v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v, np.float64)
    vec = lambda v: np.broadcast_to(num(v), (len(x0),))

    def results(ref, mode):
        res = ref.forward(x0, y, mode, τ=spec['tau'])
        out = dict(c_err=np.stack([vec(res['out'][id(ℓ)]['c_err']) for ℓ in leaves]))
        if key != 'sr':
            out.update(p_ev=np.stack([vec(res['out'][id(ℓ)]['p_ev']) for ℓ in layers]), p_tr=np.stack([vec(res['out'][id(ℓ)]['p_tr']) for ℓ in layers]))
        return out

    def close(a, b):
        return a.shape == b.shape and np.abs(a - b).max() <= 1e-9 * (1 + np.abs(b).max())
    ours, literal = R.RefNetDropout(net), R.RefNetDropout(net)
    ours.step = literal.step = 0
    literal.literal = True
    for ref in (ours, literal):
        ref.load_params(vals)
    with np.load(GOLDEN) as gold:
        assert [n for n, _ in params] == list(gold['%s/names' % key])
        # 'tr': the layer as built is the reference's line (the same words drawn on both sides)
        for ref in (ours, literal):
            got = results(ref, 'tr')
            for k, v in got.items():
                assert (np.array_equal(v, gold['%s/tr/%s' % (key, k)]) if k == 'p_ev' else close(v, gold['%s/tr/%s' % (key, k)])), (k, ref.literal)
        # 'ev': the reference's line has no mode test and drops there too; the layer as built is the identity
        lit = results(literal, 'ev')
        assert all(close(v, gold['%s/ev/%s' % (key, k)]) for k, v in lit.items() if k != 'p_ev')
        got = results(ours, 'ev')
        assert not close(got['c_err'], gold['%s/ev/c_err' % key])
        # one training step with the step-0 masks: every variable (parameters after the TALR-scaled momentum update, averages)
        ours.train_step(x0, y, M.LR, τ=spec['tau'])
        after = np.array([M.digest(ours.V(p).detach().numpy()) for _, p in params])
        g = gold['%s/after' % key]
        err = np.abs(after - g) / (1e-12 + np.abs(g).max(0, keepdims=True))
        assert err.max() <= 1e-9, ([params[i][0] for i in np.argwhere(err > 1e-9)[:, 0][:5]], err.max())
    # ... and 'ev' of the layer as built gives the numbers of the same net without the layer, exactly
    import activity_error_ref as AR
    for ℓ in leaves:
        del ℓ.comps[1]
    plain = AR.RefNetActivity(net)
    plain.load_params(vals)
    want = results(plain, 'ev')
    assert all(np.array_equal(got[k], want[k]) for k in got)


# ------------------------------------------------------------------ the layer
@pytest.mark.parametrize('λ', [0.9, 0.5, 1e-3, 1.0])
def test_layer_and_backward_against_autograd(λ):
    rng = np.random.default_rng(3)
    n, K = 6, 37
    x, dxd, dx0 = rng.standard_normal((n, K)), rng.standard_normal((n, K)), rng.standard_normal((n, K))
    m = R.mask(7, 2, 1, n, K, 0.5 if λ == 1e-3 else λ)     # (at 1e-3 nothing of 222 elements would be kept: any mask serves)
    xt = torch.tensor(x, requires_grad=True)
    yt = xt * torch.tensor(m, dtype=torch.float64) / λ
    assert np.array_equal(R.layer(x, m, λ), yt.detach().numpy())
    yt.backward(torch.tensor(dxd))
    got, bound = R.layer_bwd(dxd, m, λ)
    assert np.array_equal(got, xt.grad.numpy()) and np.array_equal(bound, np.abs(dxd) / λ)
    got, bound = R.layer_bwd(dxd, m, λ, dx0)
    assert np.allclose(got, dx0 + xt.grad.numpy(), rtol=0, atol=1e-15) and np.array_equal(bound, np.abs(dx0) + np.abs(dxd) / λ)
    # the float32 stand-ins: within rounding of the float64 lines, dropped elements exact
    f = np.float32
    y32 = R.layer(x.astype(f), m, λ, f)
    assert y32.dtype == f and (y32.view(np.int32)[~m] == 0).all()
    assert np.abs(y32 - R.layer(x.astype(f).astype(np.float64), m, λ)).max() <= 2.0 ** -22 * np.abs(x).max() / λ
    d0 = dx0.astype(f)
    d0[0, 0] = -0.0
    g32, _ = R.layer_bwd(dxd.astype(f), m, λ, d0, f)
    assert g32.dtype == f and np.array_equal(g32.view(np.int32)[~m], d0.view(np.int32)[~m])
    g32, _ = R.layer_bwd(dxd.astype(f), m, λ, None, f)
    assert (g32.view(np.int32)[~m] == 0).all()
    assert R.inv_keep(λ).dtype == f and R.inv_keep(0.5) == 2.0


def test_kernel_cases_cover_the_sizes_the_issue_names():
    rows = {c[1] for c in R.KERNEL_CASES}
    maps = {(c[2], c[3]) for c in R.KERNEL_CASES}
    assert rows == {1, 5, 128, 130} and maps == {(16, 16), (16, 128), (4, 6), (1, 5), (3, 2), (6, 10)}
    assert {c[5] for c in R.KERNEL_CASES} == {1.0, 0.9, 0.5, 1e-3} and {c[4] for c in R.KERNEL_CASES} == {'batch', 'identity'}
    assert len(R.KERNEL_CASES) == 12 and sorted(n for t in R.KERNEL_TABLES for n in t) == sorted(R.CASE)
    assert {len(t) for t in R.KERNEL_TABLES} == {1, 2, 3}
    for t in R.KERNEL_TABLES:                               # different n, seeds and leaves inside a table
        assert len({R.CASE[n][6] for n in t}) == len(t)
    d = R.kernel_inputs('k5-tail')
    a, bound = R.activated(d)
    assert a.shape == bound.shape == (130, 5) and (a >= 0).all() and (bound >= np.abs(a) - 1e-12).all()
    assert 0.2 < (a > 0).mean() < 0.8                       # (the ReLU is live on both sides)


# ------------------------------------------------------------------ the layer on the host
def test_link_passes_x_through_and_validates():
    from lib.layer_types import Chain, Dropout, Sym
    for x in (Sym((10,)), Sym((4, 4, 16))):
        ℓ = Dropout(λ=0.5, seed=3)
        Chain(comps=[ℓ]).link(x, Sym((10,)), 'tr')
        assert ℓ.x is x and ℓ.c_err == 0.0 and ℓ.c_mod == 0.0 and ℓ.n_ops == 0 and vars(ℓ.params) == {} and ℓ.l2_terms == []
        assert ℓ.hypers.λ == 0.5 and ℓ.hypers.seed == 3
    assert vars(Dropout().hypers) == {'λ': 1, 'seed': 0}
    for λ in (0, 0.0, -0.5, 1.5, float('nan'), float('inf'), None, 'x', True):
        with pytest.raises(ValueError, match='Dropout'):
            Chain(comps=[Dropout(λ=λ)]).link(Sym((10,)), Sym((10,)), 'tr')
    for seed in (-1, 2 ** 64, 0.5, None, True):
        with pytest.raises(ValueError, match='Dropout'):
            Chain(comps=[Dropout(λ=0.5, seed=seed)]).link(Sym((10,)), Sym((10,)), 'tr')
    Chain(comps=[Dropout(λ=1e-3, seed=2 ** 64 - 1)]).link(Sym((10,)), Sym((10,)), 'tr')
    with pytest.raises(NotImplementedError, match='in front of its LinTrans'):
        Dropout(λ=0.5).link(Sym((10,)), Sym((10,)), 'tr')


POSITION = "once, directly in front of the head's LinTrans.*Select, \\[Dropout\\], LinTrans"


def test_reg_and_the_knobs_build_the_chains(monkeypatch):
    import arch_and_hypers as A
    from lib import _hip
    from lib._eng_common import _kind, head_activity, head_dropout, head_parts
    names = lambda ch: [type(c).__name__ for c in ch.comps]
    assert A.exit_dropout is None and A.dropout_seed == 0 and head_dropout(A.reg(10)) is None
    ch = A.reg(10, dropout=0.5, seed=7)
    assert names(ch) == ['Select', 'Dropout', 'LinTrans', 'Softmax', 'CrossEntropyError'] and _kind(ch) == 'head'
    assert head_dropout(ch) is ch.comps[1] and (ch.comps[1].hypers.λ, ch.comps[1].hypers.seed) == (0.5, 7)
    assert head_parts(ch)[0] is ch.comps[2] and head_parts(ch)[1] is ch.comps[-1] and head_parts(ch)[2] == _hip.LOSS_CE
    ch = A.reg(10, dropout=1)                                # λ = 1: in the chain, planned away
    assert names(ch)[1] == 'Dropout' and _kind(ch) == 'head' and head_dropout(ch) is None
    # all four error-layer shapes, with ActivityError at the other two positions
    ch = A.reg(10, loss='squared-linear', activity={'logits': -1}, dropout=0.9)
    assert names(ch) == ['Select', 'Dropout', 'LinTrans', 'ActivityError', 'SquaredError'] and _kind(ch) == 'head'
    assert head_activity(ch) == (0.0, -1.0, 0.0) and head_parts(ch)[2] == _hip.LOSS_SQ_LIN
    ch = A.reg(10, loss='squared', activity={'probs': 1, 'logits': 2}, dropout=0.9)
    assert names(ch) == ['Select', 'Dropout', 'LinTrans', 'ActivityError', 'Softmax', 'ActivityError', 'SquaredError']
    assert _kind(ch) == 'head' and head_activity(ch) == (0.0, 2.0, 1.0) and head_parts(ch)[2] == _hip.LOSS_SQ
    ch = A.reg(10, np.ones((10, 2), np.float32), dropout=0.9)
    assert names(ch) == ['Select', 'Dropout', 'LinTrans', 'Softmax', 'SuperclassCrossEntropyError'] and _kind(ch) == 'head'
    assert ch.comps[2].hypers.n_chan == 2
    for bad in (0, -1, 1.5, float('nan'), 'a', True, {'λ': 0.5}):
        with pytest.raises(ValueError, match='dropout'):
            A.reg(10, dropout=bad)
    with pytest.raises(ValueError, match="activity\\['map'\\]"):
        A.reg(10, activity={'map': 1e-3}, dropout=0.5)
    # the knobs: one λ for every exit, or {block index: λ}; the seed of every layer
    monkeypatch.setattr(A, 'arch', A.arch[:3])
    monkeypatch.setattr(A, 'exit_dropout', 0.5)
    monkeypatch.setattr(A, 'dropout_seed', 9)
    hyp = lambda net: [(d.hypers.λ, d.hypers.seed) if d is not None else None for d in (head_dropout(ℓ) for ℓ in net.leaves)]
    assert hyp(A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))) == [(0.5, 9)] * 3
    monkeypatch.setattr(A, 'exit_dropout', {0: 0.25, 2: 1.0})
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert hyp(net) == [(0.25, 9), None, None]
    assert [names(ℓ)[1] == 'Dropout' for ℓ in net.leaves] == [True, False, True]
    assert hyp(A.sr_chain(1)((32, 32, 3), (10,))) == [(0.25, 9)]


def test_the_flag_parser():
    import arch_and_hypers as A
    assert A.parse_exit_dropout('0.5') == 0.5 and A.parse_exit_dropout('1') == 1.0
    assert A.parse_exit_dropout('0.5:2') == {0: 0.5, 1: 0.5} and A.parse_exit_dropout('1e-3:0') == {}
    for bad in ('', '0', '-0.5', '1.5', 'nan', 'inf', 'a', '0.5:', '0.5:k', '0.5:-1', '0.5,0.6'):
        with pytest.raises(ValueError, match='--exit-dropout'):
            A.parse_exit_dropout(bad)


def test_every_other_position_is_refused(monkeypatch):
    import arch_and_hypers as A
    from lib._eng_common import _kind
    from lib._eng_structure import Structure
    from lib.layer_types import ActivityError, Dropout
    monkeypatch.setattr(A, 'arch', A.arch[:2])

    def at(k, ch):
        ch.comps.insert(k, Dropout(λ=0.5))
        return ch
    for k in (0, 2, 3, 4):                                  # in front of Select; behind the LinTrans, the Softmax, the error layer
        with pytest.raises(NotImplementedError, match=POSITION):
            _kind(at(k, A.reg(10)))
    with pytest.raises(NotImplementedError, match=POSITION):    # twice in one head
        _kind(at(1, A.reg(10, dropout=0.5)))
    for k in (1, 2):                                        # beside a 'map' ActivityError, on either side of it
        ch = A.reg(10, activity={'map': 1e-3})
        with pytest.raises(NotImplementedError, match=POSITION):
            _kind(at(k, ch))
    block = A.rcm(0)
    block.comps.append(Dropout(λ=0.5))                      # a block chain
    with pytest.raises(NotImplementedError, match=POSITION):
        _kind(block)
    pyr = A.pyr(A.rcm(0, A.reg(10)))
    pyr.comps.append(Dropout(λ=0.5))
    with pytest.raises(NotImplementedError, match=POSITION):
        _kind(pyr)
    # a router's chain: refused when the net's structure is classified
    real = A.router

    def router_with_dropout(n_sinks):
        r = real(n_sinks)
        if r is not None:
            r.comps.insert(1, Dropout(λ=0.5))
        return r
    monkeypatch.setattr(A, 'router', router_with_dropout)
    net = A.ac_chain(k_cpt=1e-9)((32, 32, 3), (10,))
    with pytest.raises(NotImplementedError, match=POSITION):
        Structure(net)
    monkeypatch.setattr(A, 'router', real)
    # λ out of range is a ValueError at link, wherever the layer stands
    monkeypatch.setattr(A, 'exit_dropout', None)
    real_reg = A.reg
    monkeypatch.setattr(A, 'reg', lambda *a, **k: _bad(real_reg(*a, **k)))
    with pytest.raises(ValueError, match='Dropout'):
        A.ac_chain(k_cpt=1e-9)((32, 32, 3), (10,))


def _bad(ch):
    from lib.layer_types import Dropout
    ch.comps.insert(1, Dropout(λ=1.5))
    return ch


def test_single_scale_conv_nets_refuse_the_layer():
    from lib._plan_conv import is_conv_net
    from lib.layer_types import Chain, Conv, CrossEntropyError, Dropout, GlobalMaxPool, LinTrans, Rect, Softmax
    from lib.net_types import SRNet

    def net(head_extra, root_extra):
        head = Chain(name='LogReg', comps=head_extra + [LinTrans(n_chan=10), Softmax(), CrossEntropyError()])
        root = Chain(name='Conv', sinks=[head], comps=[Conv(n_chan=16, supp=3), Rect()] + root_extra + [GlobalMaxPool()])
        return SRNet(x0_shape=(16, 16, 3), y_shape=(10,), root=root)
    assert is_conv_net(net([], []))
    for n in (net([Dropout(λ=0.5)], []), net([], [Dropout(λ=0.5)])):
        with pytest.raises(NotImplementedError, match=POSITION):
            is_conv_net(n)


def test_seed_per_net_and_per_rank():
    from lib._eng_common import DROPOUT_RANK_STRIDE, dropout_seed
    assert DROPOUT_RANK_STRIDE == R.RANK_STRIDE == 0x9E3779B97F4A7C15
    assert dropout_seed(3) == dropout_seed(3, 0) == 3
    for seed, rank in ((0, 1), (3, 2), (2 ** 64 - 1, 1), (2 ** 63, 7)):
        want = (seed + rank * 0x9E3779B97F4A7C15) % 2 ** 64
        assert dropout_seed(seed, rank) == R.rank_seed(seed, rank) == want and 0 <= want < 2 ** 64
    assert len({dropout_seed(5, r) for r in range(64)}) == 64
    # train-nets: net i of an experiment is built with --dropout-seed + i
    import importlib.machinery
    import importlib.util
    import types
    import arch_and_hypers as A
    path = os.path.join(os.path.dirname(HERE), 'multipath-nn_amd', 'train-nets')
    loader = importlib.machinery.SourceFileLoader('train_nets_for_test', path)
    mod = types.ModuleType(loader.name)
    mod.__file__ = path
    loader.exec_module(mod)
    keep = (A.exit_dropout, A.dropout_seed, A.arch)
    try:
        A.exit_dropout, A.arch = 0.5, A.arch[:2]
        mod.DROPOUT_SEED[0] = 3
        expt = types.SimpleNamespace(nets=[A.ac_chain(k_cpt=k) for k in A.k_cpts[:3]])
        ds = types.SimpleNamespace(x0_shape=(32, 32, 3), y_shape=(10,))
        for i in range(3):
            net = mod.build_net(expt, i, ds)
            assert [c.hypers.seed for ℓ in net.leaves for c in ℓ.comps if type(c).__name__ == 'Dropout'] == [3 + i] * 2
    finally:
        A.exit_dropout, A.dropout_seed, A.arch = keep


def test_record_fields_match_the_c_layout():
    import tempfile
    from lib import _hip
    root = os.path.dirname(HERE)
    fields = [f[0] for f in _hip.DropoutArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpnn_hip.h"', 'int main(void){']
    lines += ['printf("%%zu ", offsetof(mpnn_dropout_args, %s));' % f for f in fields]
    lines += ['printf("%zu ", sizeof(mpnn_dropout_args));', 'return 0;}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'a.c'), os.path.join(d, 'a.out')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), src, '-o', exe])
        v = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert v[:-1] == [getattr(_hip.DropoutArgs, f).offset for f in fields] and v[-1] == C.sizeof(_hip.DropoutArgs)
    lib = _hip.load()
    assert lib.mpnn_dropout_check(None) == _hip.E_ARG and lib.mpnn_dropout_check(C.byref(_hip.DropoutArgs())) == _hip.E_ARG
    assert lib.mpnn_dropout_fwd(None, 1, 1, 1, None) == _hip.E_ARG and lib.mpnn_dropout_bwd(None, 1, 1, 1, None) == _hip.E_ARG
    assert all(s in _hip.EXPORTS for s in ('mpnn_dropout_fwd', 'mpnn_dropout_bwd', 'mpnn_dropout_check'))


# ------------------------------------------------------------------ the exit planner on the host
class HostRing:
    """Stands in for the pinned upload rings (no GPU here; nothing is uploaded)."""
    def __init__(self, *a, **k):
        pass


def host_planner(net, monkeypatch):
    """Structure + Allocation + Planner over CPU tensors: everything Planner._exit_launches reads."""
    import lib._eng_alloc as EA
    from lib._eng_alloc import Allocation
    from lib._eng_ksteps import KStepGraphs
    from lib._eng_planner import Planner
    from lib._eng_structure import Structure
    monkeypatch.setattr(EA, 'ValueRing', HostRing)

    class Host(Structure, Allocation, Planner):
        STEPS_MAX = KStepGraphs.STEPS_MAX

        def __init__(self, net):
            Structure.__init__(self, net)
            self.dev = torch.device('cpu')
            self.multi_stream, self.bwd_levels, self.fuse_opt, self.co_share, self.fold_clear = False, True, True, 1, True
            self.dropout_rank = 0
            self._keep, self._progs, self._graphs, self._gen = [], {}, {}, 0
            self.n_max = self.n_max_bwd = 0
            self._stat_part = None
            self._alloc_params()

        def invalidate_packs(self):
            pass
    return Host(net)


def exit_lists(monkeypatch, ctor, dropout, n):
    import arch_and_hypers as A
    monkeypatch.setattr(A, 'exit_dropout', dropout)
    monkeypatch.setattr(A, 'dropout_seed', 2 ** 33 + 5)
    h = host_planner(ctor()((32, 32, 3), (10,)), monkeypatch)
    h._ensure_capacity(n, True)
    fwd, bwd, fold = h._exit_launches(n)
    return h, fwd, bwd


def record_fields(rec, base):
    """The scalar fields of a record, pointers as (buffer name, offset) of the net's own buffers where they are one."""
    out = {}
    for name, typ in rec._fields_:
        v = getattr(rec, name)
        if isinstance(v, C.Structure):
            out[name] = record_fields(v, base)
        elif isinstance(v, C.Array):
            out[name] = [base.get(x, 'ptr' if x else None) if isinstance(x, int) or x is None else x for x in v]
        else:
            out[name] = base.get(v, 'ptr' if v else None) if typ is C.c_void_p else v
    return out


@pytest.mark.parametrize('n', [5, 128, 1024])
def test_exit_planner_with_and_without_the_layer(monkeypatch, n):
    import arch_and_hypers as A
    from lib import _hip
    monkeypatch.setattr(A, 'arch', A.arch[:3])
    ctor = lambda: A.ac_chain(k_cpt=1e-9)
    kinds = lambda ops: [(op.what, len(op.host)) for op in ops]
    plain, pf, pb = exit_lists(monkeypatch, ctor, None, n)
    assert kinds(pf) == [('lin_fwd', 3), ('exit_tail_fwd', 3)] and kinds(pb) == [('exit_tail_bwd', 3), ('lin_bwd', 3)]
    assert not plain.has_dropout
    # λ = 1 on every exit: the layer is in the chains and nowhere in the program -- the same launches, the same entry points,
    # and records whose every field is the plain net's (pointers: the same buffer of the net, or both null)
    one, of, ob = exit_lists(monkeypatch, ctor, 1.0, n)
    assert all(type(ℓ.comps[1]).__name__ == 'Dropout' for ℓ in one.net.leaves) and not one.has_dropout
    assert kinds(of) == kinds(pf) and kinds(ob) == kinds(pb)
    for a, b in zip(of + ob, pf + pb):
        assert a.fn is b.fn and a.args[1:] == b.args[1:] and a.tag == b.tag
        for ra, rb in zip(a.host, b.host):
            names = lambda h: {getattr(blk, f).data_ptr(): (k, f) for k, blk in enumerate(h.blocks)
                               for f in ('z', 'dzh', 'dx', 'h1', 'dh1') if getattr(blk, f, None) is not None}
            assert record_fields(ra, names(one)) == record_fields(rb, names(plain))
    # the layer under blocks 0 and 2 (the last block has no router): two records of the new launches, the router of block 0
    # keeps a lin record of its own, block 1 is what it was
    drop, df, db = exit_lists(monkeypatch, ctor, {0: 0.5, 2: 0.25}, n)
    assert drop.has_dropout
    assert kinds(df) == [('dropout_fwd', 2), ('lin_fwd', 4), ('exit_tail_fwd', 3)]
    assert kinds(db) == [('exit_tail_bwd', 3), ('lin_bwd', 4), ('dropout_bwd', 2)]
    assert df[0].fn is drop.lib.mpnn_dropout_fwd and db[-1].fn is drop.lib.mpnn_dropout_bwd and df[0].host is db[-1].host
    b0, b1, b2 = drop.blocks
    d0, d2 = df[0].host
    seed = 2 ** 33 + 5
    for d, b, λ, acc in ((d0, b0, 0.5, 1), (d2, b2, 0.25, 0)):
        assert (d.a.x, d.a.mode, d.a.C, d.a.shift) == (b.s[-1].data_ptr(), _hip.ACT_BN_BATCH, b.C[-1], 0)
        assert (d.HW, d.n, d.leaf) == (b.H[-1] * b.W[-1], n, b.head.leaf_id)
        assert (d.seed_lo, d.seed_hi, d.thresh, d.inv_keep) == (seed & 0xffffffff, seed >> 32, R.thresh(λ), float(R.inv_keep(λ)))
        assert (d.step, d.xd, d.dxd, d.dx, d.accumulate) == (drop.drop_steps.data_ptr(), b.xd.data_ptr(), b.dxd.data_ptr(), b.dx.data_ptr(), acc)
        assert drop.lib.mpnn_dropout_check(C.byref(d)) == 0
    lf, lb = df[1].host, db[1].host
    # block 0: the router's record on the block's map, then the head's on xd; block 1: one shared record; block 2: the head's
    assert [(r.a.x, r.a.mode, bool(r.w[0]), bool(r.w[1])) for r in lf] == [
        (b0.s[-1].data_ptr(), _hip.ACT_BN_BATCH, False, True), (b0.xd.data_ptr(), _hip.ACT_IDENTITY, True, False),
        (b1.s[-1].data_ptr(), _hip.ACT_BN_BATCH, True, True), (b2.xd.data_ptr(), _hip.ACT_IDENTITY, True, False)]
    assert [(r.a.x, r.dx, r.dz_out, bool(r.w[0]), bool(r.w[1])) for r in lb] == [
        (b0.s[-1].data_ptr(), b0.dx.data_ptr(), None, False, True), (b0.xd.data_ptr(), b0.dxd.data_ptr(), None, True, False),
        (b1.s[-1].data_ptr(), b1.dx.data_ptr(), None, True, True), (b2.xd.data_ptr(), b2.dxd.data_ptr(), None, True, False)]
    # (the plain net's last block, without a child, has lin_bwd reduce its BatchNorm backward itself: dz_out set, dx null)
    assert pb[1].host[2].dz_out and not pb[1].host[2].dx
    for r_f, r_b in zip(lf, lb):
        assert (r_f.HW, r_f.n, r_f.a.C) == (r_b.HW, r_b.n, r_b.a.C) and r_f.n == n
    # every record with scratch has scratch of its own
    for field, recs in (('kpart', lf), ('kcnt', lf), ('kpart', lb), ('kcnt', lb)):
        ptrs = [getattr(r, field) for r in recs if getattr(r, field)]
        assert len(ptrs) == len(set(ptrs))
    assert (len([r for r in lb if r.kpart]) == 4) == (n <= 512)


def test_multi_stream_refusal_names_the_schedule(monkeypatch):
    import arch_and_hypers as A
    monkeypatch.setattr(A, 'arch', A.arch[:2])
    h, _, _ = exit_lists(monkeypatch, lambda: A.ac_chain(k_cpt=1e-9), 0.5, 5)
    h.multi_stream, h.allreduce, h.generic_convs = True, None, False
    h.group_fwd = True
    with pytest.raises(NotImplementedError, match='Dropout.*single-stream'):
        h._program('tr', 5, False)
