"""CPU: the float64 reference of SuperclassCrossEntropyError (tests/superclass_ref.py) and the host side of the layer.

  * golden vectors: tests/golden/superclass_ref_golden.npz, written by the reference's own SuperclassCrossEntropyError.link
    over the TensorFlow stand-in (tests/golden/superclass_ref_graph.py --emit), alone and inside a small actor net built from
    the reference's own classes, reproduced to float64 rounding by the literal lines and by RefNetSuper;
  * the GPU kernel test's tolerance can be met: an fp32 numpy model of the kernel's fold stays inside it on its soft
    inputs, and gives its exact cases exactly;
  * link (shapes, the map kept as float32 C-contiguous), the refusals, net.leaf_n_cls, `coarse_exits` (None leaves the
    constructors' nets as they are; read at call time), the checkpoint record, the kind of the head chain, the ConvEngine
    refusal.
"""
import os
import sys

import numpy as np
import pytest

import superclass_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'superclass_ref_golden.npz')
sys.path.insert(0, os.path.join(HERE, 'golden'))


def test_golden_vectors_of_the_reference_layer():
    import superclass_ref_graph as G
    assert os.path.getsize(GOLDEN) < 200 * 1024
    with np.load(GOLDEN) as gold:
        for key, case in G.LAYER_CASES.items():
            x, y = G.layer_input(case)
            c_err, d_cor, y_sup = R.layer(x, y, case['w'], case['hypers'].get('ϵ', 1e-6))
            g = gold['layer/%s/c_err' % key]
            assert c_err.shape == g.shape == (case['n'],)
            assert np.abs(c_err - g).max() <= 1e-13 * np.abs(g).max(), key
            assert np.array_equal(d_cor, gold['layer/%s/d_cor' % key]), key
            assert 0 < d_cor.sum() < case['n']                           # (both answers occur)
        # the tie case: the two largest outputs are equal in every row, and the first index decides
        x, y = G.layer_input(G.LAYER_CASES['tie3'])
        assert all(np.sort(r)[-1] == np.sort(r)[-2] for r in x)
        # the divisor is the width of y_sup, not the net's class count: with ϵ = 1e-3 (hard2) the two differ visibly
        case = G.LAYER_CASES['hard2']
        x, y = G.layer_input(case)
        wrong = -np.sum(R.label_map(y, case['w']) * np.log(1e-3 / 10 + (1 - 1e-3) * x), 1)
        assert np.abs(wrong - gold['layer/hard2/c_err']).max() > 1e-5


def _golden_net():
    import arch_and_hypers as A
    import lib.net_types as NT
    import superclass_ref_graph as G
    import make_ref_graph_golden as M
    from test_ref_graph_golden import ordered
    net = G.coarse_chain(A, NT)((32, 32, 3), (10,))
    rng = np.random.RandomState(G.NET['seed'])
    vals = {id(p): M.param_value(n, p.shape, rng) for n, p in ordered(net)}
    return G, net, vals


def test_refnet_super_reproduces_the_reference_net():
    G, net, vals = _golden_net()
    assert net.leaf_n_cls == [2, 5, 10]
    ref = R.RefNetSuper(net)
    ref.load_params(vals)
    x0, y = G.net_inputs()
    layers = list(net.layers)
    leaves = [ℓ for ℓ in layers if not ℓ.sinks]
    with np.load(GOLDEN) as gold:
        for mode in ('ev', 'tr'):
            res = ref.forward(x0, y, mode, τ=G.NET['tau'])
            Rr = lambda ℓ: res['out'][id(ℓ)]
            num = lambda v: v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v, np.float64)
            vec = lambda v: np.broadcast_to(num(v), (len(x0),))

            def close(a, b, what):
                assert a.shape == b.shape and np.abs(a - b).max() <= 1e-9 * (1 + np.abs(b).max()), (mode, what)
            assert np.array_equal(np.stack([vec(Rr(ℓ)['p_ev']) for ℓ in layers]), gold['net/%s/p_ev' % mode])
            close(np.stack([vec(Rr(ℓ)['p_tr']) for ℓ in layers]), gold['net/%s/p_tr' % mode], 'p_tr')
            close(np.stack([vec(Rr(ℓ)['c_err']) for ℓ in leaves]), gold['net/%s/c_err' % mode], 'c_err')
            assert np.array_equal(np.stack([vec(Rr(ℓ)['δ_cor']) for ℓ in leaves]), gold['net/%s/d_cor' % mode])
            p = 'p_tr' if mode == 'tr' else 'p_ev'
            cost = sum(vec(Rr(ℓ)[p]) * vec(Rr(ℓ)['c_err']) for ℓ in leaves)
            close(cost[None], gold['net/%s/cost' % mode], 'cost')


def test_refnet_super_agrees_with_the_literal_lines():
    import torch
    G, net, vals = _golden_net()
    ref = R.RefNetSuper(net)
    rng = np.random.default_rng(4)
    for ℓ in net.leaves:
        ce = ℓ.comps[-1]
        if type(ce).__name__ != 'SuperclassCrossEntropyError':
            continue
        w = ce.hypers.w_cls
        z = rng.standard_normal((7, w.shape[1]))
        x = np.exp(z) / np.exp(z).sum(1, keepdims=True)
        y = np.eye(10)[rng.integers(0, 10, 7)]
        out = {}
        ref._link(ce, torch.tensor(x), torch.tensor(y), 'ev', out)
        c_err, d_cor, _ = R.layer(x, y, w, ce.hypers.ϵ)
        assert np.abs(out[id(ce)]['c_err'].numpy() - c_err).max() <= 1e-13 * np.abs(c_err).max()
        assert np.array_equal(out[id(ce)]['δ_cor'].numpy(), d_cor)


# ------------------------------------------------------------------ the kernel's fold
@pytest.mark.parametrize('n_cls,n_sup', R.kernel_cases())
def test_fp32_model_of_the_fold_meets_the_kernel_tolerance(n_cls, n_sup):
    y, w = R.kernel_input('soft', n_cls, n_sup)
    ref, bnd = R.bound(y, w)
    got = R.model_fp32(y, w).astype(np.float64)
    assert (bnd > 0).all() and float((np.abs(got - ref) / bnd).max()) <= 1.0
    y, w = R.kernel_input('onehot', n_cls, n_sup)
    assert np.isfinite(w).all() and (w != 0).all() and ((y == 1).sum(1) == 1).all()
    assert np.array_equal(R.model_fp32(y, w), w[y.argmax(1)])
    y, w = R.kernel_input('dyadic', n_cls, n_sup)
    assert np.array_equal(R.model_fp32(y, w).astype(np.float64), R.label_map(y, w))


def test_the_maps_of_the_net_tests_keep_their_margin():
    for n_cls, n_sup in ((10, 2), (10, 5), (100, 20)):
        for w in (R.hard_map(n_cls, n_sup), R.soft_map(n_cls, n_sup)):
            assert w.dtype == np.float32 and np.array_equal(w.sum(1), np.ones(n_cls))
            top = np.sort(w, 1)                                  # y one-hot: y_sup is a row of the map
            assert (top[:, -1] - top[:, -2] >= 0.5).all()


# ------------------------------------------------------------------ the layer on the host
def _linked(w, n_in=None, y_shape=(10,)):
    from lib.layer_types import SuperclassCrossEntropyError, Sym
    ℓ = SuperclassCrossEntropyError(**({} if w is None else dict(w_cls=w)))
    ℓ.link(Sym((np.shape(w)[1] if n_in is None else n_in,)), Sym(y_shape), 'tr')
    return ℓ


def test_link_keeps_the_map_as_float32_c_contiguous():
    from lib.layer_types import Sym
    w64 = np.asfortranarray(R.soft_map(10, 5).astype(np.float64))
    ℓ = _linked(w64)
    w = ℓ.hypers.w_cls
    assert w.dtype == np.float32 and w.flags.c_contiguous and np.array_equal(w, w64)
    assert isinstance(ℓ.c_err, Sym) and isinstance(ℓ.δ_cor, Sym) and ℓ.c_err.producer is ℓ
    assert ℓ.n_ops == 0 and ℓ.c_mod == 0.0 and vars(ℓ.params) == {} and ℓ.hypers.ϵ == 1e-6
    assert _linked(R.hard_map(10, 2).tolist()).hypers.w_cls.shape == (10, 2)          # (a nested list is an array too)


def test_refusals():
    bad = R.hard_map(10, 2).copy()
    bad[3, 1] = np.nan
    inf = R.hard_map(10, 2).copy()
    inf[0, 0] = np.inf
    for w, n_in, y_shape in [(None, 2, (10,)),                             # no map
                             (np.ones(10), 1, (10,)), (np.ones((10, 2, 1)), 2, (10,)),      # not 2-D
                             (R.hard_map(9, 2), None, (10,)), (R.hard_map(11, 2), None, (10,)),      # rows != y_shape[0]
                             (R.hard_map(10, 2), 3, (10,)), (R.hard_map(10, 5), 10, (10,)),       # columns != the incoming width
                             (bad, None, (10,)), (inf, None, (10,)),       # non-finite
                             (np.ones((2000, 1025)), None, (2000,))]:      # more than 1 024 columns
        with pytest.raises(ValueError):
            _linked(w, n_in, y_shape)
    assert _linked(np.ones((2000, 1024)), None, (2000,)).hypers.w_cls.shape == (2000, 1024)


def test_kind_of_the_head_chain_and_leaf_n_cls(monkeypatch):
    import arch_and_hypers as A
    from lib._eng_common import _kind
    w2, w5 = R.hard_map(10, 2), R.soft_map(10, 5)
    monkeypatch.setattr(A, 'coarse_exits', {0: w2, 1: w2, 3: w5})
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert net.leaf_n_cls == [2, 2, 10, 5, 10, 10, 10, 10]
    assert all(_kind(ℓ) == 'head' for ℓ in net.leaves)
    names = [type(ℓ.comps[-1]).__name__ for ℓ in net.leaves]
    assert names == ['SuperclassCrossEntropyError'] * 2 + ['CrossEntropyError', 'SuperclassCrossEntropyError'] + ['CrossEntropyError'] * 4
    assert [ℓ.comps[1].hypers.n_chan for ℓ in net.leaves] == net.leaf_n_cls
    tree = A.ac_tree(k_cpt=1e-9)((32, 32, 3), (10,))
    widths = tree.leaf_n_cls
    assert len(widths) == 47 and sorted(set(widths)) == [2, 5, 10] and widths.count(5) == 8
    monkeypatch.setattr(A, 'coarse_exits', {1: w2})
    assert A.sr_chain(2)((32, 32, 3), (10,)).leaf_n_cls == [2]
    assert A.sr_chain(3)((32, 32, 3), (10,)).leaf_n_cls == [10]          # (its one head is under block 2)
    assert A.reg(10, w5).comps[1].hypers.n_chan == 5 and A.reg(10).comps[1].hypers.n_chan == 10


def test_coarse_exits_none_leaves_the_constructors_nets_as_they_are(monkeypatch):
    import arch_and_hypers as A
    assert A.coarse_exits is None
    sig = lambda net: [(type(ℓ).__name__, ℓ.name, [type(c).__name__ for c in ℓ.comps], sorted(vars(ℓ.hypers)), ℓ.n_ops)
                       for ℓ in net.layers]
    prm = lambda net: [(p.name, p.shape, p.init[0], p.l2) for p in net._all_params]
    makers = [A.sr_chain(2), A.ac_chain(k_cpt=1.6e-8), A.cr_chain(k_cpt=8e-9), A.ac_tree(), A.cr_tree()]
    plain = [mk((32, 32, 3), (10,)) for mk in makers]
    for net in plain:
        assert all(type(ℓ.comps[-1]).__name__ == 'CrossEntropyError' for ℓ in net.leaves)
        assert net.leaf_n_cls == [10] * len(list(net.leaves))
    # ... the knob is read when a constructor is CALLED; with a map for no block of the net, nothing changes either
    monkeypatch.setattr(A, 'coarse_exits', {99: R.hard_map(10, 2)})
    for mk, a in zip(makers, plain):
        b = mk((32, 32, 3), (10,))
        assert sig(a) == sig(b) and prm(a) == prm(b)
    monkeypatch.setattr(A, 'coarse_exits', {0: R.hard_map(10, 2)})
    coarse = makers[1]((32, 32, 3), (10,))
    assert coarse.leaf_n_cls == [2] + [10] * 7
    assert [p.shape for p in coarse._all_params] != [p.shape for p in plain[1]._all_params]


def test_checkpoint_record_round_trips_the_map(monkeypatch):
    """encode_layer / decode_layer (lib/serdes.py; encode_net / decode_net wrap them around an engine, which needs a GPU:
    tests/test_superclass_nets.py): the map travels as an ndarray among the hypers, through np.save too, and the rebuilt
    tree links."""
    import arch_and_hypers as A
    from lib import serdes
    from lib.net_types import ActorNet
    monkeypatch.setattr(A, 'coarse_exits', {0: R.soft_map(10, 2), 2: R.hard_map(10, 5)})
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))

    def strip(ℓ):
        """encode_layer without parameter values (they live on the device)."""
        if ℓ is None:
            return None
        return dict(type=type(ℓ).__name__, name=ℓ.name, hypers=dict(vars(ℓ.hypers)), params={}, router=strip(ℓ.router),
                    sinks=[strip(s) for s in ℓ.sinks], comps=[strip(c) for c in ℓ.comps])
    rec = strip(net.root)
    import io
    buf = io.BytesIO()
    np.save(buf, rec)
    buf.seek(0)
    rec = np.load(buf, allow_pickle=True)[()]
    back = ActorNet(x0_shape=(32, 32, 3), y_shape=(10,), root=serdes.decode_layer(rec), k_cpt=1.6e-8)
    assert back.leaf_n_cls == net.leaf_n_cls == [2, 10, 5, 10, 10, 10, 10, 10]
    for a, b in zip(net.leaves, back.leaves):
        assert type(a.comps[-1]) is type(b.comps[-1]) and sorted(vars(a.comps[-1].hypers)) == sorted(vars(b.comps[-1].hypers))
        if hasattr(a.comps[-1].hypers, 'w_cls'):
            w = b.comps[-1].hypers.w_cls
            assert w.dtype == np.float32 and np.array_equal(w, a.comps[-1].hypers.w_cls)


def test_single_scale_conv_nets_refuse_the_layer():
    from lib.layer_types import Chain, Conv, LinTrans, Rect, Softmax, SuperclassCrossEntropyError
    from lib.net_types import SRNet
    from lib._plan_conv import is_conv_net
    head = Chain(comps=[LinTrans(n_chan=2), Softmax(), SuperclassCrossEntropyError(w_cls=R.hard_map(10, 2))])
    net = SRNet(x0_shape=(8, 8, 3), y_shape=(10,), root=Chain(comps=[Conv(n_chan=16, supp=3), Rect()], sinks=[head]))
    with pytest.raises(NotImplementedError, match='single-scale Conv'):
        is_conv_net(net)
