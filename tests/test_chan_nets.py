"""GPU: whole nets whose channel counts are no multiples of 16, on the any-channel conv entry points (csrc/conv_gen_ch.hip:
mpnn_msconv_*_ch) -- the `arch` table of the spec file (arch_and_hypers.py) replaced by tables such as [8, 12, 20] /
[24, 40] / [10] and [4, 6] / [7], on images of 2, 3, 4 and 5 channels.  Their exits sit on maps such as 4x4x20 and 4x4x10
(K = 160, a multiple of 16 with C = 10) and run on the any-width exit kernels.

Parity: tests/test_net_parity.py's run_case at its own TOL and its own decision-flip cap (teacher-forced steps against
the decision-forced float64 oracle, the free-run check included), on the three nets of
tests/golden/chan_ref_graph_golden.npz (where the oracle itself is held to the reference's graph code) and on the odd
table over 12x20 images; the shipped actor chain under MPNN_ANYCHAN_CONVS=1 is the cross-check of the new family against
the tuned one.

Behaviour on the odd-table actor chain over 16x16x2 images: routed evaluation equals dense evaluation, predict agrees with
eval and its routed form with its dense form, K training steps in one hipGraph equal K single steps, runs are repeatable,
co-training runs as groups of one that equal the solo steps, a checkpoint restores the net."""
import os
import sys

import numpy as np
import pytest
import torch

import test_net_parity
from test_net_parity import perturb_routers, run_case

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from chan_ref_graph import NARROW, ODD

pytestmark = pytest.mark.gpu


def _batch(shape, n, n_cls=10, seed=0):
    rng = np.random.default_rng(seed)
    x0 = rng.random((n,) + tuple(shape)).astype(np.float32)
    y = np.eye(n_cls, dtype=np.float32)[rng.integers(0, n_cls, n)]
    return x0, y


@pytest.fixture
def spec(monkeypatch):
    """spec(arch=None, forced=False) -> the arch_and_hypers module with the table `arch` (the constructors read it when
    they are called); forced: MPNN_ANYCHAN_CONVS=1."""
    def make(arch=None, forced=False):
        import arch_and_hypers as A
        if arch is not None:
            monkeypatch.setattr(A, 'arch', arch)
        if forced:
            monkeypatch.setenv('MPNN_ANYCHAN_CONVS', '1')
        return A
    return make


def _on_ch(net, exits=True):
    eng = net.engine()
    return eng.anychan_convs and eng.anymap_convs and eng.generic_convs and (eng.generic_exits or not exits)


# ------------------------------------------------------------------ parity with the float64 oracle
def test_ac_odd_16x16x2(spec):
    A = spec(ODD)
    net = A.ac_chain(k_cpt=1.6e-8)((16, 16, 2), (10,))
    assert _on_ch(net) and [b.C for b in net.engine().blocks] == ODD
    run_case(A.ac_chain(k_cpt=1.6e-8), 16, lambda net, t: {net.τ: 0.7}, c0=2, hw=16)


def test_cr_odd_16x16x4(spec):
    A = spec(ODD)
    assert _on_ch(A.cr_chain(k_cpt=4e-9)((16, 16, 4), (10,)))
    run_case(A.cr_chain(k_cpt=4e-9), 16, lambda net, t: {net.τ: 0.9}, c0=4, hw=16)


def test_sr_narrow_8x8x5(spec):
    A = spec(NARROW)
    net = A.sr_chain(3)((8, 8, 5), (10,))
    assert _on_ch(net) and [b.C for b in net.engine().blocks] == NARROW
    run_case(A.sr_chain(3), 8, lambda net, t: {}, c0=5, hw=8)


def test_ac_odd_12x20x3(spec, monkeypatch):
    """The odd table on a rectangular image: maps of 12x20, 6x10 and 3x5 (overhanging tiles and channel tails together)."""
    A = spec(ODD)
    shape = (12, 20, 3)
    monkeypatch.setattr(test_net_parity, 'batch', lambda n, c0=3, n_cls=10, seed=0, hw=32: _batch(shape, n, n_cls, seed))
    ctor = A.ac_chain(k_cpt=1.6e-8)
    net = ctor(shape, (10,))
    assert _on_ch(net) and {(h, w) for b in net.engine().blocks for h, w in zip(b.H, b.W)} == {(12, 20), (6, 10), (3, 5)}
    run_case(lambda x0_shape, y_shape: ctor(shape, y_shape), 16, lambda net, t: {net.τ: 0.7})


def test_shipped_ac_chain_forced_onto_the_any_channel_entry_points(spec):
    A = spec(forced=True)
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert _on_ch(net, exits=False)
    run_case(A.ac_chain(k_cpt=1.6e-8), 16, lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def test_dispatch_is_decided_per_net(spec):
    A = spec()
    flags = lambda net: (net.engine().generic_convs, net.engine().anymap_convs, net.engine().anychan_convs)
    assert flags(A.sr_chain(3)((32, 32, 3), (10,))) == (False, False, False)
    assert flags(A.sr_chain(3)((32, 32, 1), (10,))) == (False, False, False)
    assert flags(A.sr_chain(3)((24, 24, 3), (10,))) == (True, True, False)
    assert flags(A.sr_chain(3)((32, 32, 2), (10,))) == (True, True, True)          # the image's channels count
    A = spec(ODD)
    assert flags(A.sr_chain(3)((16, 16, 3), (10,))) == (True, True, True)


def test_a_600_channel_block_is_refused(spec):
    A = spec([[16, 16, 600], [16, 16, 32]])
    net = A.sr_chain(2)((16, 16, 3), (10,))
    with pytest.raises(NotImplementedError, match=r'600 channels.*1\.\.512 channels'):
        net.engine()


# ------------------------------------------------------------------ behaviour of the odd-table actor chain
SHAPE = (16, 16, 2)


def _net(A, seed=1234):
    net = A.ac_chain(k_cpt=1.6e-8, seed=7)(SHAPE, (10,))
    net.engine().init_params(seed)
    perturb_routers(net)
    return net


def _trained(A, n=64):
    net = _net(A)
    x0, y = _batch(SHAPE, n, seed=3)
    for t in range(2):                                     # (moving averages away from their initial values)
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    return net, x0, y


def test_routed_evaluation_equals_dense(spec):
    from test_routed_eval import calibrate_exit_fractions, check_routed_equals_dense
    net, x0, y = _trained(spec(ODD))
    calibrate_exit_fractions(net, x0, y, [1 / 6] * 5)
    dense = check_routed_equals_dense(net, x0, y)
    hist = np.stack([dense['p_ev'][nd.idx] for nd in net.engine().leaves]).mean(1)
    assert (hist > 0).all(), hist                          # (every block below the root ran on a proper sample list)


def test_predict_agrees_with_eval_and_routed_with_dense(spec):
    """tests/test_predict_nets.py's check_consistent: cls == arg-max y exactly where d_cor at the chosen leaf says so, leaf
    and cost from the labelled evaluation, and predict(routed=...) equal to predict(routed=False) bit for bit."""
    from test_predict_nets import check_consistent
    from test_routed_eval import calibrate_exit_fractions
    net, x0, y = _trained(spec(ODD), n=96)
    calibrate_exit_fractions(net, x0, y, [1 / 6] * 5)
    dense = check_consistent(net, x0, y, modes=(True, 1, 3))
    assert np.array_equal(np.bincount(dense['leaf'], minlength=6), [16] * 6)
    # predict_all, 40 images per launch: the concatenation of predict over the chunks
    res = net.predict_all(x0, batch=40, routed=1, probs=True)
    torch.cuda.synchronize()
    for k in ('cls', 'leaf', 'ops', 'conf', 'probs'):
        assert np.array_equal(getattr(res, k).cpu().numpy(), dense[k]), k


def test_k_steps_in_one_graph_equal_single_steps(spec):
    A = spec(ODD)
    nets = [_net(A) for _ in range(2)]
    n, K = 32, 4
    x0, y = (torch.from_numpy(v).cuda() for v in _batch(SHAPE, n, seed=3))
    engs = [net.engine() for net in nets]
    for e in engs:
        e._ensure_capacity(n)
        e.x0[:n].copy_(x0); e.y[:n].copy_(y)

    def feed(net, t):
        e = net.engine()
        return {net.x0: e.x0[:n], net.y: e.y[:n], net.mode: 'tr', net.λ_lrn: 0.05 / (1 + 0.3 * t), net.τ: 1.0 / (1 + 0.1 * t)}
    a, b = nets
    rel = lambda u, v: float((u - v).abs().max() / v.abs().max())
    for call in range(3):
        ts = range(call * K, (call + 1) * K)
        a.train.run_steps([feed(a, t) for t in ts])
        for t in ts:
            b.train.run(feed(b, t))
        torch.cuda.synchronize()
        # (the same launches on the same data: only the fp64-atomic BatchNorm statistics may round differently)
        assert rel(engs[0].P, engs[1].P) <= 1e-6 and rel(engs[0].A, engs[1].A) <= 1e-6 and rel(engs[0].S, engs[1].S) <= 1e-6
        for la, lb in zip(a.layers, b.layers):
            assert torch.equal(la.p_ev, lb.p_ev) and torch.allclose(la.p_tr, lb.p_tr, rtol=1e-5, atol=1e-8)
    assert any(k[0] == 'trK' and not isinstance(v, str) for k, v in engs[0]._graphs.items())


def test_seeded_runs_are_repeatable(spec):
    A = spec(ODD)
    nets = [_net(A) for _ in range(2)]
    for t in range(3):
        x0, y = _batch(SHAPE, 32, seed=t)
        for net in nets:
            net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    torch.cuda.synchronize()
    e0, e1 = (net.engine() for net in nets)
    for u, v in ((e0.P, e1.P), (e0.A, e1.A), (e0.S, e1.S)):
        assert float((u - v).abs().max()) <= 1e-6 * float(v.abs().max())


def test_cotraining_groups_of_one_equal_solo_steps(spec, monkeypatch):
    import test_cotrain
    from test_cotrain import _compare_with_solo_steps, _nets
    from lib._co import CoGroups
    A = spec(ODD)
    monkeypatch.setattr(test_cotrain, 'batch', lambda n, seed=0: _batch(SHAPE, n, seed=seed))
    on_shape = lambda ctor: (lambda x0_shape, y_shape: ctor(SHAPE, y_shape))
    mk = lambda: [on_shape(A.ac_chain(k_cpt=A.k_cpts[i])) for i in range(2)]
    co_nets, solo = _nets(mk()), _nets(mk())
    assert all(_on_ch(net) for net in co_nets)
    cg = CoGroups.plan(co_nets, streams=2)
    assert [c.K for c in cg.groups] == [1, 1]

    def run(feeds):
        cg.run(feeds)
        cg.join()
    _compare_with_solo_steps(co_nets, solo, run, cg.share, 16, steps=3)


def test_checkpoint_round_trip(spec, tmp_path):
    """write_net / read_net: the restored net has the same parameters, momentum and BatchNorm state, runs on the
    any-channel entry points again and takes the same next training step, bit for bit."""
    from lib.serdes import write_net, read_net
    net, x0, y = _trained(spec(ODD), n=12)
    feed = lambda m: {m.x0: x0, m.y: y, m.mode: 'tr', m.λ_lrn: 0.05, m.τ: 0.6}
    path = str(tmp_path / 'net.npy')
    write_net(path, net, with_optimizer=True)
    net2 = read_net(path)
    assert type(net2) is type(net) and _on_ch(net2)
    for p, q in zip(net._all_params, net2._all_params):
        assert (p.name, p.shape) == (q.name, q.shape) and torch.equal(p.data.cpu(), q.data.cpu()), (p.owner.name, p.name)
        if p.trainable:
            assert torch.equal(p.accum.cpu(), q.accum.cpu()), (p.owner.name, p.name)
    net.train.run(feed(net)); net2.train.run(feed(net2))
    torch.cuda.synchronize()
    assert float((net.engine().P - net2.engine().P).abs().max()) == 0.0
    st, st2 = net.state(), net2.state()                     # (the statistics of the step just taken)
    assert all(torch.equal(v.cpu(), w.cpu()) for v, w in zip(st.values(), st2.values()))
