"""GPU: whole nets on the general conv kernels (csrc/conv_gen.hip) -- `conv_supp` other than 3 in the spec file
(arch_and_hypers.py), or MPNN_GENERIC_CONVS=1 on a 3x3 net.

Parity: tests/test_net_parity.py's run_case (teacher-forced steps against the decision-forced float64 oracle, the
free-run check included).  oracle/ref_net.conv_same pads symmetrically, which is TensorFlow's SAME only for odd filters;
with conv_supp = 5 the 4x4 maps get CLIPPED 4x4 horizontal filters, so this module replaces it by TF SAME padding (pad
(k - 1) / 2 before and the rest after, then a convolution without padding).

Behaviour on a conv_supp = 5 actor chain: routed evaluation equals dense evaluation, K training steps in one hipGraph
equal K single steps, runs are repeatable, and co-training (CoGroups: an architecture without the table-driven launch
forms runs as groups of one) equals each net's solo steps."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from test_net_parity import perturb_routers, run_case

pytestmark = pytest.mark.gpu


def _tf_same(x, w):                        # tf.nn.conv2d(x, w, (1, 1, 1, 1), 'SAME') for any kh x kw
    kh, kw = w.shape[0], w.shape[1]
    pt, pl = (kh - 1) // 2, (kw - 1) // 2
    xp = TF.pad(x.permute(0, 3, 1, 2), (pl, kw - 1 - pl, pt, kh - 1 - pt))
    return TF.conv2d(xp, w.permute(3, 2, 0, 1)).permute(0, 2, 3, 1)


@pytest.fixture
def spec(monkeypatch):
    """spec(supp, forced=False) -> the arch_and_hypers module with conv_supp = supp (and the oracle on TF SAME padding)."""
    def make(supp, forced=False):
        import arch_and_hypers as A
        from oracle import ref_net
        monkeypatch.setattr(A, 'conv_supp', supp)
        monkeypatch.setattr(ref_net, 'conv_same', _tf_same)
        if forced:
            monkeypatch.setenv('MPNN_GENERIC_CONVS', '1')
        return A
    return make


def _shapes(net):
    return sorted({tuple(p.shape[:2]) for p in net._all_params if p.name.startswith(('w_horz', 'w_vert'))})


def test_oracle_padding_patch_is_tf_same():
    """The replacement conv_same equals oracle/np_ops.conv_same (TF SAME, asymmetric for even sizes)."""
    from oracle import np_ops as O
    rng = np.random.default_rng(0)
    for k in (1, 2, 4, 5):
        x, w = rng.standard_normal((2, 4, 4, 3)), rng.standard_normal((k, k, 3, 5))
        got = _tf_same(torch.from_numpy(x), torch.from_numpy(w)).numpy()
        assert np.allclose(got, O.conv_same(x, w), atol=1e-12)


@pytest.mark.parametrize('supp', [1, 5])
def test_sr_chain_3(spec, supp):
    A = spec(supp)
    net = A.sr_chain(3)((32, 32, 3), (10,))
    assert net.engine().generic_convs and (supp, supp) in _shapes(net)
    run_case(A.sr_chain(3), 8, lambda net, t: {})


@pytest.mark.parametrize('supp', [1, 5])
def test_ac_chain(spec, supp):
    A = spec(supp)
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert net.engine().generic_convs
    if supp == 5:
        assert {(4, 4), (5, 5)} <= set(_shapes(net))        # clipped horizontal filters on the 4x4 maps
    run_case(A.ac_chain(k_cpt=1.6e-8), 16, lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def test_cr_chain_supp5_batch_128(spec):
    A = spec(5)
    run_case(A.cr_chain(k_cpt=1e-9), 128, lambda net, t: {net.τ: 0.1}, steps=1)


def test_ac_chain_3x3_forced_general(spec):
    A = spec(3, forced=True)
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert net.engine().generic_convs and _shapes(net) == [(3, 3)]
    run_case(A.ac_chain(k_cpt=1.6e-8), 16, lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def test_multi_stream_schedule_refuses(spec, monkeypatch):
    A = spec(5)
    monkeypatch.setenv('MPNN_STREAMS', '1')
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    rng = np.random.default_rng(0)
    x0 = rng.random((8, 32, 32, 3)).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 8)]
    with pytest.raises(NotImplementedError, match='multi-stream'):
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})


# ------------------------------------------------------------------ behaviour of a conv_supp = 5 actor chain
def _net5(A, seed=1234):
    net = A.ac_chain(k_cpt=1.6e-8, seed=7)((32, 32, 3), (10,))
    net.engine().init_params(seed)
    perturb_routers(net)
    return net


def test_routed_evaluation_equals_dense(spec):
    from test_routed_eval import batch, check_routed_equals_dense
    A = spec(5)
    net = _net5(A)
    x0, y = batch(64, seed=3)
    for t in range(2):                                     # (moving averages away from their initial values)
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    check_routed_equals_dense(net, x0, y)


def test_k_steps_in_one_graph_equal_single_steps(spec):
    A = spec(5)
    nets = [_net5(A) for _ in range(2)]
    n, K = 32, 4
    rng = np.random.default_rng(3)
    x0 = torch.from_numpy(rng.random((n, 32, 32, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]).cuda()
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
    """Two nets from the same seed through the same steps: the same parameters.  The weight gradients come out of the
    slabs in a fixed order (no fp32 atomics on the conv path); only the fp64-atomic BatchNorm sums can round differently."""
    from test_net_parity import batch
    A = spec(5)
    nets = [_net5(A) for _ in range(2)]
    for t in range(3):
        x0, y = batch(32, 3, 10, seed=t)
        for net in nets:
            net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    torch.cuda.synchronize()
    e0, e1 = (net.engine() for net in nets)
    for u, v in ((e0.P, e1.P), (e0.A, e1.A), (e0.S, e1.S)):
        assert float((u - v).abs().max()) <= 1e-6 * float(v.abs().max())
    # one step from identical state, twice: forward sums bit-identical
    P0, A0, S0 = e0.P.clone(), e0.A.clone(), e0.S.clone()
    x0, y = batch(32, 3, 10, seed=9)
    outs = []
    for _ in range(2):
        e0.P.copy_(P0); e0.A.copy_(A0); e0.S.copy_(S0)
        nets[0].train.run({nets[0].x0: x0, nets[0].y: y, nets[0].mode: 'tr', nets[0].λ_lrn: 0.05, nets[0].τ: 1.0})
        torch.cuda.synchronize()
        outs.append([s.clone() for b in e0.blocks for s in b.s])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_cotraining_groups_of_one_equal_solo_steps(spec):
    from test_cotrain import _compare_with_solo_steps, _nets
    from lib._co import CoGroups
    A = spec(5)
    mk = lambda: [A.ac_chain(k_cpt=A.k_cpts[i]) for i in range(2)]
    co_nets, solo = _nets(mk()), _nets(mk())
    cg = CoGroups.plan(co_nets, streams=2)
    assert [c.K for c in cg.groups] == [1, 1]

    def run(feeds):
        cg.run(feeds)
        cg.join()
    _compare_with_solo_steps(co_nets, solo, run, cg.share, 16, steps=3)
