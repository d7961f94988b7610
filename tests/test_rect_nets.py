"""GPU: whole nets on rectangular images and on maps of any size -- 24x24, 24x40, 16x64, 28x28 (a three-scale table),
48x48, 8x16 (coarsest map 1x2) -- which run ALL their multiscale convs on the any-map entry points of the general kernels
(csrc/conv_gen.hip: mpnn_msconv_*_hw; lib/_eng_alloc.py picks them once per net), and a 32x32 net forced onto them
(MPNN_ANYMAP_CONVS=1).

Parity: tests/test_net_parity.py's run_case at its own TOL and its own decision-flip cap (teacher-forced steps against
the decision-forced float64 oracle, the free-run check included).  run_case builds square images from `hw`: here its
`batch` is replaced by one of the case's shape, and the net constructor is wrapped to be given that shape.
oracle/ref_net.conv_same pads every axis by (kh - 1) / 2, which is TensorFlow's SAME only for odd, square filters; filters
clipped to a small map (3x5 with conv_supp = 5, 1x2 on the 1x2 map) need SAME per axis, so this module replaces it the
way tests/test_conv_gen_nets.py does (for odd square filters the two are the same function).

Behaviour on the 24x40 conv_supp = 5 actor chain: routed evaluation equals dense evaluation, K training steps in one
hipGraph equal K single steps, seeded runs repeat.  Refusals: a 30x30 image under a four-scale pyramid, the multi-stream
schedule.  The train-nets driver on 24x40 synthetic images."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import test_net_parity
from test_net_parity import perturb_routers, run_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH3 = [3 * [16], 3 * [16], 2 * [32], 2 * [32]]       # a three-scale table: 28x28 -> 28, 14, 7


def _tf_same(x, w):                        # tf.nn.conv2d(x, w, (1, 1, 1, 1), 'SAME') for any kh x kw
    kh, kw = w.shape[0], w.shape[1]
    pt, pl = (kh - 1) // 2, (kw - 1) // 2
    xp = TF.pad(x.permute(0, 3, 1, 2), (pl, kw - 1 - pl, pt, kh - 1 - pt))
    return TF.conv2d(xp, w.permute(3, 2, 0, 1)).permute(0, 2, 3, 1)


def _batch(shape, n, n_cls=10, seed=0):
    rng = np.random.default_rng(seed)
    x0 = rng.random((n,) + tuple(shape)).astype(np.float32)
    y = np.eye(n_cls, dtype=np.float32)[rng.integers(0, n_cls, n)]
    return x0, y


@pytest.fixture
def spec(monkeypatch):
    """spec(shape, supp=3, arch=None, forced=False) -> (the arch_and_hypers module with conv_supp = supp and the table
    `arch`, wrap) with the oracle on TF SAME padding and run_case's batches of `shape`; wrap(ctor) is the net constructor
    run_case is handed (it builds the net on `shape` whatever square shape run_case asks for)."""
    def make(shape, supp=3, arch=None, forced=False):
        import arch_and_hypers as A
        from oracle import ref_net
        monkeypatch.setattr(A, 'conv_supp', supp)
        if arch is not None:
            monkeypatch.setattr(A, 'arch', arch)           # (the constructors read it when they are called)
        monkeypatch.setattr(ref_net, 'conv_same', _tf_same)
        monkeypatch.setattr(test_net_parity, 'batch',
                            lambda n, c0=3, n_cls=10, seed=0, hw=32: _batch(shape, n, n_cls, seed))
        if forced:
            monkeypatch.setenv('MPNN_ANYMAP_CONVS', '1')
        return A, (lambda ctor: (lambda x0_shape, y_shape: ctor(tuple(shape), y_shape)))
    return make


def _maps(net):
    return [(h, w) for b in net.engine().blocks for h, w in zip(b.H, b.W)]


def _filters(net):
    return sorted({tuple(p.shape[:2]) for p in net._all_params if p.name.startswith(('w_horz', 'w_vert'))})


def _on_hw(net):
    eng = net.engine()
    return eng.anymap_convs and eng.generic_convs


# ------------------------------------------------------------------ parity with the float64 oracle
def test_a_24x24_ac_chain(spec):
    A, wrap = spec((24, 24, 3))
    net = A.ac_chain(k_cpt=1.6e-8)((24, 24, 3), (10,))
    assert _on_hw(net) and set(_maps(net)) == {(24, 24), (12, 12), (6, 6), (3, 3)} and _filters(net) == [(3, 3)]
    run_case(wrap(A.ac_chain(k_cpt=1.6e-8)), 16, lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def test_b_24x40_sr_chain_3(spec):
    A, wrap = spec((24, 40, 3))
    net = A.sr_chain(3)((24, 40, 3), (10,))
    assert _on_hw(net) and set(_maps(net)) == {(24, 40), (12, 20), (6, 10), (3, 5)}
    run_case(wrap(A.sr_chain(3)), 8, lambda net, t: {})


def test_c_16x64_cr_chain(spec):
    A, wrap = spec((16, 64, 3))
    net = A.cr_chain(k_cpt=1e-9)((16, 64, 3), (10,))
    assert _on_hw(net) and set(_maps(net)) == {(16, 64), (8, 32), (4, 16), (2, 8)}
    run_case(wrap(A.cr_chain(k_cpt=1e-9)), 16, lambda net, t: {net.τ: 0.1})


def test_d_28x28x1_sr_chain_on_a_three_scale_table(spec):
    A, wrap = spec((28, 28, 1), arch=ARCH3)
    net = A.sr_chain(4)((28, 28, 1), (10,))
    assert _on_hw(net) and set(_maps(net)) == {(28, 28), (14, 14), (7, 7)}
    run_case(wrap(A.sr_chain(4)), 8, lambda net, t: {}, c0=1)


def test_e_24x40_ac_chain_supp_5(spec):
    A, wrap = spec((24, 40, 3), supp=5)
    net = A.ac_chain(k_cpt=1.6e-8)((24, 40, 3), (10,))
    assert _on_hw(net) and {(3, 5), (5, 5)} <= set(_filters(net))          # horizontal filters clipped to the 3x5 maps
    run_case(wrap(A.ac_chain(k_cpt=1.6e-8)), 16, lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def test_f_8x16_ac_chain_coarsest_map_1x2(spec):
    A, wrap = spec((8, 16, 3))
    net = A.ac_chain(k_cpt=1.6e-8)((8, 16, 3), (10,))
    assert _on_hw(net) and (1, 2) in _maps(net) and (1, 2) in _filters(net)
    run_case(wrap(A.ac_chain(k_cpt=1.6e-8)), 16, lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def test_g_24x40_ac_chain_kcpt0_batch_128(spec):
    A, wrap = spec((24, 40, 3))
    run_case(wrap(A.ac_chain(k_cpt=0.0)), 128, lambda net, t: {net.τ: A.τ_ds(0)}, steps=1)


def test_h_48x48_sr_chain_4(spec):
    A, wrap = spec((48, 48, 3))
    net = A.sr_chain(4)((48, 48, 3), (10,))
    assert _on_hw(net) and set(_maps(net)) == {(48, 48), (24, 24), (12, 12), (6, 6)}      # 12x12 and 6x6 are pooled maps too
    run_case(wrap(A.sr_chain(4)), 8, lambda net, t: {})


def test_i_32x32_ac_chain_forced_onto_the_any_map_entry_points(spec):
    A, wrap = spec((32, 32, 3), forced=True)
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert _on_hw(net) and _filters(net) == [(3, 3)]
    run_case(wrap(A.ac_chain(k_cpt=1.6e-8)), 16, lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def test_dispatch_is_decided_per_net(spec, monkeypatch):
    """Tuned launches where every map and filter is theirs, the general entry points where every map is theirs, the
    any-map entry points otherwise."""
    A, _ = spec((32, 32, 3))
    flags = lambda net: (net.engine().generic_convs, net.engine().anymap_convs)
    assert flags(A.sr_chain(3)((32, 32, 3), (10,))) == (False, False)
    assert flags(A.sr_chain(3)((64, 64, 3), (10,))) == (False, False)
    assert flags(A.sr_chain(3)((24, 24, 3), (10,))) == (True, True)
    assert flags(A.sr_chain(3)((32, 64, 3), (10,))) == (True, True)
    monkeypatch.setattr(A, 'conv_supp', 5)
    assert flags(A.sr_chain(3)((32, 32, 3), (10,))) == (True, False)
    assert flags(A.sr_chain(3)((24, 40, 3), (10,))) == (True, True)


# ------------------------------------------------------------------ refusals
def test_image_that_is_no_multiple_of_the_pyramid_step_is_refused(spec):
    A, _ = spec((30, 30, 3))
    for shape in [(30, 30, 3), (24, 30, 3), (30, 24, 3), (36, 36, 3)]:
        net = A.sr_chain(3)(shape, (10,))
        with pytest.raises(NotImplementedError, match=r'pyramid of 4 scales .* multiples of 8 .* %dx%d image' % shape[:2]):
            net.engine()


def test_multi_stream_schedule_refuses(spec, monkeypatch):
    A, _ = spec((24, 40, 3))
    monkeypatch.setenv('MPNN_STREAMS', '1')
    net = A.ac_chain(k_cpt=1.6e-8)((24, 40, 3), (10,))
    x0, y = _batch((24, 40, 3), 8)
    with pytest.raises(NotImplementedError, match='multi-stream'):
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})


# ------------------------------------------------------------------ behaviour of the 24x40 conv_supp = 5 actor chain
SHAPE = (24, 40, 3)


def _net5(A, seed=1234):
    net = A.ac_chain(k_cpt=1.6e-8, seed=7)(SHAPE, (10,))
    net.engine().init_params(seed)
    perturb_routers(net)
    return net


def test_routed_evaluation_equals_dense(spec):
    from test_routed_eval import check_routed_equals_dense
    A, _ = spec(SHAPE, supp=5)
    net = _net5(A)
    x0, y = _batch(SHAPE, 64, seed=3)
    for t in range(2):                                     # (moving averages away from their initial values)
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    check_routed_equals_dense(net, x0, y)


def test_k_steps_in_one_graph_equal_single_steps(spec):
    A, _ = spec(SHAPE, supp=5)
    nets = [_net5(A) for _ in range(2)]
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
    """Two nets from the same seed through the same steps: the same parameters.  The weight gradients come out of the
    slabs in a fixed order (no fp32 atomics on the conv path); only the fp64-atomic BatchNorm sums can round differently."""
    A, _ = spec(SHAPE, supp=5)
    nets = [_net5(A) for _ in range(2)]
    for t in range(3):
        x0, y = _batch(SHAPE, 32, seed=t)
        for net in nets:
            net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    torch.cuda.synchronize()
    e0, e1 = (net.engine() for net in nets)
    for u, v in ((e0.P, e1.P), (e0.A, e1.A), (e0.S, e1.S)):
        assert float((u - v).abs().max()) <= 1e-6 * float(v.abs().max())
    # one step from identical state, twice: forward sums bit-identical
    P0, A0, S0 = e0.P.clone(), e0.A.clone(), e0.S.clone()
    x0, y = _batch(SHAPE, 32, seed=9)
    outs = []
    for _ in range(2):
        e0.P.copy_(P0); e0.A.copy_(A0); e0.S.copy_(S0)
        nets[0].train.run({nets[0].x0: x0, nets[0].y: y, nets[0].mode: 'tr', nets[0].λ_lrn: 0.05, nets[0].τ: 1.0})
        torch.cuda.synchronize()
        outs.append([s.clone() for b in e0.blocks for s in b.s])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------ the driver
def test_train_nets_cli_on_24x40_synthetic_images(tmp_path):
    out = str(tmp_path / 'nets')
    cmd = [sys.executable, os.path.join(ROOT, 'multipath-nn_amd', 'train-nets'), 'cifar10-ac', '--synthetic',
           '--synthetic-shape', '24', '40', '--iters', '8', '--log-every', '4', '--nets', '0', '--out', out]
    res = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    base = os.path.join(out, 'cifar10-ac')
    for f in ('0000.npy', '0000-stats.npy', '0000-log.txt', '0000-stats/00000004.npy', '0000-stats/00000008.npy'):
        assert os.path.exists(os.path.join(base, f)), f
    desc = np.load(os.path.join(base, '0000-stats.npy'), allow_pickle=True)[()]
    assert desc['type'] == 'ActorNet' and 0 <= desc['stats_ts']['acc'] <= 1
