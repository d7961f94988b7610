"""GPU: whole nets with MultiscaleLLN behind ToPyramid (arch_and_hypers.lln) -- sr_chain(2) and ac_chain(k_cpt=1.6e-8) on
32x32x3 (the tuned conv kernels) and on 24x40x3 (the general ones), n = 5, positive images (the normalisation is then
well conditioned).

  * oracle parity: one training step and one evaluation against RefNetLLN (tests/lln_ref.py) in float64, with
    tests/test_net_parity.py's run_case -- its decision-forced comparison, its tolerances, its flip cap;
  * the evaluation paths agree as they do without the layer: dense, routed, predict (tests/test_predict_nets.py);
  * K-step replay: run_steps with K = 4 equals 4 single steps bit for bit;
  * input pipeline: a step through the bound pipeline equals the array-fed step on the same batch bit for bit;
  * predict_all from uint8 with decode='unit' equals predict on the decoded floats;
  * co-training: a CoTrainer of 2 LLN nets equals their solo steps under the same co_share (tests/test_cotrain.py);
  * a checkpoint written by write_net and read back predicts the same bits.
"""
import numpy as np
import pytest
import torch

import lln_ref as R
import test_net_parity
from test_cotrain import _compare_with_solo_steps, _nets
from test_net_parity import perturb_routers, run_case
from test_rect_nets import _batch, spec            # noqa: F401  (spec: the fixture that hands run_case batches of a shape)

pytestmark = pytest.mark.gpu

N = 5
SHAPES = {'32x32': (32, 32, 3), '24x40': (24, 40, 3)}


def ctor(A, kind):
    return A.sr_chain(2) if kind == 'sr2' else A.ac_chain(k_cpt=1.6e-8)


def feeds_of(A, kind):
    return (lambda net, t: {}) if kind == 'sr2' else (lambda net, t: {net.τ: A.τ_ds(t * 5000)})


def lln_net(A, kind, shape, seed=1234):
    net = ctor(A, kind)(shape, (10,))
    net.engine().init_params(seed)
    if net._net_kind != 'sr':
        perturb_routers(net)
    return net


def has_lln_launch(eng, mode, n, **kw):
    return [op.what for op in eng.program(mode, n, **kw)['fwd']].count('lln') == 1


# ------------------------------------------------------------------ parity with the float64 oracle
@pytest.mark.parametrize('kind,shape,lln', [('sr2', '32x32', {}), ('ac', '32x32', {}), ('sr2', '24x40', {}), ('ac', '24x40', {}),
                                            ('ac', '32x32', {'σ': 1.5}), ('ac', '24x40', {'σ': 1.5})])
def test_oracle_parity(spec, monkeypatch, kind, shape, lln):
    from oracle import ref_net
    shape = SHAPES[shape]
    A, wrap = spec(shape)
    monkeypatch.setattr(A, 'lln', lln)
    monkeypatch.setattr(ref_net, 'RefNet', R.RefNetLLN)          # (run_case imports it when it is called)
    seen = []

    def make(x0_shape, y_shape):
        net = wrap(ctor(A, kind))(x0_shape, y_shape)
        seen.append(net)
        return net
    run_case(make, N, feeds_of(A, kind), steps=1)
    net, = seen
    eng = net.engine()
    assert [type(c).__name__ for c in net.root.comps] == ['ToPyramid', 'MultiscaleLLN']
    assert eng.generic_convs == (shape != (32, 32, 3))
    assert has_lln_launch(eng, 'tr', N) and has_lln_launch(eng, 'ev', N)
    # the layer's x through the inspection path: the normalised scales of the last run (run_case's evaluation batch),
    # at the kernel's own tolerance (tests/test_lln_kernel.py)
    x0, _ = test_net_parity.batch(N, seed=99)
    ℓ = net.root.comps[1]
    ref, bnd = R.bound(x0, len(ℓ.x), ℓ.hypers.σ, ℓ.hypers.ϵ, False)
    for sym, r, b in zip(ℓ.x, ref, bnd):
        got = sym.buf.cpu().numpy().astype(np.float64)
        assert got.shape == r.shape and (np.abs(got - r) <= b).all()


# ------------------------------------------------------------------ the evaluation paths
@pytest.mark.parametrize('shape', ['32x32', '24x40'])
def test_dense_routed_and_predict_agree(monkeypatch, shape):
    import arch_and_hypers as A
    from test_predict_nets import _calibrated, check_consistent
    shape = SHAPES[shape]
    monkeypatch.setattr(A, 'lln', {})
    net = lln_net(A, 'ac', shape)
    x0, y = _batch(shape, N, seed=3)
    for t in range(2):                                     # (moving averages away from their initial values)
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    _calibrated(net, x0, y)                                # one image leaves at each of the first five exits
    dense = check_consistent(net, x0, y, modes=(True, 1, 3, 'auto'), every_leaf=False, min_leaves=4)
    assert sorted(dense['leaf'].tolist()) == [0, 1, 2, 3, 4]
    eng = net.engine()
    for mode, kw in (('ev', {}), ('ev', dict(routed=1)), ('pr', {}), ('pr', dict(routed=3)), ('pr+p', {})):
        assert has_lln_launch(eng, mode, N, **kw), (mode, kw)


# ------------------------------------------------------------------ K-step replay
@pytest.mark.parametrize('shape', ['32x32', '24x40'])
def test_k_step_replay_equals_single_steps(monkeypatch, shape):
    import arch_and_hypers as A
    shape = SHAPES[shape]
    monkeypatch.setattr(A, 'lln', {})
    nets = [lln_net(A, 'ac', shape) for _ in range(2)]
    K = 4
    x0, y = (torch.from_numpy(v).cuda() for v in _batch(shape, N, seed=3))
    engs = [net.engine() for net in nets]
    for e in engs:
        e.ensure_capacity(N)
        e.x0[:N].copy_(x0); e.y[:N].copy_(y)

    def feed(net, t):
        e = net.engine()
        return {net.x0: e.x0[:N], net.y: e.y[:N], net.mode: 'tr', net.λ_lrn: 0.05 / (1 + 0.3 * t), net.τ: 1.0 / (1 + 0.1 * t)}
    a, b = nets
    for call in range(3):                                  # single steps | capture | replay
        ts = range(call * K, (call + 1) * K)
        a.train.run_steps([feed(a, t) for t in ts])
        for t in ts:
            b.train.run(feed(b, t))
        torch.cuda.synchronize()
        for u, v in zip(engs[0].lln_out, engs[1].lln_out):
            assert torch.equal(u, v)
        assert torch.equal(engs[0].P, engs[1].P) and torch.equal(engs[0].A, engs[1].A) and torch.equal(engs[0].S, engs[1].S), call
        for la, lb in zip(a.layers, b.layers):
            assert torch.equal(la.p_ev, lb.p_ev) and torch.equal(la.p_tr, lb.p_tr)
    assert any(k[0] == 'trK' and not isinstance(v, str) for k, v in engs[0]._graphs.items())


# ------------------------------------------------------------------ the input pipeline
def test_bound_input_pipeline_equals_the_array_fed_step(monkeypatch):
    import arch_and_hypers as A
    from lib.data import Dataset
    from test_cotrain import _copy_state
    monkeypatch.setattr(A, 'lln', {})
    ds = Dataset.synthetic(n_tr=60, n_ts=20, seed=1)
    a, b = (lln_net(A, 'ac', tuple(ds.x0_shape)) for _ in range(2))
    ea, eb = a.engine(), b.engine()
    np.random.seed(3)
    x0, y = ds.bind_engine(ea, N)
    seen = []
    for t in range(4):                                     # eager | capture | replays: every form reads the step's own batch
        _copy_state(a, b)
        ds.stage_training_draws(N, eng=ea)
        a.train.run({a.x0: x0, a.y: y, a.mode: 'tr', a.λ_lrn: 0.05, a.τ: 1.0})
        torch.cuda.synchronize()
        xb, yb = ea.x0[:N].cpu().numpy().copy(), ea.y[:N].cpu().numpy().copy()
        seen.append(xb)
        b.train.run({b.x0: xb, b.y: yb, b.mode: 'tr', b.λ_lrn: 0.05, b.τ: 1.0})
        torch.cuda.synchronize()
        for u, v in zip(ea.lln_out, eb.lln_out):
            assert torch.equal(u[:N], v[:N]), t
        assert torch.equal(ea.P, eb.P) and torch.equal(ea.A, eb.A) and torch.equal(ea.S, eb.S), t
        ref = R.lln(xb, 4)[0]                              # ... and it is this step's batch that was normalised
        assert np.abs(ea.lln_out[0][:N].cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
    assert all(np.abs(u - v).max() > 0 for u, v in zip(seen, seen[1:]))


# ------------------------------------------------------------------ 8-bit images, streamed
def test_predict_all_from_uint8_equals_predict_on_the_decoded_floats(monkeypatch):
    import arch_and_hypers as A
    from lib.decode import decode_table
    from test_predict_nets import host
    monkeypatch.setattr(A, 'lln', {})
    net = lln_net(A, 'ac', (32, 32, 3))
    rng = np.random.default_rng(5)
    x8 = rng.integers(0, 256, (3 * N + 2, 32, 32, 3), dtype=np.uint8)
    xf = decode_table('unit')[x8]
    want = []
    for i in range(0, len(x8), N):
        want.append(host(net.predict(xf[i:i + N], probs=True)))
    got = host(net.predict_all(x8, batch=N, probs=True, decode='unit'))
    for k in got:
        assert np.array_equal(got[k], np.concatenate([w[k] for w in want])), k
    one = host(net.predict(x8[:N], probs=True, decode='unit'))
    for k in one:
        assert np.array_equal(one[k], want[0][k]), k


# ------------------------------------------------------------------ co-training
def test_cotrained_lln_nets_equal_their_solo_steps(monkeypatch):
    import arch_and_hypers as A
    from lib._co import CoTrainer
    monkeypatch.setattr(A, 'lln', {})
    mk = lambda i: A.ac_chain(k_cpt=A.k_cpts[i + 1])
    co_nets, solo = _nets([mk(i) for i in range(2)]), _nets([mk(i) for i in range(2)])
    co = CoTrainer(co_nets)
    _compare_with_solo_steps(co_nets, solo, co.run, 2, N)
    merged = [op for op in co._program(N)['ops'] if op.what == 'lln']
    assert len(merged) == 1 and len(merged[0].host) == 2          # one launch, the two nets' records
    for a, b in zip(co_nets, solo):
        for u, v in zip(a.engine().lln_out, b.engine().lln_out):
            assert torch.equal(u, v)


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_predicts_the_same_bits(monkeypatch, tmp_path):
    import arch_and_hypers as A
    from lib.serdes import read_net, write_net
    from test_predict_nets import host
    monkeypatch.setattr(A, 'lln', {'σ': 1.5, 'ϵ': 0.01})
    net = lln_net(A, 'ac', (32, 32, 3))
    x0, y = _batch((32, 32, 3), N, seed=3)
    net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    want = host(net.predict(x0, probs=True))
    path = str(tmp_path / 'net.npy')
    write_net(path, net)
    monkeypatch.setattr(A, 'lln', None)                    # (the file alone says what the net is)
    back = read_net(path)
    ℓ = back.root.comps[1]
    assert type(ℓ).__name__ == 'MultiscaleLLN' and ℓ.hypers.σ == 1.5 and ℓ.hypers.ϵ == 0.01
    got = host(back.predict(x0, probs=True))
    for k in want:
        assert np.array_equal(got[k], want[k]), k
