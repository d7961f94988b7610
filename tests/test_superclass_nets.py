"""GPU: whole nets whose early exits classify superclasses (arch_and_hypers.coarse_exits -> SuperclassCrossEntropyError), 5
images per batch:

  (a) ac_chain(k_cpt=1.6e-8) on 32x32x3, 10 classes: the exits of blocks 0-2 on a 10>2 map, those of blocks 3-4 on a 10>5
      map, the rest fine -- two records, the tuned exit kernels;
  (b) the same on 24x40x3 (the general convs);
  (c) 100 classes, a 100>20 map on the exits of blocks 0-2 (the any-width exits: generic_exits);
  (d) sr_chain(2) whose only head is coarse;  (e) cr_chain with the maps of (a);  (f) (a) with the soft maps (0.75 / 0.25).

  * oracle parity: one training step and one evaluation against RefNetSuper (tests/superclass_ref.py) in float64, with
    tests/test_net_parity.py's run_case -- its decision-forced comparison, its tolerances, its flip cap, its batches.  The
    maps put no near-tie into a decision: one-hot y_sup has a unique maximum, the soft maps keep a 0.75 / 0.25 margin;
  * launch counts: one 'label_map' launch in 'tr' and 'ev' (dense and routed), none in 'pr' / 'pr+p', one record per
    distinct map;
  * the evaluation paths agree as tests/test_predict_nets.py's check_consistent demands (dense, routed at depths 1, 3 and
    'auto', predict with NaN labels, eval -> predict -> eval), with `cls` read in the label space of the exit taken:
    cls < leaf_n_cls[leaf], probs zero beyond the leaf's width and summing to 1 within it, δ_cor == (cls == argmax y_sup);
  * K-step replay equals single steps, the bound input pipeline equals the array-fed step, two co-trained nets equal
    their solo steps, a checkpoint read back predicts the same bits;
  * nets without the layer: every program is launch for launch what a net built without consulting the knob gets.
"""
import numpy as np
import pytest
import torch

import superclass_ref as R
import test_net_parity
from test_cotrain import _compare_with_solo_steps, _nets
from test_net_parity import perturb_routers, run_case
from test_rect_nets import _batch, spec            # noqa: F401  (spec: the fixture that hands run_case batches of a shape)

pytestmark = pytest.mark.gpu

N = 5
SHAPES = {'32x32': (32, 32, 3), '24x40': (24, 40, 3)}


def maps_of(case):
    """The `coarse_exits` dict of a case."""
    if case == 'c':
        return {i: R.hard_map(100, 20) for i in range(3)}
    if case == 'd':
        return {1: R.hard_map(10, 2)}
    mk = R.soft_map if case == 'f' else R.hard_map
    return {**{i: mk(10, 2) for i in range(3)}, **{i: mk(10, 5) for i in (3, 4)}}


# case -> (constructor, image shape, classes, feeds of run_case, distinct maps, leaf widths)
def case_of(A, case):
    ac = lambda: A.ac_chain(k_cpt=1.6e-8)
    τ_ds = lambda net, t: {net.τ: A.τ_ds(t * 5000)}
    return {
        'a': (ac, '32x32', 10, τ_ds, 2, [2, 2, 2, 5, 5, 10, 10, 10]),
        'b': (ac, '24x40', 10, τ_ds, 2, [2, 2, 2, 5, 5, 10, 10, 10]),
        'c': (ac, '32x32', 100, τ_ds, 1, [20, 20, 20, 100, 100, 100, 100, 100]),
        'd': (lambda: A.sr_chain(2), '32x32', 10, lambda net, t: {}, 1, [2]),
        'e': (lambda: A.cr_chain(k_cpt=8e-9), '32x32', 10, lambda net, t: {net.τ: A.τ_cr(t * 5000)}, 2, [2, 2, 2, 5, 5, 10, 10, 10]),
        'f': (ac, '32x32', 10, τ_ds, 2, [2, 2, 2, 5, 5, 10, 10, 10]),
    }[case]


def super_net(A, monkeypatch, case='a', seed=1234):
    ctor, shape, n_cls, _, _, widths = case_of(A, case)
    monkeypatch.setattr(A, 'coarse_exits', maps_of(case))
    net = ctor()(SHAPES[shape], (n_cls,))
    assert net.leaf_n_cls == widths
    net.engine().init_params(seed)
    if net._net_kind != 'sr':
        perturb_routers(net)
    return net


def whats(eng, mode, n, **kw):
    p = eng.program(mode, n, **kw)
    return [op.what for op in list(p['fwd']) + list(p['bwd'])]


def leaf_maps(net):
    """Per leaf: its map [n_cls, width] (the identity for a fine exit)."""
    n_cls = net.hypers.y_shape[0]
    return [np.asarray(ℓ.comps[-1].hypers.w_cls, np.float64) if type(ℓ.comps[-1]).__name__ == 'SuperclassCrossEntropyError'
            else np.eye(n_cls) for ℓ in net.leaves]


# ------------------------------------------------------------------ parity with the float64 oracle
@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd', 'e', 'f'])
def test_oracle_parity(spec, monkeypatch, case):
    from oracle import ref_net
    import arch_and_hypers as A0
    ctor, shape, n_cls, feeds, n_maps, widths = case_of(A0, case)
    A, wrap = spec(SHAPES[shape])
    monkeypatch.setattr(A, 'coarse_exits', maps_of(case))
    monkeypatch.setattr(ref_net, 'RefNet', R.RefNetSuper)          # (run_case imports it when it is called)
    seen = []

    def make(x0_shape, y_shape):
        net = wrap(ctor())(x0_shape, y_shape)
        seen.append(net)
        return net
    run_case(make, N, feeds, steps=1, n_cls=n_cls)
    net, = seen
    eng = net.engine()
    assert net.leaf_n_cls == widths == eng.leaf_n_cls
    assert eng.generic_convs == (shape != '32x32') and eng.generic_exits == (case == 'c')
    # launch counts: one 'label_map' launch where there are labels, one record per distinct map
    routed = [{}] if net._net_kind == 'sr' else [{}, dict(routed=1), dict(routed=3)]
    for mode, kw in [('tr', {})] + [('ev', kw) for kw in routed]:
        ops = [op for op in eng.program(mode, N, **kw)['fwd'] if op.what == 'label_map']
        assert len(ops) == 1 and len(ops[0].host) == n_maps == len(eng.label_maps), (mode, kw)
        assert eng.program(mode, N, **kw)['fwd'][0].what == 'label_map'
    for mode, kw in [(m, kw) for m in ('pr', 'pr+p') for kw in routed]:
        assert 'label_map' not in whats(eng, mode, N, **kw), (mode, kw)
    # y_sup of the last run (run_case's evaluation batch): exactly y @ w_cls for these maps (every term 0 or dyadic)
    _, y = test_net_parity.batch(N, 3, n_cls, seed=99)
    for w, y_sup in zip(eng.label_maps, eng.y_sup):
        assert np.array_equal(y_sup[:N].cpu().numpy().astype(np.float64), R.label_map(y, w))


# ------------------------------------------------------------------ the evaluation paths
def check_consistent_super(net, x0, y, modes, min_leaves):
    """tests/test_predict_nets.py's check_consistent, with `cls` read in the label space of the exit taken."""
    from test_predict_nets import KEYS, predict_poisoned, same_snapshot
    from test_routed_eval import snapshot
    eng = net.engine()
    feed = {net.x0: x0, net.y: y}
    n = len(x0)
    net.eval(feed)
    torch.cuda.synchronize()
    first = snapshot(net)
    acc = net.state()[(net, 'acc')].cpu().numpy()
    pev = np.stack([first['p_ev'][nd.idx] for nd in eng.nodes])
    leaf_rows = pev[[nd.idx for nd in eng.leaves]]
    assert ((leaf_rows == 1).sum(0) == 1).all()
    want_leaf = leaf_rows.argmax(0)
    assert len(set(want_leaf.tolist())) >= min_leaves, np.bincount(want_leaf, minlength=len(eng.leaves))
    want_ops = (pev.astype(np.float64) * np.array(eng.node_ops_host, np.float64)[:, None]).sum(0)
    widths = np.array(net.leaf_n_cls)
    y_sup = [R.label_map(y, w) for w in leaf_maps(net)]              # per leaf [n, width]
    want_cls = np.array([y_sup[l][i].argmax() for i, l in enumerate(want_leaf)])
    d_cor = np.stack([first['d_cor'][nd.idx] for nd in eng.leaves])[want_leaf, np.arange(n)]

    dense = predict_poisoned(net, x0, routed=False, probs=True)
    assert np.array_equal(dense['leaf'], want_leaf)
    assert (dense['cls'] >= 0).all() and (dense['cls'] < widths[dense['leaf']]).all()
    assert np.array_equal(dense['cls'] == want_cls, d_cor == 1) and set(np.unique(d_cor)) <= {0.0, 1.0}
    assert np.array_equal(d_cor, acc)                              # (acc: δ_cor of the exit taken)
    assert dense['ops'].dtype == np.int64 and np.array_equal(dense['ops'].astype(np.float64), want_ops)
    assert dense['cls'].dtype == np.int32 and dense['leaf'].dtype == np.int32
    ar = np.arange(n)
    assert dense['probs'].shape == (n, widths.max())
    assert np.array_equal(dense['conf'], dense['probs'][ar, dense['cls']])
    assert np.array_equal(dense['probs'].argmax(1), dense['cls'])
    beyond = np.arange(widths.max())[None, :] >= widths[dense['leaf']][:, None]
    assert (dense['probs'][beyond] == 0).all()                     # zero beyond the leaf's width ...
    assert np.abs(np.where(beyond, 0, dense['probs']).astype(np.float64).sum(1) - 1).max() < 1e-5       # ... 1 within it
    with pytest.raises(RuntimeError, match='predict'):
        net.state()
    assert net.predict(x0, routed=False).probs is None
    for mode in modes:
        got = predict_poisoned(net, x0, routed=mode, probs=True)
        for k in KEYS:
            assert np.array_equal(got[k], dense[k]), (mode, k)
    net.eval(feed)
    torch.cuda.synchronize()
    same_snapshot(first, snapshot(net))
    return dense


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'f'])
def test_dense_routed_and_predict_agree(monkeypatch, case):
    import arch_and_hypers as A
    from test_predict_nets import _calibrated
    _, shape, n_cls, _, _, _ = case_of(A, case)
    net = super_net(A, monkeypatch, case)
    x0, y = _batch(SHAPES[shape], N, n_cls, seed=3)
    for t in range(2):                                     # (moving averages away from their initial values)
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    _calibrated(net, x0, y)                                # one image leaves at each of the first five exits: 2, 2, 2, 5, 5 wide
    dense = check_consistent_super(net, x0, y, modes=(True, 1, 3, 'auto'), min_leaves=4)
    assert sorted(dense['leaf'].tolist()) == [0, 1, 2, 3, 4]
    # a larger batch regrows the buffers: the rows are zero beyond each leaf's width there too
    eng = net.engine()
    x1, _ = _batch(SHAPES[shape], 3 * N, n_cls, seed=4)
    res = net.predict(x1, probs=True)
    torch.cuda.synchronize()
    leaf, probs = res.leaf.cpu().numpy(), res.probs.cpu().numpy()
    widths = np.array(net.leaf_n_cls)
    assert eng.n_max >= 3 * N and (probs[np.arange(widths.max())[None, :] >= widths[leaf][:, None]] == 0).all()


def test_sr_chain_with_a_coarse_head_predicts_superclasses(monkeypatch):
    import arch_and_hypers as A
    from test_predict_nets import predict_poisoned
    net = super_net(A, monkeypatch, 'd')
    x0, y = _batch((32, 32, 3), N, seed=3)
    net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05})
    net.eval({net.x0: x0, net.y: y})
    acc = net.state()[(net, 'acc')].cpu().numpy()
    want = R.label_map(y, R.hard_map(10, 2)).argmax(1)
    for routed in (False, True, 'auto'):
        got = predict_poisoned(net, x0, routed=routed, probs=True)
        assert got['probs'].shape == (N, 2) and (got['cls'] < 2).all() and (got['leaf'] == 0).all()
        assert np.array_equal(got['cls'] == want, acc == 1)


# ------------------------------------------------------------------ K-step replay
def test_k_step_replay_equals_single_steps(monkeypatch):
    import arch_and_hypers as A
    shape = (32, 32, 3)
    nets = [super_net(A, monkeypatch, 'a') for _ in range(2)]
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
        for w, u, v in zip(engs[0].label_maps, engs[0].y_sup, engs[1].y_sup):
            assert torch.equal(u, v) and np.array_equal(u[:N].cpu().numpy(), R.label_map(y.cpu().numpy(), w))
        assert torch.equal(engs[0].P, engs[1].P) and torch.equal(engs[0].A, engs[1].A) and torch.equal(engs[0].S, engs[1].S), call
        for la, lb in zip(a.layers, b.layers):
            assert torch.equal(la.p_ev, lb.p_ev) and torch.equal(la.p_tr, lb.p_tr)
    assert any(k[0] == 'trK' and not isinstance(v, str) for k, v in engs[0]._graphs.items())


# ------------------------------------------------------------------ the input pipeline
def test_bound_input_pipeline_equals_the_array_fed_step(monkeypatch):
    import arch_and_hypers as A
    from lib.data import Dataset
    from test_cotrain import _copy_state
    ds = Dataset.synthetic(n_tr=60, n_ts=20, seed=1)
    a, b = (super_net(A, monkeypatch, 'a') for _ in range(2))
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
        seen.append(yb)
        b.train.run({b.x0: xb, b.y: yb, b.mode: 'tr', b.λ_lrn: 0.05, b.τ: 1.0})
        torch.cuda.synchronize()
        for w, u, v in zip(ea.label_maps, ea.y_sup, eb.y_sup):
            assert torch.equal(u[:N], v[:N]), t
            assert np.array_equal(u[:N].cpu().numpy(), R.label_map(yb, w)), t        # ... of THIS step's labels
        assert torch.equal(ea.P, eb.P) and torch.equal(ea.A, eb.A) and torch.equal(ea.S, eb.S), t
    assert any(np.abs(u - v).max() > 0 for u, v in zip(seen, seen[1:]))


# ------------------------------------------------------------------ co-training
def test_cotrained_superclass_nets_equal_their_solo_steps(monkeypatch):
    import arch_and_hypers as A
    from lib._co import CoTrainer
    monkeypatch.setattr(A, 'coarse_exits', maps_of('a'))
    mk = lambda i: A.ac_chain(k_cpt=A.k_cpts[i + 1])
    co_nets, solo = _nets([mk(i) for i in range(2)]), _nets([mk(i) for i in range(2)])
    co = CoTrainer(co_nets)
    _compare_with_solo_steps(co_nets, solo, co.run, 2, N)
    merged = [op for op in co._program(N)['ops'] if op.what == 'label_map']
    assert len(merged) == 1 and len(merged[0].host) == 4          # one launch, two records of each of the two nets
    for a, b in zip(co_nets, solo):
        for u, v in zip(a.engine().y_sup, b.engine().y_sup):
            assert torch.equal(u, v)


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_predicts_the_same_bits(monkeypatch, tmp_path):
    import arch_and_hypers as A
    from lib.serdes import read_net, write_net
    from test_predict_nets import host
    net = super_net(A, monkeypatch, 'f')
    x0, y = _batch((32, 32, 3), N, seed=3)
    net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    want = host(net.predict(x0, probs=True))
    path = str(tmp_path / 'net.npy')
    write_net(path, net)
    monkeypatch.setattr(A, 'coarse_exits', None)           # (the file alone says what the net is)
    back = read_net(path)
    assert back.leaf_n_cls == net.leaf_n_cls == [2, 2, 2, 5, 5, 10, 10, 10]
    for ℓa, ℓb in zip(net.leaves, back.leaves):
        assert type(ℓa.comps[-1]) is type(ℓb.comps[-1])
        if type(ℓa.comps[-1]).__name__ == 'SuperclassCrossEntropyError':
            w = ℓb.comps[-1].hypers.w_cls
            assert w.dtype == np.float32 and w.flags.c_contiguous and np.array_equal(w, ℓa.comps[-1].hypers.w_cls)
    got = host(back.predict(x0, probs=True))
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    back.eval({back.x0: x0, back.y: y})
    net.eval({net.x0: x0, net.y: y})
    torch.cuda.synchronize()
    for ℓa, ℓb in zip(net.leaves, back.leaves):
        assert torch.equal(ℓa.c_err, ℓb.c_err) and torch.equal(ℓa.δ_cor, ℓb.δ_cor)


# ------------------------------------------------------------------ the command-line tools
def test_train_nets_coarse_exits_and_classify_images(tmp_path):
    """train-nets --coarse-exits MAP.npy:K writes a checkpoint whose first K exits classify the map's superclasses, and
    classify-images answers in each exit's label space and writes leaf_n_cls beside the keys it always wrote."""
    import os
    import subprocess
    import sys
    from lib.serdes import read_net
    from test_predict_nets import KEYS, ROOT, host
    pkg = os.path.join(ROOT, 'multipath-nn_amd')
    np.save(str(tmp_path / 'map.npy'), R.hard_map(10, 2))
    out = str(tmp_path / 'nets')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '8', '--nets', '0',
                          '--out', out, '--coarse-exits', str(tmp_path / 'map.npy') + ':3'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    ckpt = os.path.join(out, 'cifar10-ac', '0000.npy')
    x = np.random.default_rng(5).random((40, 32, 32, 3)).astype(np.float32)
    np.savez(str(tmp_path / 'images.npz'), x=x)
    pred = str(tmp_path / 'pred.npz')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'classify-images'), ckpt, str(tmp_path / 'images.npz'), '--out', pred,
                          '--batch', '16', '--probs'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    got = dict(np.load(pred))
    assert set(got) == set(KEYS) | {'leaf_n_cls'}
    assert got['leaf_n_cls'].tolist() == [2, 2, 2, 10, 10, 10, 10, 10] and got['leaf_n_cls'].dtype == np.int32
    assert (got['cls'] < got['leaf_n_cls'][got['leaf']]).all() and got['probs'].shape == (40, 10)
    net = read_net(ckpt)
    assert net.leaf_n_cls == got['leaf_n_cls'].tolist()
    want = host(net.predict(x, routed='auto', probs=True))
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '1', '--nets', '0',
                          '--out', out, '--coarse-exits', 'nowhere.npy'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 2 and b'--coarse-exits takes MAP.npy:K' in res.stderr


# ------------------------------------------------------------------ nets without the layer
def _by_hand(A, kind):
    """The default nets built from the spec's own pyr / rcm / reg without going through the constructors (which consult
    `coarse_exits`): what the constructors built before there was a knob."""
    from lib.net_types import ActorNet, SRNet

    def make_net(x0_shape, y_shape):
        if kind == 'sr2':
            return SRNet(x0_shape=x0_shape, y_shape=y_shape, root=A.pyr(A.rcm(0, A.rcm(1, A.reg(y_shape[0])))))
        node = A.rcm(len(A.arch) - 1, A.reg(y_shape[0]))
        for i in range(len(A.arch) - 2, -1, -1):
            node = A.rcm(i, A.reg(y_shape[0]), node)
        return ActorNet(x0_shape=x0_shape, y_shape=y_shape, root=A.pyr(node))
    return make_net


@pytest.mark.parametrize('kind', ['ac', 'sr2'])
def test_nets_without_the_layer_keep_their_launch_lists(kind):
    import arch_and_hypers as A
    assert A.coarse_exits is None
    ctor = A.ac_chain() if kind == 'ac' else A.sr_chain(2)
    nets = [mk((32, 32, 3), (10,)) for mk in (ctor, _by_hand(A, kind))]
    assert [type(c).__name__ for ℓ in nets[0].layers for c in ℓ.comps] == [type(c).__name__ for ℓ in nets[1].layers for c in ℓ.comps]
    routed = [{}] if kind == 'sr2' else [{}, dict(routed=1), dict(routed=3)]
    progs = [('tr', {})] + [(m, kw) for m in ('ev', 'pr', 'pr+p') for kw in routed]
    lists = []
    for net in nets:
        eng = net.engine()
        eng.init_params(3)
        assert eng.label_maps == []
        out = []
        for n in (N, 128):
            for mode, kw in progs:
                p = eng.program(mode, n, **kw)
                out.append([(op.what, op.tag) for op in list(p['fwd']) + list(p['bwd'])])
        lists.append(out)
    assert lists[0] == lists[1]
    assert not any(what == 'label_map' for prog in lists[0] for what, _ in prog)
    assert nets[0].leaf_n_cls == [10] * len(list(nets[0].leaves))
