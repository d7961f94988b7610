"""GPU: whole nets whose exits end in SquaredError (arch_and_hypers.exit_loss), small ones on 32x32x3 images, 5 images per
training batch (16 or 32 where every exit has to be taken): chains -- sr_chain(3), ac_chain, cr_chain -- on the first three
blocks of the spec's table (four for the net that mixes all four head kinds), and trees -- ac_tree, cr_tree -- on the first
four: a binary tree over blocks 0-2 with a block 3 under each of its four ends, 15 blocks and 15 exits, every switch of
blocks 0-2 with THREE sinks (its exit and two forked blocks), `exit_loss` naming the forked blocks by their index.

  * oracle parity: one training step and one evaluation against RefNetSquared (tests/squared_error_ref.py) in float64,
    with tests/test_net_parity.py's run_case -- its decision-forced comparison, its tolerances, its flip cap -- as
    tests/test_superclass_nets.py::test_oracle_parity: SR, actor, critic (use_cls_err, optimistic), dyn_k_cpt, both forms,
    real-valued targets, 24 classes (the any-width exit kernels), a net mixing cross-entropy, superclass and both
    squared exits, and the two trees (actor: squared, squared-linear and cross-entropy exits; critic with use_cls_err:
    squared-linear and squared exits on real-valued targets);
  * the evaluation paths agree as tests/test_predict_nets.py's check_consistent demands (dense, routed, predict with NaN
    labels, eval -> predict -> eval), on the chains and on the actor tree with every one of its 15 exits taken (sibling
    sample lists under three-sink switches); the exits on the softmax return probabilities, the linear ones raw outputs;
  * K-step replay equals single steps, the bound input pipeline equals the array-fed step, two co-trained nets equal
    their solo steps as tests/test_cotrain.py holds them, a checkpoint read back predicts the same bits, train-nets
    --exit-loss and classify-images run end to end;
  * launch lists: a net with squared exits has the launch list of the same net with plain exits; every tail / exit_ev
    record of a plain net carries loss == 0, of a squared net its exit's kind.
"""
import numpy as np
import pytest
import torch

import squared_error_ref as R
import superclass_ref as S
import test_net_parity
from lib import _hip
from test_cotrain import _compare_with_solo_steps, _nets
from test_net_parity import perturb_routers, run_case
from test_rect_nets import _batch, spec            # noqa: F401  (spec: the fixture that hands run_case batches of a shape)

pytestmark = pytest.mark.gpu

N = 5
SHAPE = (32, 32, 3)
MIXED = {0: 'squared', 2: 'squared-linear'}        # with a superclass exit under block 1 and a plain one under block 3
# the trees (block index -> the exits of EVERY block of that index: 1, 2, 4 and 8 of them)
TREE_AC = {0: 'squared', 1: 'squared-linear', 3: 'squared'}            # (the four exits of the blocks 2: cross-entropy)
TREE_CR = {0: 'squared-linear', 2: 'squared', 3: 'squared-linear'}


class RefNetAll(R.RefNetSquared, S.RefNetSuper):
    """SquaredError, SuperclassCrossEntropyError and RefNet's own layers."""


def real_batch(shape, n, n_cls=10, seed=0):
    """Regression targets: any float vector."""
    x0, _ = _batch(shape, n, n_cls, seed)
    return x0, np.random.default_rng(1000 + seed).standard_normal((n, n_cls)).astype(np.float32)


# case -> (constructor, blocks, classes, exit_loss, coarse_exits, real-valued targets, feeds, k_cpt_vec)
def case_of(A, case):
    τ_ds = lambda net, t: {net.τ: A.τ_ds(t * 5000)}
    τ_cr = lambda net, t: {net.τ: A.τ_cr(t * 5000)}
    none = lambda net, t: {}
    kv = lambda t, n: np.random.default_rng(t).choice(A.k_cpts, n).astype(np.float32)
    ac = lambda: A.ac_chain(k_cpt=1.6e-8)
    cr = lambda: A.cr_chain(k_cpt=8e-9, optimistic=True, use_cls_err=True)
    return {
        'sr-sq': (lambda: A.sr_chain(3), 3, 10, 'squared', None, False, none, None),
        'sr-lin-real': (lambda: A.sr_chain(3), 3, 10, 'squared-linear', None, True, none, None),
        'ac-sq': (ac, 3, 10, 'squared', None, False, τ_ds, None),
        'ac-lin': (ac, 3, 10, 'squared-linear', None, False, τ_ds, None),
        'ac-lin-real': (ac, 3, 10, 'squared-linear', None, True, τ_ds, None),
        'cr-sq': (cr, 3, 10, 'squared', None, False, τ_cr, None),
        'cr-lin': (cr, 3, 10, 'squared-linear', None, False, τ_cr, None),
        'dyn-sq': (lambda: A.ac_chain(dyn_k_cpt=True), 3, 10, 'squared', None, False, lambda net, t: {net.τ: 0.8}, kv),
        'ac-24': (ac, 3, 24, {0: 'squared', 1: 'squared-linear'}, None, False, τ_ds, None),
        'ac-mixed': (ac, 4, 10, MIXED, {1: S.hard_map(10, 2)}, False, τ_ds, None),
        'tree-ac': (lambda: A.ac_tree(k_cpt=1e-9), 4, 10, TREE_AC, None, False, τ_ds, None),
        'tree-cr': (lambda: A.cr_tree(k_cpt=8e-9, use_cls_err=True), 4, 10, TREE_CR, None, True, τ_cr, None),
    }[case]


CASES = ['sr-sq', 'sr-lin-real', 'ac-sq', 'ac-lin', 'ac-lin-real', 'cr-sq', 'cr-lin', 'dyn-sq', 'ac-24', 'ac-mixed', 'tree-ac', 'tree-cr']


def knobs(A, monkeypatch, blocks=3, exit_loss='squared', coarse=None):
    monkeypatch.setattr(A, 'arch', A.arch[:blocks])
    monkeypatch.setattr(A, 'exit_loss', exit_loss)
    monkeypatch.setattr(A, 'coarse_exits', coarse)


def squared_net(A, monkeypatch, case='ac-sq', seed=1234):
    ctor, blocks, n_cls, loss, coarse, _, _, _ = case_of(A, case)
    knobs(A, monkeypatch, blocks, loss, coarse)
    net = ctor()(SHAPE, (n_cls,))
    net.engine().init_params(seed)
    if net._net_kind != 'sr':
        perturb_routers(net)
    return net


def kinds_of(net):
    from lib._eng_common import head_parts
    return [head_parts(ℓ)[2] for ℓ in net.leaves]


def records(eng, mode, n, **kw):
    """(what, record) of every tail / exit_ev record of a program."""
    p = eng.program(mode, n, **kw)
    out = []
    for op in list(p['fwd']) + list(p['bwd']):
        if op.what in ('exit_tail_fwd', 'exit_tail_bwd', 'exit_ev'):
            assert op.host, op.what
            out += [(op.what, r.f if op.what == 'exit_tail_bwd' else r) for r in op.host]
    return out


PROGRAMS = [('tr', {}), ('ev', {}), ('ev', dict(routed=1)), ('pr', {}), ('pr+p', {}), ('pr+p', dict(routed=1))]


# ------------------------------------------------------------------ parity with the float64 oracle
@pytest.mark.parametrize('case', CASES)
def test_oracle_parity(spec, monkeypatch, case):
    from oracle import ref_net
    import arch_and_hypers as A0
    ctor, blocks, n_cls, loss, coarse, real, feeds, kv = case_of(A0, case)
    A, wrap = spec(SHAPE)
    knobs(A, monkeypatch, blocks, loss, coarse)
    monkeypatch.setattr(ref_net, 'RefNet', RefNetAll)              # (run_case imports it when it is called)
    if real:
        monkeypatch.setattr(test_net_parity, 'batch', lambda n, c0=3, n_cls=10, seed=0, hw=32: real_batch(SHAPE, n, n_cls, seed))
    seen = []

    def make(x0_shape, y_shape):
        net = wrap(ctor())(x0_shape, y_shape)
        seen.append(net)
        return net
    run_case(make, N, feeds, steps=1, n_cls=n_cls, k_cpt_vec=kv)
    net, = seen
    eng = net.engine()
    assert eng.generic_exits == (n_cls > 16)
    want = {'squared': _hip.LOSS_SQ, 'squared-linear': _hip.LOSS_SQ_LIN, None: _hip.LOSS_CE}
    kinds = [want[loss if isinstance(loss, str) else loss.get(i)] for i in range(blocks)]
    if net._net_kind == 'sr':
        kinds = kinds[-1:]
    if case.startswith('tree'):
        # 1, 2, 4 and 8 blocks of index 0 .. 3, each with its exit; every switch of the blocks 0-2 has three sinks
        kinds = sorted(k for i, k in enumerate(kinds) for _ in range(2 ** i))
        assert len(eng.blocks) == 15 and [len(ℓ.sinks) for ℓ in net.switches] == [3] * 7
        assert sorted(kinds_of(net)) == kinds == sorted(b.loss for b in eng.blocks if b.head is not None) and len(set(kinds)) >= 2
    else:
        assert kinds_of(net) == kinds == [b.loss for b in eng.blocks if b.head is not None]
    for mode, kw in PROGRAMS if net._net_kind != 'sr' else [p for p in PROGRAMS if not p[1]]:
        recs = records(eng, mode, N, **kw)
        assert recs and sorted(r.loss for _, r in recs if r.n_cls) == sorted(kinds * (2 if mode == 'tr' else 1)), (mode, kw)


# ------------------------------------------------------------------ the evaluation paths
def check_consistent_squared(net, x0, y, modes):
    """tests/test_predict_nets.py's check_consistent for exits that may answer with raw outputs."""
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
    want_ops = (pev.astype(np.float64) * np.array(eng.node_ops_host, np.float64)[:, None]).sum(0)
    dense = predict_poisoned(net, x0, routed=False, probs=True)
    # (a superclass exit of the mixed net answers in its own label space: tests/test_superclass_nets.py)
    from test_superclass_nets import leaf_maps
    y_leaf = [S.label_map(y, w) for w in leaf_maps(net)]
    want_cls = np.array([y_leaf[l][i].argmax() for i, l in enumerate(want_leaf)])
    assert np.array_equal(dense['cls'] == want_cls, acc == 1) and set(np.unique(acc)) <= {0.0, 1.0}
    assert np.array_equal(dense['leaf'], want_leaf)
    assert np.array_equal(dense['ops'].astype(np.float64), want_ops)
    ar = np.arange(n)
    assert np.array_equal(dense['conf'], dense['probs'][ar, dense['cls']])
    assert np.array_equal(dense['probs'].argmax(1), dense['cls'])
    linear = np.array(kinds_of(net))[dense['leaf']] == _hip.LOSS_SQ_LIN
    sums = dense['probs'].astype(np.float64).sum(1)
    assert np.abs(sums[~linear] - 1).max(initial=0) < 1e-5          # probabilities where the exit has a softmax
    for mode in modes:
        got = predict_poisoned(net, x0, routed=mode, probs=True)
        for k in KEYS:
            assert np.array_equal(got[k], dense[k]), (mode, k)
    net.eval(feed)
    torch.cuda.synchronize()
    same_snapshot(first, snapshot(net))
    return dense, linear


@pytest.mark.parametrize('case', ['ac-sq', 'ac-lin-real', 'ac-24', 'ac-mixed', 'tree-ac', 'tree-cr'])
def test_dense_routed_and_predict_agree(monkeypatch, case):
    import arch_and_hypers as A
    from test_predict_nets import spread_over_leaves
    from test_routed_eval import calibrate_exit_fractions, randomise_routers
    _, blocks, n_cls, _, _, real, _, _ = case_of(A, case)
    net = squared_net(A, monkeypatch, case)
    tree = case.startswith('tree')
    n_leaves = len(list(net.leaves))
    n = 32 if tree else 4 * blocks
    x0, y = (real_batch if real else _batch)(SHAPE, n, n_cls, seed=3)
    for t in range(2):                                     # (moving averages away from their initial values)
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    randomise_routers(net)
    if tree:
        # every leaf of the tree: two samples each, three at two of them -- every three-sink switch fills both sibling lists
        net.eval({net.x0: x0, net.y: y})
        r = {id(ℓ): ℓ.router.x.cpu().numpy().copy() for ℓ in net.switches}
        spread_over_leaves(net, lambda ℓ: r[id(ℓ)], n)
    else:
        calibrate_exit_fractions(net, x0, y, [1 / blocks] * (blocks - 1))
    dense, linear = check_consistent_squared(net, x0, y, modes=(True, 1, 2, 'auto') if tree else (True, 1, 'auto'))
    assert n_leaves == (15 if tree else blocks) and len(set(dense['leaf'].tolist())) == n_leaves     # every exit is taken
    if linear.any():
        # raw outputs: the row is the head's LinTrans output, not a distribution
        assert np.abs(dense['probs'][linear].astype(np.float64).sum(1) - 1).min() > 1e-3
        eng = net.engine()
        for b in eng.blocks:
            if b.loss == _hip.LOSS_SQ_LIN and eng.generic_exits:          # (the any-width forms keep z in memory)
                rows = np.flatnonzero(dense['leaf'] == b.head.leaf_id)
                net.eval({net.x0: x0, net.y: y})
                torch.cuda.synchronize()
                assert np.array_equal(dense['probs'][rows][:, :b.n_out], b.z[:n].cpu().numpy()[rows])


def test_sr_chain_with_a_linear_head_predicts_raw_outputs(monkeypatch):
    import arch_and_hypers as A
    from test_predict_nets import predict_poisoned
    net = squared_net(A, monkeypatch, 'sr-lin-real')
    x0, y = real_batch(SHAPE, N, seed=3)
    net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05})
    net.eval({net.x0: x0, net.y: y})
    acc = net.state()[(net, 'acc')].cpu().numpy()
    c_err = next(iter(net.leaves)).c_err.cpu().numpy()
    for routed in (False, True, 'auto'):
        got = predict_poisoned(net, x0, routed=routed, probs=True)
        assert got['probs'].shape == (N, 10) and (got['leaf'] == 0).all()
        assert np.array_equal(got['cls'] == y.argmax(1), acc == 1)
        assert np.array_equal(got['conf'], got['probs'].max(1))
        # the rows are the outputs the loss was computed on
        want = ((got['probs'].astype(np.float64) - y) ** 2).sum(1)
        assert np.abs(want - c_err).max() <= 2e-5 * (1 + np.abs(want).max())


# ------------------------------------------------------------------ K-step replay
def test_k_step_replay_equals_single_steps(monkeypatch):
    import arch_and_hypers as A
    nets = [squared_net(A, monkeypatch, 'ac-mixed') for _ in range(2)]
    K = 4
    x0, y = (torch.from_numpy(v).cuda() for v in _batch(SHAPE, N, seed=3))
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
    a, b = (squared_net(A, monkeypatch, 'ac-mixed') for _ in range(2))
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
        assert torch.equal(ea.P, eb.P) and torch.equal(ea.A, eb.A) and torch.equal(ea.S, eb.S), t
        for la, lb in zip(a.leaves, b.leaves):
            assert torch.equal(la.c_err, lb.c_err), t
    assert any(np.abs(u - v).max() > 0 for u, v in zip(seen, seen[1:]))


# ------------------------------------------------------------------ co-training
def test_cotrained_squared_nets_equal_their_solo_steps(monkeypatch):
    import arch_and_hypers as A
    from lib._co import CoTrainer
    knobs(A, monkeypatch, 4, MIXED, {1: S.hard_map(10, 2)})
    mk = lambda i: A.ac_chain(k_cpt=A.k_cpts[i + 1])
    co_nets, solo = _nets([mk(i) for i in range(2)]), _nets([mk(i) for i in range(2)])
    co = CoTrainer(co_nets)
    _compare_with_solo_steps(co_nets, solo, co.run, 2, N)
    for what in ('exit_tail_fwd', 'exit_tail_bwd'):
        merged = [op for op in co._program(N)['ops'] if op.what == what]
        assert len(merged) == 1 and len(merged[0].host) == 8          # one launch, the four records of each of the two nets
        loss = [(r.f if what == 'exit_tail_bwd' else r).loss for r in merged[0].host]
        assert loss == 2 * [_hip.LOSS_SQ, _hip.LOSS_CE, _hip.LOSS_SQ_LIN, _hip.LOSS_CE]


# ------------------------------------------------------------------ checkpoints and drivers
def test_checkpoint_round_trip_predicts_the_same_bits(monkeypatch, tmp_path):
    import arch_and_hypers as A
    from lib.serdes import read_net, write_net
    from test_predict_nets import host
    net = squared_net(A, monkeypatch, 'ac-mixed')
    x0, y = _batch(SHAPE, N, seed=3)
    net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
    want = host(net.predict(x0, probs=True))
    path = str(tmp_path / 'net.npy')
    write_net(path, net)
    monkeypatch.setattr(A, 'exit_loss', None)              # (the file alone says what the net is)
    monkeypatch.setattr(A, 'coarse_exits', None)
    back = read_net(path)
    assert kinds_of(back) == kinds_of(net) == [_hip.LOSS_SQ, _hip.LOSS_CE, _hip.LOSS_SQ_LIN, _hip.LOSS_CE]
    got = host(back.predict(x0, probs=True))
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    back.eval({back.x0: x0, back.y: y})
    net.eval({net.x0: x0, net.y: y})
    torch.cuda.synchronize()
    for ℓa, ℓb in zip(net.leaves, back.leaves):
        assert torch.equal(ℓa.c_err, ℓb.c_err) and torch.equal(ℓa.δ_cor, ℓb.δ_cor)


def test_train_nets_exit_loss_and_classify_images(tmp_path):
    """train-nets --exit-loss squared:2 writes a checkpoint whose first two exits end in Softmax -> SquaredError, and
    classify-images needs no flag: the checkpoint's description carries the chains."""
    import os
    import subprocess
    import sys
    from lib.serdes import read_net
    from test_predict_nets import KEYS, ROOT, host
    pkg = os.path.join(ROOT, 'multipath-nn_amd')
    out = str(tmp_path / 'nets')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '8', '--nets', '0',
                          '--out', out, '--exit-loss', 'squared:2'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    ckpt = os.path.join(out, 'cifar10-ac', '0000.npy')
    x = np.random.default_rng(5).random((40, 32, 32, 3)).astype(np.float32)
    np.savez(str(tmp_path / 'images.npz'), x=x)
    pred = str(tmp_path / 'pred.npz')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'classify-images'), ckpt, str(tmp_path / 'images.npz'), '--out', pred,
                          '--batch', '16', '--probs'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    got = dict(np.load(pred))
    assert set(got) == set(KEYS)
    net = read_net(ckpt)
    assert kinds_of(net) == [_hip.LOSS_SQ] * 2 + [_hip.LOSS_CE] * 6
    want = host(net.predict(x, routed='auto', probs=True))
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------ launch lists
@pytest.mark.parametrize('kind', ['ac', 'sr2'])
def test_launch_lists_and_the_loss_of_every_record(monkeypatch, kind):
    import arch_and_hypers as A
    assert A.exit_loss is None
    ctor = (lambda: A.ac_chain()) if kind == 'ac' else (lambda: A.sr_chain(2))
    progs = PROGRAMS if kind == 'ac' else [p for p in PROGRAMS if not p[1]]
    lists, kinds = {}, {}
    for loss in (None, 'squared', 'squared-linear'):
        monkeypatch.setattr(A, 'exit_loss', loss)
        net = ctor()(SHAPE, (10,))
        eng = net.engine()
        eng.init_params(3)
        out, seen = [], []
        for n in (N, 128):
            for mode, kw in progs:
                p = eng.program(mode, n, **kw)
                out.append([(op.what, op.tag) for op in list(p['fwd']) + list(p['bwd'])])
                seen += [r.loss for _, r in records(eng, mode, n, **kw) if r.n_cls]
                assert all(r.loss == 0 for _, r in records(eng, mode, n, **kw) if not r.n_cls)
        lists[loss], kinds[loss] = out, seen
    assert lists[None] == lists['squared'] == lists['squared-linear']
    assert kinds[None] and set(kinds[None]) == {_hip.LOSS_CE}
    assert set(kinds['squared']) == {_hip.LOSS_SQ} and set(kinds['squared-linear']) == {_hip.LOSS_SQ_LIN}
    assert len(kinds[None]) == len(kinds['squared']) == len(kinds['squared-linear'])
