"""GPU: whole nets whose exits carry ActivityError layers (arch_and_hypers.exit_activity), small ones as in
tests/test_squared_error_nets.py: 5 images of 32x32x3 per training batch, chains on the first three blocks of the spec's
table (four for the net that mixes all four head kinds), the tree on the first four (15 blocks, 15 exits).

  * oracle parity: one training step against RefNetActivity (tests/activity_error_ref.py) in float64 with
    tests/test_net_parity.py's run_case -- its decision-forced comparison, its tolerances, its flip cap: SR with 'map' and
    with 'logits', an actor with all three positions, a critic (optimistic, use_cls_err) with 'logits' + 'probs', dyn_k_cpt
    with 'map', 24 classes (the any-width exit kernels) with all three, a four-block actor mixing plain, superclass, squared
    and squared-linear exits with a per-block dict, the 15-exit tree with 'map' on blocks 0 and 3, and a 24x40 net on the
    general conv kernels.  The layer is backward-only on the device, so the forward quantities run_case compares are those
    of the net without it; every gradient and update carries the penalty's;
  * evaluation: eval dense and routed, predict and exit_conf_curve of a net with the layer equal, bit for bit, those of the
    same net built without it from the same parameters;
  * K-step replay equals single steps, the bound input pipeline equals the array-fed step, two co-trained nets with
    DIFFERENT α equal their solo steps, a checkpoint read back takes the same next step, train-nets --exit-activity runs;
  * launch lists: a net with the layer has the launch list of the plain net; every tail-backward / lin_bwd record of a
    plain net carries zeros in the new fields, every record of a net with the layer its own exit's values.
"""
import numpy as np
import pytest
import torch

import activity_error_ref as R
import superclass_ref as S
from test_cotrain import _compare_with_solo_steps, _nets
from test_net_parity import perturb_routers, run_case
from test_rect_nets import _batch, spec            # noqa: F401  (spec: the fixture that hands run_case batches of a shape)

pytestmark = pytest.mark.gpu

N = 5
SHAPE = (32, 32, 3)
ALL = {'map': 2e-2, 'logits': 5e-2, 'probs': -0.5}
MIXED_LOSS = {0: 'squared', 2: 'squared-linear'}    # with a superclass exit under block 1 and a plain one under block 3
MIXED_ACT = {0: {'logits': 5e-2, 'probs': 0.5}, 1: {'map': 2e-2, 'probs': -0.5}, 2: {'map': -1e-2, 'logits': 2e-2}, 3: ALL}
TREE_ACT = {0: {'map': 2e-2}, 3: {'map': -1e-2}}
PENALTIES = {'map': 2e-2, 'logits': 5e-2, 'probs': 0.5}      # all positive: twelve steps at these learning rates stay finite


# case -> (constructor, blocks, classes, exit_activity, exit_loss, coarse_exits, feeds, k_cpt_vec, image shape)
def case_of(A, case):
    τ_ds = lambda net, t: {net.τ: A.τ_ds(t * 5000)}
    τ_cr = lambda net, t: {net.τ: A.τ_cr(t * 5000)}
    none = lambda net, t: {}
    kv = lambda t, n: np.random.default_rng(t).choice(A.k_cpts, n).astype(np.float32)
    ac = lambda: A.ac_chain(k_cpt=1.6e-8)
    return {
        'sr-map': (lambda: A.sr_chain(3), 3, 10, {'map': 2e-2}, None, None, none, None, SHAPE),
        'sr-logits': (lambda: A.sr_chain(3), 3, 10, {'logits': 5e-2}, None, None, none, None, SHAPE),
        'ac-all': (ac, 3, 10, ALL, None, None, τ_ds, None, SHAPE),
        'cr-logits-probs': (lambda: A.cr_chain(k_cpt=8e-9, optimistic=True, use_cls_err=True), 3, 10, {'logits': -5e-2, 'probs': 0.5},
                            None, None, τ_cr, None, SHAPE),
        'dyn-map': (lambda: A.ac_chain(dyn_k_cpt=True), 3, 10, {'map': 2e-2}, None, None, lambda net, t: {net.τ: 0.8}, kv, SHAPE),
        'ac-24': (ac, 3, 24, ALL, None, None, τ_ds, None, SHAPE),
        'ac-mixed': (ac, 4, 10, MIXED_ACT, MIXED_LOSS, {1: S.hard_map(10, 2)}, τ_ds, None, SHAPE),
        'tree-ac': (lambda: A.ac_tree(k_cpt=1e-9), 4, 10, TREE_ACT, None, None, τ_ds, None, SHAPE),
        'ac-24x40': (ac, 3, 10, ALL, None, None, τ_ds, None, (24, 40, 3)),
    }[case]


CASES = ['sr-map', 'sr-logits', 'ac-all', 'cr-logits-probs', 'dyn-map', 'ac-24', 'ac-mixed', 'tree-ac', 'ac-24x40']


def knobs(A, monkeypatch, blocks=3, activity=None, exit_loss=None, coarse=None):
    monkeypatch.setattr(A, 'arch', A.arch[:blocks])
    monkeypatch.setattr(A, 'exit_activity', activity)
    monkeypatch.setattr(A, 'exit_loss', exit_loss)
    monkeypatch.setattr(A, 'coarse_exits', coarse)


def activity_net(A, monkeypatch, case='ac-all', seed=1234, activity='case'):
    ctor, blocks, n_cls, act, loss, coarse, _, _, shape = case_of(A, case)
    knobs(A, monkeypatch, blocks, act if activity == 'case' else activity, loss, coarse)
    net = ctor()(shape, (n_cls,))
    net.engine().init_params(seed)
    if net._net_kind != 'sr':
        perturb_routers(net)
    return net


def alphas_of(net):
    from lib._eng_common import head_activity
    return [head_activity(ℓ) for ℓ in net.leaves]


def want_alphas(act, blocks):
    per = lambda a: tuple(float((a or {}).get(k, 0.0)) for k in ('map', 'logits', 'probs'))
    return [per(act.get(i) if not any(k in act for k in ('map', 'logits', 'probs')) else act) for i in blocks]


def train_records(eng, n):
    """(tail-backward records, lin_bwd records) of the training program, in exit order."""
    p = eng.program('tr', n)
    ops = {op.what: op for op in list(p['fwd']) + list(p['bwd']) if op.what in ('exit_tail_bwd', 'lin_bwd')}
    assert set(ops) == {'exit_tail_bwd', 'lin_bwd'} and len(ops['lin_bwd'].host) == len(ops['exit_tail_bwd'].host)
    return ops['exit_tail_bwd'].host, ops['lin_bwd'].host


def check_records(eng, n, want):
    """Every record of an exit with a head carries that exit's α (float32 of it); act_w is the tail's w_cerr exactly when the
    map is penalised; a record without a head carries zeros."""
    f32 = lambda v: float(np.float32(v))
    tails, lins = train_records(eng, n)
    want = list(want)
    for tb, lb in zip(tails, lins):
        a_map, a_z, a_p = want.pop(0) if tb.f.n_cls else (0.0, 0.0, 0.0)
        assert (lb.act_alpha, tb.act_z, tb.act_p) == (f32(a_map), f32(a_z), f32(a_p))
        assert (lb.act_w == tb.w_cerr and lb.act_w) if a_map else not lb.act_w
    assert not want


# ------------------------------------------------------------------ parity with the float64 oracle
@pytest.mark.parametrize('case', CASES)
def test_oracle_parity(spec, monkeypatch, case):
    from oracle import ref_net
    import arch_and_hypers as A0
    ctor, blocks, n_cls, act, loss, coarse, feeds, kv, shape = case_of(A0, case)
    A, wrap = spec(shape)
    knobs(A, monkeypatch, blocks, act, loss, coarse)
    monkeypatch.setattr(ref_net, 'RefNet', R.RefNetActivity)           # (run_case imports it when it is called)
    seen = []

    def make(x0_shape, y_shape):
        net = wrap(ctor())(x0_shape, y_shape)
        seen.append(net)
        return net
    run_case(make, N, feeds, steps=1, n_cls=n_cls, k_cpt_vec=kv)
    net, = seen
    eng = net.engine()
    assert eng.generic_exits == (n_cls > 16) and eng.generic_convs == (shape != SHAPE)
    index = list(range(blocks)) if net._net_kind != 'sr' else [blocks - 1]
    want = want_alphas(act, index)
    if case.startswith('tree'):
        # 1, 2, 4 and 8 blocks of index 0 .. 3, each with its exit
        assert len(eng.blocks) == 15
        want = sorted(w for i, w in zip(index, want) for _ in range(2 ** i))
        assert sorted(alphas_of(net)) == want and sum(1 for w in want if w[0]) == 9
    else:
        assert alphas_of(net) == want
        check_records(eng, N, want)
    assert any(any(w) for w in want)


# ------------------------------------------------------------------ evaluation ignores the layer
@pytest.mark.parametrize('case', ['ac-all', 'ac-24', 'ac-mixed'])
def test_evaluation_and_predict_equal_the_net_without_the_layer(monkeypatch, case):
    import arch_and_hypers as A
    from test_predict_nets import host
    from test_routed_eval import snapshot
    a, b = activity_net(A, monkeypatch, case), activity_net(A, monkeypatch, case, activity=None)
    assert any(any(w) for w in alphas_of(a)) and not any(any(w) for w in alphas_of(b))
    assert torch.equal(a.engine().P, b.engine().P)
    n_cls = case_of(A, case)[2]
    x0, y = _batch(SHAPE, 16, n_cls, seed=3)

    def snaps(net):
        out = []
        for routed in (False, True):
            net.eval({net.x0: x0, net.y: y}, routed=routed)
            torch.cuda.synchronize()
            out.append(snapshot(net))
        pr = [host(net.predict(x0, routed=r, probs=True)) for r in (False, True, 'auto')]
        gated = host(net.predict(x0, exit_conf=0.3))
        curve = net.exit_conf_curve(x0, y, np.array([0.0, 0.3, 0.6, 2.0], np.float32))
        return out, pr, gated, curve
    sa, pa, ga, ca = snaps(a)
    sb, pb, gb, cb = snaps(b)
    for u, v in zip(sa, sb):
        for grp in ('p_ev', 'c_err', 'd_cor', 'r'):
            assert u[grp].keys() == v[grp].keys() and u[grp]
            for i in u[grp]:
                assert np.array_equal(u[grp][i], v[grp][i]), (grp, i)
        # (the statistics: keyed by the id of their layer; the same layers in the same order)
        assert [k[:2] for k in u['state']] == [k[:2] for k in v['state']] and u['state']
        assert all(np.array_equal(p, q) for p, q in zip(u['state'].values(), v['state'].values()))
    for u, v in list(zip(pa, pb)) + [(ga, gb)]:
        assert set(u) == set(v) and 'cls' in u
        for k in u:
            assert np.array_equal(u[k], v[k]), k
    for k in ('correct', 'ops', 'hist'):
        assert np.array_equal(getattr(ca, k), getattr(cb, k)), k
    assert len(set(ca.ops.tolist())) > 1                       # (the thresholds do move images between exits)


# ------------------------------------------------------------------ K-step replay
def test_k_step_replay_equals_single_steps(monkeypatch):
    import arch_and_hypers as A
    nets = [activity_net(A, monkeypatch, 'ac-all', activity=PENALTIES) for _ in range(2)]
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
        assert all(torch.isfinite(v).all() for v in (engs[0].P, engs[0].A, engs[0].S)), call       # (equal NaNs would compare unequal)
        assert torch.equal(engs[0].P, engs[1].P) and torch.equal(engs[0].A, engs[1].A) and torch.equal(engs[0].S, engs[1].S), call
    assert any(k[0] == 'trK' and not isinstance(v, str) for k, v in engs[0]._graphs.items())


# ------------------------------------------------------------------ the input pipeline
def test_bound_input_pipeline_equals_the_array_fed_step(monkeypatch):
    import arch_and_hypers as A
    from lib.data import Dataset
    from test_cotrain import _copy_state
    ds = Dataset.synthetic(n_tr=60, n_ts=20, seed=1)
    a, b = (activity_net(A, monkeypatch, 'ac-all') for _ in range(2))
    ea, eb = a.engine(), b.engine()
    np.random.seed(3)
    x0, y = ds.bind_engine(ea, N)
    for t in range(4):                                     # eager | capture | replays: every form reads the step's own batch
        _copy_state(a, b)
        ds.stage_training_draws(N, eng=ea)
        a.train.run({a.x0: x0, a.y: y, a.mode: 'tr', a.λ_lrn: 0.05, a.τ: 1.0})
        torch.cuda.synchronize()
        xb, yb = ea.x0[:N].cpu().numpy().copy(), ea.y[:N].cpu().numpy().copy()
        b.train.run({b.x0: xb, b.y: yb, b.mode: 'tr', b.λ_lrn: 0.05, b.τ: 1.0})
        torch.cuda.synchronize()
        assert torch.equal(ea.P, eb.P) and torch.equal(ea.A, eb.A) and torch.equal(ea.S, eb.S), t


# ------------------------------------------------------------------ co-training
def test_cotrained_nets_with_different_alpha_equal_their_solo_steps(monkeypatch):
    import arch_and_hypers as A
    from lib._co import CoTrainer
    knobs(A, monkeypatch, 3)
    acts = [ALL, {'map': -1e-2, 'logits': 0.1}]

    def mk(i):
        ctor = A.ac_chain(k_cpt=A.k_cpts[i + 1])

        def make(x0_shape, y_shape):
            A.exit_activity = acts[i]                      # (read when the constructor is called; monkeypatch restores it)
            try:
                return ctor(x0_shape, y_shape)
            finally:
                A.exit_activity = None
        return make
    co_nets, solo = _nets([mk(i) for i in range(2)]), _nets([mk(i) for i in range(2)])
    assert [alphas_of(n)[0] for n in co_nets] == [want_alphas(a, [0])[0] for a in acts]
    co = CoTrainer(co_nets)
    _compare_with_solo_steps(co_nets, solo, co.run, 2, N)
    f32 = lambda v: float(np.float32(v))
    for what, get in (('exit_tail_bwd', lambda r: (r.act_z, r.act_p)), ('lin_bwd', lambda r: (r.act_alpha,))):
        merged = [op for op in co._program(N)['ops'] if op.what == what]
        assert len(merged) == 1 and len(merged[0].host) == 6          # one launch, the three records of each of the two nets
        want = [tuple(f32(a.get(k, 0.0)) for k in (('logits', 'probs') if what == 'exit_tail_bwd' else ('map',))) for a in acts]
        assert [get(r) for r in merged[0].host] == [want[0]] * 3 + [want[1]] * 3
    lins = [op for op in co._program(N)['ops'] if op.what == 'lin_bwd'][0].host
    assert len({r.act_w for r in lins}) == 6                           # each record its own leaf's (and its own net's) w_cerr


# ------------------------------------------------------------------ checkpoints and drivers
def test_checkpoint_read_back_takes_the_same_next_step(monkeypatch, tmp_path):
    import arch_and_hypers as A
    from lib.serdes import read_net, write_net
    net = activity_net(A, monkeypatch, 'ac-mixed')
    x0, y = _batch(SHAPE, N, seed=3)
    feed = lambda m: {m.x0: x0, m.y: y, m.mode: 'tr', m.λ_lrn: 0.05, m.τ: 1.0}
    net.train.run(feed(net))
    path = str(tmp_path / 'net.npy')
    write_net(path, net, with_optimizer=True)
    back = read_net(path)                                  # (the file carries the chains: the layers and their α)
    assert alphas_of(back) == alphas_of(net) == want_alphas(MIXED_ACT, range(4))
    again = activity_net(A, monkeypatch, 'ac-mixed', seed=7)           # ... and a net built with the same knob takes its parameters
    from lib.serdes import load_params
    load_params(again.root, np.load(path, allow_pickle=True)[()]['root'])
    for m in (net, back, again):
        m.train.run(feed(m))
    torch.cuda.synchronize()
    for m in (back, again):
        for p, q in zip(net._all_params, m._all_params):
            if p.trainable:
                assert torch.equal(p.grad, q.grad), (p.owner.name, p.name)
        for ℓa, ℓb in zip(net.leaves, m.leaves):
            assert torch.equal(ℓa.c_err, ℓb.c_err) and torch.equal(ℓa.p_tr, ℓb.p_tr)


def test_train_nets_exit_activity(tmp_path):
    """train-nets --exit-activity logits=0.01,map=1e-4:2 writes a checkpoint whose first two exits carry the two layers."""
    import os
    import subprocess
    import sys
    from lib.serdes import read_net
    from test_predict_nets import ROOT
    pkg = os.path.join(ROOT, 'multipath-nn_amd')
    out = str(tmp_path / 'nets')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '4', '--nets', '0',
                          '--out', out, '--exit-activity', 'logits=0.01,map=1e-4:2'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    net = read_net(os.path.join(out, 'cifar10-ac', '0000.npy'))
    assert alphas_of(net) == [(1e-4, 0.01, 0.0)] * 2 + [(0.0, 0.0, 0.0)] * 6
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '4', '--nets', '0',
                          '--out', out, '--exit-activity', 'logit=0.01'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 2 and b'--exit-activity' in res.stderr


# ------------------------------------------------------------------ launch lists
PROGRAMS = [('tr', {}), ('ev', {}), ('ev', dict(routed=1)), ('pr', {}), ('pr+p', {}), ('pr+p', dict(routed=1))]


@pytest.mark.parametrize('kind', ['ac', 'sr2'])
def test_launch_lists_and_the_fields_of_every_record(monkeypatch, kind):
    import arch_and_hypers as A
    assert A.exit_activity is None
    ctor = (lambda: A.ac_chain()) if kind == 'ac' else (lambda: A.sr_chain(2))
    progs = PROGRAMS if kind == 'ac' else [p for p in PROGRAMS if not p[1]]
    per_block = {i: {'map': 1e-3 * (i + 1), 'logits': 1e-2 * (i + 1), 'probs': -0.1 * (i + 1)} for i in range(len(A.arch))}
    lists = {}
    for name, act in (('plain', None), ('all', ALL), ('per-block', per_block)):
        monkeypatch.setattr(A, 'exit_activity', act)
        net = ctor()(SHAPE, (10,))
        eng = net.engine()
        eng.init_params(3)
        out = []
        index = range(len(A.arch)) if kind == 'ac' else [1]
        want = [(0.0, 0.0, 0.0)] * len(index) if act is None else want_alphas(act, index)
        assert alphas_of(net) == want
        for n in (N, 128, 256):                            # (the tuned tails; beyond 128 samples the any-width tails)
            for mode, kw in progs:
                p = eng.program(mode, n, **kw)
                out.append([(op.what, op.tag) for op in list(p['fwd']) + list(p['bwd'])])
            check_records(eng, n, want)
        lists[name] = out
    assert lists['plain'] == lists['all'] == lists['per-block']
