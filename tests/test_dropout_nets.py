"""GPU: whole nets whose exits carry Dropout in front of their classifier (arch_and_hypers.exit_dropout), small ones as in
tests/test_activity_nets.py: 5 images of 32x32x3 per training batch, chains on the first three blocks of the spec's table
(four for the net that mixes head kinds), the tree on the first four (15 blocks, 15 exits, 3-sink switches).

  * oracle parity: training steps against RefNetDropout (tests/dropout_ref.py: the masks restated in numpy from the layer's
    seed, the leaf and the engine's step counter) in float64 with tests/test_net_parity.py's run_case -- its decision-forced
    comparison, its tolerances, its flip cap: an SR chain, an actor (two steps: the counter moves), a critic, dyn_k_cpt, the
    tree, 24 classes (the any-width exit kernels), a 24x40 net on the general conv kernels, and a four-block actor mixing
    heads with and without the layer with squared, superclass and logit-ActivityError exits;
  * bit for bit: λ = 1 trains as the net without the layer, launch for launch; eval dense and routed, predict and
    exit_conf_curve of a net with λ = 0.5 equal those of the same weights without the layer, launch lists included; the
    training launch list differs by the two launches and the extra lin records alone; run_steps(K = 4) equals 4 x run();
    the bound input pipeline equals the array-fed step;
  * state: a long-lived engine through a dozen random train / eval / predict / run_steps operations against fresh engines
    with dropout_step set; two engines with one seed agree, with two seeds they do not; co-training 2 and 4 nets with
    different seeds equals each net alone (tests/test_cotrain.py's standard), K joint steps in one graph equal K joint
    steps; a checkpoint keeps λ and the seed; the drivers run with --exit-dropout 0.5:2 --dropout-seed 3.
"""
import numpy as np
import pytest
import torch

import dropout_ref as R
import superclass_ref as S
from test_cotrain import _compare_with_solo_steps, _copy_state, _nets
from test_net_parity import perturb_routers, run_case
from test_rect_nets import _batch, spec            # noqa: F401  (spec: the fixture that hands run_case batches of a shape)

pytestmark = pytest.mark.gpu

N = 5
SHAPE = (32, 32, 3)
MIXED_LOSS = {0: 'squared', 2: 'squared-linear'}    # with a superclass exit under block 1 and a plain one under block 3
MIXED_DROP = {0: 0.5, 1: 0.8, 3: 0.5}               # block 2 (squared-linear) without the layer
MIXED_ACT = {1: {'logits': 5e-2}, 2: {'logits': 2e-2, 'map': 1e-2}, 3: {'probs': -0.5}}
TREE_DROP = {0: 0.5, 2: 0.7, 3: 0.5}


# case -> (constructor, blocks, classes, exit_dropout, seed, exit_loss, coarse_exits, exit_activity, feeds, k_cpt_vec, shape, steps)
def case_of(A, case):
    τ_ds = lambda net, t: {net.τ: A.τ_ds(t * 5000)}
    τ_cr = lambda net, t: {net.τ: A.τ_cr(t * 5000)}
    none = lambda net, t: {}
    kv = lambda t, n: np.random.default_rng(t).choice(A.k_cpts, n).astype(np.float32)
    ac = lambda: A.ac_chain(k_cpt=1.6e-8)
    return {
        'sr': (lambda: A.sr_chain(3), 3, 10, 0.5, 0, None, None, None, none, None, SHAPE, 1),
        'ac': (ac, 3, 10, 0.5, 11, None, None, None, τ_ds, None, SHAPE, 2),
        'cr': (lambda: A.cr_chain(k_cpt=8e-9, optimistic=True, use_cls_err=True), 3, 10, 0.7, 2 ** 40 + 3, None, None, None, τ_cr, None, SHAPE, 1),
        'dyn': (lambda: A.ac_chain(dyn_k_cpt=True), 3, 10, 0.5, 5, None, None, None, lambda net, t: {net.τ: 0.8}, kv, SHAPE, 1),
        'tree-ac': (lambda: A.ac_tree(k_cpt=1e-9), 4, 10, TREE_DROP, 7, None, None, None, τ_ds, None, SHAPE, 1),
        'ac-24': (ac, 3, 24, 0.5, 1, None, None, None, τ_ds, None, SHAPE, 1),
        'ac-24x40': (ac, 3, 10, 0.5, 2, None, None, None, τ_ds, None, (24, 40, 3), 1),
        'ac-mixed': (ac, 4, 10, MIXED_DROP, 3, MIXED_LOSS, {1: S.hard_map(10, 2)}, MIXED_ACT, τ_ds, None, SHAPE, 1),
    }[case]


CASES = ['sr', 'ac', 'cr', 'dyn', 'tree-ac', 'ac-24', 'ac-24x40', 'ac-mixed']


def knobs(A, monkeypatch, blocks=3, dropout=None, seed=0, exit_loss=None, coarse=None, activity=None):
    monkeypatch.setattr(A, 'arch', A.arch[:blocks])
    monkeypatch.setattr(A, 'exit_dropout', dropout)
    monkeypatch.setattr(A, 'dropout_seed', seed)
    monkeypatch.setattr(A, 'exit_loss', exit_loss)
    monkeypatch.setattr(A, 'coarse_exits', coarse)
    monkeypatch.setattr(A, 'exit_activity', activity)


def dropout_net(A, monkeypatch, case='ac', init=1234, dropout='case', seed='case'):
    ctor, blocks, n_cls, drop, sd, loss, coarse, act, _, _, shape, _ = case_of(A, case)
    knobs(A, monkeypatch, blocks, drop if dropout == 'case' else dropout, sd if seed == 'case' else seed, loss, coarse, act)
    net = ctor()(shape, (n_cls,))
    net.engine().init_params(init)
    if net._net_kind != 'sr':
        perturb_routers(net)
    return net


def layers_of(net):
    """(λ, seed) of every leaf's Dropout layer, None without one, in net.leaves order."""
    out = []
    for ℓ in net.leaves:
        d = [c for c in ℓ.comps if type(c).__name__ == 'Dropout']
        out.append((d[0].hypers.λ, d[0].hypers.seed) if d else None)
    return out


def launch_list(eng, mode, n, **kw):
    p = eng.program(mode, n, **kw)
    return [(op.what, op.tag, len(op.host) if isinstance(op.host, list) else None) for op in list(p['fwd']) + list(p.get('bwd', []))]


def state_equal(a, b):
    ea, eb = a.engine(), b.engine()
    return torch.equal(ea.P, eb.P) and torch.equal(ea.A, eb.A) and torch.equal(ea.S, eb.S)


# ------------------------------------------------------------------ parity with the float64 oracle
@pytest.mark.parametrize('case', CASES)
def test_oracle_parity(spec, monkeypatch, case):
    from oracle import ref_net
    import arch_and_hypers as A0
    ctor, blocks, n_cls, drop, seed, loss, coarse, act, feeds, kv, shape, steps = case_of(A0, case)
    A, wrap = spec(shape)
    knobs(A, monkeypatch, blocks, drop, seed, loss, coarse, act)
    monkeypatch.setattr(ref_net, 'RefNet', R.RefNetDropout)            # (run_case imports it when it is called)
    seen = []

    def make(x0_shape, y_shape):
        net = wrap(ctor())(x0_shape, y_shape)
        seen.append(net)
        return net
    run_case(make, N, feeds, steps=steps, n_cls=n_cls, k_cpt_vec=kv)
    net, = seen
    eng = net.engine()
    assert eng.generic_exits == (n_cls > 16) and eng.generic_convs == (shape != SHAPE)
    assert net.dropout_step == steps and eng.has_dropout
    got = layers_of(net)
    assert any(got) and all(g is None or g[1] == seed for g in got)
    n_drop = sum(1 for g in got if g is not None)
    ops = {op.what: op for k in ('fwd', 'bwd') for op in eng.program('tr', N)[k]}
    assert len(ops['dropout_fwd'].host) == len(ops['dropout_bwd'].host) == n_drop
    if case == 'tree-ac':
        assert len(eng.blocks) == 15 and n_drop == 1 + 4 + 8 and max(len(ℓ.sinks) for ℓ in net.layers) == 3
    if case == 'ac-mixed':
        assert got == [(0.5, 3), (0.8, 3), None, (0.5, 3)]


# ------------------------------------------------------------------ λ = 1 and evaluation: bit for bit the net without the layer
def test_lambda_one_trains_as_the_net_without_the_layer(monkeypatch):
    import arch_and_hypers as A
    a, b = dropout_net(A, monkeypatch, 'ac', dropout=1.0), dropout_net(A, monkeypatch, 'ac', dropout=None)
    assert all(g == (1.0, 11) for g in layers_of(a)) and not any(layers_of(b))
    assert not a.engine().has_dropout and state_equal(a, b)
    assert launch_list(a.engine(), 'tr', N) == launch_list(b.engine(), 'tr', N)
    x0, y = _batch(SHAPE, N, seed=3)
    for t in range(3):
        for net in (a, b):
            net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0 / (1 + t)})
    torch.cuda.synchronize()
    assert state_equal(a, b) and bool(torch.isfinite(a.engine().P).all())
    assert a.dropout_step == b.dropout_step == 3


PROGRAMS = [('ev', {}), ('ev', dict(routed=1)), ('pr', {}), ('pr+p', {}), ('pr+p', dict(routed=1))]


@pytest.mark.parametrize('case', ['ac', 'ac-24', 'ac-mixed'])
def test_evaluation_and_predict_equal_the_net_without_the_layer(monkeypatch, case):
    import arch_and_hypers as A
    from test_predict_nets import host
    from test_routed_eval import snapshot
    a, b = dropout_net(A, monkeypatch, case), dropout_net(A, monkeypatch, case, dropout=None)
    assert any(layers_of(a)) and not any(layers_of(b)) and state_equal(a, b)
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
        assert [k[:2] for k in u['state']] == [k[:2] for k in v['state']] and u['state']
        assert all(np.array_equal(p, q) for p, q in zip(u['state'].values(), v['state'].values()))
    for u, v in list(zip(pa, pb)) + [(ga, gb)]:
        assert set(u) == set(v) and 'cls' in u
        for k in u:
            assert np.array_equal(u[k], v[k]), k
    for k in ('correct', 'ops', 'hist'):
        assert np.array_equal(getattr(ca, k), getattr(cb, k)), k
    assert a.dropout_step == 0                                 # (evaluation never moves the counter)
    for n in (N, 16, 256):
        for mode, kw in PROGRAMS:
            assert launch_list(a.engine(), mode, n, **kw) == launch_list(b.engine(), mode, n, **kw), (mode, kw, n)


@pytest.mark.parametrize('case,n', [('ac', N), ('ac', 256), ('ac', 1024), ('sr', N), ('ac-mixed', N), ('ac-24', N)])
def test_training_launch_list_differs_by_the_two_launches_and_the_lin_records(monkeypatch, case, n):
    import arch_and_hypers as A
    a, b = dropout_net(A, monkeypatch, case), dropout_net(A, monkeypatch, case, dropout=None)
    la, lb = launch_list(a.engine(), 'tr', n), launch_list(b.engine(), 'tr', n)
    n_drop = sum(1 for g in layers_of(a) if g is not None)
    routers = sum(1 for blk in a.engine().blocks if blk.drop is not None and blk.router is not None)
    extra = [x for x in la if x[0] in ('dropout_fwd', 'dropout_bwd')]
    assert [x[0] for x in extra] == ['dropout_fwd', 'dropout_bwd'] and all(x[2] == n_drop for x in extra)
    # the last block of a chain has no child: with the layer its BatchNorm-backward reduction is a launch of its own
    last_drop = [blk for blk in a.engine().blocks if blk.drop is not None and not blk.children and not a.engine().generic_exits]
    rest_a = [x for x in la if x[0] not in ('dropout_fwd', 'dropout_bwd')]
    rest_a_wo = [x for x in rest_a if x[0] != 'bn_bwd_reduce']
    rest_b_wo = [x for x in lb if x[0] != 'bn_bwd_reduce']
    assert len(rest_a) - len(rest_a_wo) == len(lb) - len(rest_b_wo) + len(last_drop)
    assert len(rest_a_wo) == len(rest_b_wo)
    for x, z in zip(rest_a_wo, rest_b_wo):
        if x[0] in ('lin_fwd', 'lin_bwd'):
            # one more record per exit that keeps a router beside its dropped head
            assert x[:2] == z[:2] and x[2] == z[2] + routers, (x, z)
        else:
            assert x == z
    # the order: dropout_fwd directly in front of lin_fwd, dropout_bwd directly behind lin_bwd
    names = [x[0] for x in la]
    assert names[names.index('lin_fwd') - 1] == 'dropout_fwd' and names[names.index('lin_bwd') + 1] == 'dropout_bwd'
    # the records: the head's reads xd as it is and leaves its dX in dxd; the router's keeps the block's map
    eng = a.engine()
    ops = {op.what: op for k in ('fwd', 'bwd') for op in eng.program('tr', n)[k]}
    from lib import _hip
    for dr in ops['dropout_fwd'].host:
        heads = [r for r in ops['lin_fwd'].host if r.a.x == dr.xd]
        assert len(heads) == 1 and heads[0].a.mode == _hip.ACT_IDENTITY and heads[0].w[0] and not heads[0].w[1]
        hb = [r for r in ops['lin_bwd'].host if r.a.x == dr.xd]
        assert len(hb) == 1 and hb[0].dx == dr.dxd and not hb[0].dz_out
        rb = [r for r in ops['lin_bwd'].host if r.a.x == dr.a.x]
        assert len(rb) == dr.accumulate and all(r.dx == dr.dx and not r.w[0] and r.w[1] for r in rb)
        assert dr.step == eng.drop_steps.data_ptr() and dr.n == n
        if case == 'ac':
            assert dr.thresh == R.thresh(0.5) == 1 << 31 and dr.inv_keep == 2.0 and (dr.seed_lo, dr.seed_hi) == (11, 0)


def test_multi_stream_schedule_refuses_the_layer(monkeypatch):
    import arch_and_hypers as A
    net = dropout_net(A, monkeypatch, 'ac')
    eng = net.engine()
    monkeypatch.setattr(eng, 'multi_stream', True)
    with pytest.raises(NotImplementedError, match='Dropout'):
        eng.program('tr', N)


# ------------------------------------------------------------------ K-step replay, the input pipeline
def resident_feed(net, t):
    e = net.engine()
    f = {net.x0: e.x0[:N], net.y: e.y[:N], net.mode: 'tr', net.λ_lrn: 0.05 / (1 + 0.3 * t)}
    if net._net_kind != 'sr':
        f[net.τ] = 1.0 / (1 + 0.1 * t)
    return f


def fill_inputs(nets, seed=3):
    x0, y = (torch.from_numpy(v).cuda() for v in _batch(SHAPE, N, seed=seed))
    for net in nets:
        e = net.engine()
        e.ensure_capacity(N)
        e.x0[:N].copy_(x0); e.y[:N].copy_(y)


def test_k_step_replay_equals_single_steps(monkeypatch):
    import arch_and_hypers as A
    a, b = (dropout_net(A, monkeypatch, 'ac') for _ in range(2))
    K = 4
    fill_inputs([a, b])
    for call in range(3):                                  # single steps (warm) | capture | replay
        ts = range(call * K, (call + 1) * K)
        a.train.run_steps([resident_feed(a, t) for t in ts])
        for t in ts:
            b.train.run(resident_feed(b, t))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(a.engine().P).all()), call
        assert state_equal(a, b), call
        assert a.dropout_step == b.dropout_step == (call + 1) * K
    assert any(k[0] == 'trK' and not isinstance(v, str) for k, v in a.engine()._graphs.items())
    # the masks did move from step to step: a net held at one step counter ends elsewhere
    c, d = (dropout_net(A, monkeypatch, 'ac') for _ in range(2))
    fill_inputs([c, d])
    for t in range(2):
        c.train.run(resident_feed(c, t))
        d.dropout_step = 0
        d.train.run(resident_feed(d, t))
    torch.cuda.synchronize()
    assert not state_equal(c, d)


def test_bound_input_pipeline_equals_the_array_fed_step(monkeypatch):
    import arch_and_hypers as A
    from lib.data import Dataset
    ds = Dataset.synthetic(n_tr=60, n_ts=20, seed=1)
    a, b = (dropout_net(A, monkeypatch, 'ac') for _ in range(2))
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
        assert state_equal(a, b), t
    # K steps through the pipeline's record slots == the same steps one by one
    c, d = (dropout_net(A, monkeypatch, 'ac') for _ in range(2))
    for net, seed in ((c, 5), (d, 5)):
        np.random.seed(seed)
        e = net.engine()
        xs, ys = ds.bind_engine(e, N)
        for rnd in range(3):
            ds.stage_training_draws_k(2, N, eng=e)
            feeds = [{net.x0: xs, net.y: ys, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0} for _ in range(2)]
            if net is c:
                net.train.run_steps(feeds)
            else:
                from lib._upload import run_one_by_one
                run_one_by_one(e, lambda f: e.run(f, True), feeds, True)
    torch.cuda.synchronize()
    assert state_equal(c, d) and c.dropout_step == d.dropout_step == 6


# ------------------------------------------------------------------ state
def test_long_lived_engine_equals_fresh_engines_with_the_step_set(monkeypatch):
    """A dozen operations on one engine -- training steps, K-step calls, evaluations dense and routed, predict, a forward
    pass in mode 'tr' -- and after each training operation a FRESH engine that starts from the state in front of it, with
    dropout_step set, ends in the same bits."""
    import arch_and_hypers as A
    rng = np.random.default_rng(17)
    live = dropout_net(A, monkeypatch, 'ac')
    fill_inputs([live])
    x_ev, y_ev = _batch(SHAPE, 16, seed=9)
    ops = list(rng.choice(['train', 'steps2', 'steps3', 'eval', 'routed', 'predict', 'fwd-tr'], 12))
    ops[0], ops[-1] = 'train', 'steps3'                      # (both ends train)
    t = 0
    fresh = {}                                               # one fresh net per operation kind (its graphs are its own)
    for k, op in enumerate(ops):
        fill_inputs([live])                                   # (eval and predict stage their images into the same buffers)
        torch.cuda.synchronize()
        before = [v.clone() for v in (live.engine().P, live.engine().A, live.engine().S)]
        step0 = live.dropout_step
        assert step0 == t
        if op == 'train':
            live.train.run(resident_feed(live, t)); steps = 1
        elif op.startswith('steps'):
            steps = int(op[-1])
            live.train.run_steps([resident_feed(live, t + j) for j in range(steps)])
        else:
            steps = 0
            if op == 'eval':
                live.eval({live.x0: x_ev, live.y: y_ev})
            elif op == 'routed':
                live.eval({live.x0: x_ev, live.y: y_ev}, routed=True)
            elif op == 'predict':
                live.predict(x_ev)
            else:
                live.eval({live.x0: live.engine().x0[:N], live.y: live.engine().y[:N], live.mode: 'tr', live.τ: 1.0})
            torch.cuda.synchronize()
            assert live.dropout_step == step0, op
            if op != 'fwd-tr':                                # (a forward pass in 'tr' moves the BatchNorm averages, as before)
                assert all(torch.equal(u, v) for u, v in zip(before, (live.engine().P, live.engine().A, live.engine().S))), op
            continue
        torch.cuda.synchronize()
        other = dropout_net(A, monkeypatch, 'ac', init=99)
        fill_inputs([other])
        eo = other.engine()
        for dst, src in zip((eo.P, eo.A, eo.S), before):
            dst.copy_(src)
        eo.invalidate_packs()
        other.dropout_step = step0
        for j in range(steps):                               # (a fresh engine: eager single steps)
            other.train.run(resident_feed(other, t + j))
        torch.cuda.synchronize()
        assert state_equal(live, other), (k, op)
        t += steps
    assert t >= 4


def test_seeds(monkeypatch):
    import arch_and_hypers as A
    a, b, c = dropout_net(A, monkeypatch, 'ac'), dropout_net(A, monkeypatch, 'ac'), dropout_net(A, monkeypatch, 'ac', seed=12)
    fill_inputs([a, b, c])
    for t in range(2):
        for net in (a, b, c):
            net.train.run(resident_feed(net, t))
    torch.cuda.synchronize()
    assert state_equal(a, b) and not state_equal(a, c)
    # a data-parallel rank draws with its own key (the host derives it): rank 1 of seed 11 is seed 11 + the stride, rank 0
    from lib._eng_common import dropout_seed
    ea = a.engine()
    ea.set_dropout_rank(1)
    recs = [r for op in ea.program('tr', N)['fwd'] if op.what == 'dropout_fwd' for r in op.host]
    want = R.rank_seed(11, 1)
    assert recs and all((r.seed_lo, r.seed_hi) == (want & 0xFFFFFFFF, want >> 32) for r in recs) and want == dropout_seed(11, 1)
    ea.set_dropout_rank(0)


@pytest.mark.parametrize('K', [2, 4])
def test_cotrained_nets_with_different_seeds_equal_their_solo_steps(monkeypatch, K):
    import arch_and_hypers as A
    from lib._co import CoTrainer
    knobs(A, monkeypatch, 3)

    def mk(i):
        ctor = A.ac_chain(k_cpt=A.k_cpts[i + 1])

        def make(x0_shape, y_shape):
            A.exit_dropout, A.dropout_seed = 0.5, 100 + i      # (read when the constructor is called; monkeypatch restores them)
            try:
                return ctor(x0_shape, y_shape)
            finally:
                A.exit_dropout, A.dropout_seed = None, 0
        return make
    co_nets, solo = _nets([mk(i) for i in range(K)]), _nets([mk(i) for i in range(K)])
    assert [layers_of(n)[0] for n in co_nets] == [(0.5, 100 + i) for i in range(K)]
    co = CoTrainer(co_nets)
    _compare_with_solo_steps(co_nets, solo, co.run, K, N)
    assert all(n.dropout_step == 4 for n in co_nets + solo)
    merged = {op.what: op for op in co._program(N)['ops']}
    for what in ('dropout_fwd', 'dropout_bwd'):
        recs = merged[what].host
        assert len(recs) == 3 * K and [r.seed_lo for r in recs] == [100 + i for i in range(K) for _ in range(3)]
        assert [r.step for r in recs] == [n.engine().drop_steps.data_ptr() for n in co_nets for _ in range(3)]


def test_k_joint_steps_in_one_graph_equal_k_joint_steps(monkeypatch):
    import arch_and_hypers as A
    from lib._co import CoTrainer
    knobs(A, monkeypatch, 3)

    def mk(i):
        ctor = A.ac_chain(k_cpt=A.k_cpts[i + 1])

        def make(x0_shape, y_shape):
            A.exit_dropout, A.dropout_seed = 0.5, 100 + i
            try:
                return ctor(x0_shape, y_shape)
            finally:
                A.exit_dropout, A.dropout_seed = None, 0
        return make
    a_nets, b_nets = _nets([mk(i) for i in range(2)]), _nets([mk(i) for i in range(2)])
    fill_inputs(a_nets + b_nets)
    co_a, co_b = CoTrainer(a_nets), CoTrainer(b_nets)
    S_ = 3
    for rnd in range(3):                                      # warm-up, capture + replay, replay
        co_a.run_steps([[resident_feed(net, rnd * S_ + j) for net in a_nets] for j in range(S_)])
        for j in range(S_):
            co_b.run([resident_feed(net, rnd * S_ + j) for net in b_nets])
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(a_nets, b_nets)):
            assert state_equal(a, b), (rnd, i)
            assert a.dropout_step == b.dropout_step == (rnd + 1) * S_
    assert any(k[0] == 'K' and not isinstance(v, str) for k, v in co_a._graphs.items() if isinstance(k, tuple)), 'no K-step graph was captured'


# ------------------------------------------------------------------ checkpoints and drivers
def test_checkpoint_keeps_lambda_and_the_seed(monkeypatch, tmp_path):
    import arch_and_hypers as A
    from lib.serdes import read_net, write_net
    net = dropout_net(A, monkeypatch, 'ac-mixed')
    x0, y = _batch(SHAPE, N, seed=3)
    feed = lambda m: {m.x0: x0, m.y: y, m.mode: 'tr', m.λ_lrn: 0.05, m.τ: 1.0}
    net.train.run(feed(net))
    path = str(tmp_path / 'net.npy')
    write_net(path, net, with_optimizer=True)
    back = read_net(path)
    assert layers_of(back) == layers_of(net) == [(0.5, 3), (0.8, 3), None, (0.5, 3)]
    back.dropout_step = net.dropout_step                    # (the counter is no part of a checkpoint)
    for m in (net, back):
        m.train.run(feed(m))
    torch.cuda.synchronize()
    for p, q in zip(net._all_params, back._all_params):
        if p.trainable:
            assert torch.equal(p.grad, q.grad), (p.owner.name, p.name)
    for ℓa, ℓb in zip(net.leaves, back.leaves):
        assert torch.equal(ℓa.c_err, ℓb.c_err) and torch.equal(ℓa.p_tr, ℓb.p_tr)


def test_drivers_run_with_exit_dropout(tmp_path):
    """train-nets and train-adaptive-nets --exit-dropout 0.5:2 --dropout-seed 3: the first two exits of net i carry the layer
    with seed 3 + i."""
    import os
    import subprocess
    import sys
    from lib.serdes import read_net
    from test_predict_nets import ROOT
    pkg = os.path.join(ROOT, 'multipath-nn_amd')
    out = str(tmp_path / 'nets')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '6', '--nets', '0', '1',
                          '--out', out, '--exit-dropout', '0.5:2', '--dropout-seed', '3'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    for i in range(2):
        net = read_net(os.path.join(out, 'cifar10-ac', '%04d.npy' % i))
        assert layers_of(net) == [(0.5, 3 + i)] * 2 + [None] * 6
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '4', '--nets', '0',
                          '--out', out, '--exit-dropout', '1.5'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 2 and b'--exit-dropout' in res.stderr
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-adaptive-nets'), 'hybrid-ac-dynkcpt', '--synthetic', '--iters', '5',
                          '--out', out, '--exit-dropout', '0.5:2', '--dropout-seed', '3'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    net = read_net(os.path.join(out, 'hybrid-ac-dynkcpt', 'net.npy'))
    assert layers_of(net) == [(0.5, 3)] * 2 + [None] * 6


# ------------------------------------------------------------------ the benchmark's net
def test_a_net_without_the_layer_has_the_launches_it_had():
    """bench.py's net (ac_chain on the spec's whole table, batch 128) has no Dropout: no launch of the layer, one lin record per
    exit shared by head and router, the last block's BatchNorm backward still fused into lin_bwd."""
    import arch_and_hypers as A
    assert A.exit_dropout is None and A.dropout_seed == 0
    net = A.ac_chain(k_cpt=0.0, seed=1234)(SHAPE, (10,))
    eng = net.engine()
    assert not eng.has_dropout and all(b.drop is None for b in eng.blocks)
    p = eng.program('tr', 128)
    ops = [op for op in list(p['fwd']) + list(p['bwd']) if op.what not in ('fork', 'join', 'bucket')]
    kinds = [op.what for op in ops]
    assert not any(k.startswith('dropout') or k == 'bn_bwd_reduce' for k in kinds)
    by = {op.what: op for op in ops}
    assert len(by['lin_fwd'].host) == len(by['lin_bwd'].host) == len(by['exit_tail_fwd'].host) == 8
    assert all(r.w[0] and (r.w[1] or k == 7) for k, r in enumerate(by['lin_fwd'].host))
    last = by['lin_bwd'].host[-1]
    assert last.dz_out and not last.dx
