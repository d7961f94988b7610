"""GPU: Net.predict(exit_conf=) -- the confidence-threshold exit policy -- on whole nets.

  * forced exits (-inf at leaf k, +inf elsewhere): every image leaves at k, `ops` is the integer sum of the operation
    counts along the path, and on the images the learnt router itself sends to k the answer is the ungated predict's, bit
    for bit;
  * real thresholds: from the forced runs' confidences the expected leaf is the first k with conf[k] >= tau_k -- leaf, cls,
    conf, probs and ops equal that bit for bit, dense and routed at every gather depth the test names, with per-exit and
    scalar thresholds taken from occurring confidences;
  * against the float64 oracle: leaf and cls equal wherever no oracle confidence on the path is within 1e-3 of its
    threshold and the top-two class gap exceeds 1e-3, probs within 2e-4 * (1 + max|ref|);
  * on other nets (a tree with 3-sink switches, any-width exits, the general conv kernels, dyn_k_cpt, gated beside ungated
    switches, superclass and squared exits) against a walk on the host over what the UNGATED programs computed: every
    head's answer for every image and the routers' outputs;
  * hipGraph replay with the thresholds changed between replays, predict_all from bytes, classify-images --exit-conf, the
    launch lists of exit_conf=None, eval -> predict(exit_conf) -> eval.

Everything but the oracle comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_predict_nets import KEYS, host, same_snapshot
from test_routed_eval import batch, calibrate_exit_fractions, make, randomise_routers, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')


def same(got, want, what=''):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def path_ops(eng, leaf):
    """The integer operation count of the path from the root to leaf `leaf` (block and router operations)."""
    nd, total = eng.leaves[leaf], 0
    while True:
        total += int(round(eng.node_ops_host[nd.idx]))
        if nd.parent < 0:
            return total
        nd = eng.nodes[nd.parent]


# ---------------------------------------------------------------------------------- A: the chain, forced exits and thresholds
@pytest.fixture(scope='module')
def chain():
    """The actor chain on 200 images, its routers calibrated to one eighth per exit; the ungated answer; the forced runs
    (everybody leaves at k), k = 0 .. 7.  Built once, shared, left unchanged."""
    from types import SimpleNamespace as Ns
    net = make('ac', k_cpt=1e-9)
    randomise_routers(net)
    x0, y = batch(200, seed=3)
    calibrate_exit_fractions(net, x0, y, [1 / 8] * 7)
    base = host(net.predict(x0, routed=False, probs=True))
    forced = [host(net.predict(x0, routed=False, probs=True, exit_conf=[-INF if j == k else INF for j in range(8)]))
              for k in range(8)]
    return Ns(net=net, x0=x0, y=y, base=base, forced=forced)


def test_forced_exits(chain):
    eng = chain.net.engine()
    assert np.array_equal(np.bincount(chain.base['leaf'], minlength=8), [25] * 8)
    for k, got in enumerate(chain.forced):
        assert (got['leaf'] == k).all(), k
        assert got['ops'].dtype == np.int64 and (got['ops'] == path_ops(eng, k)).all(), k
        own = chain.base['leaf'] == k                           # the images the learnt router itself sends to leaf k
        assert own.sum() == 25
        for key in ('cls', 'conf', 'probs', 'ops'):
            assert np.array_equal(got[key][own], chain.base[key][own]), (k, key)
        assert np.array_equal(got['conf'], got['probs'][np.arange(200), got['cls']])
    # the routed programs force the same exits (the deeper blocks then run on nobody)
    for k in (0, 3, 7):
        for mode in (True, 1, 3):
            got = host(chain.net.predict(chain.x0, routed=mode, probs=True, exit_conf=[-INF if j == k else INF for j in range(8)]))
            same(got, chain.forced[k], (k, mode))


def expected(chain, taus):
    """The first k with conf[k] >= tau_k (float32, as the forced runs report it); the last exit takes the rest."""
    n = len(chain.x0)
    leaf = np.full(n, 7)
    for k in range(6, -1, -1):
        if taus[k] is not None:
            leaf[chain.forced[k]['conf'] >= np.float32(taus[k])] = k
    ar = np.arange(n)
    return {key: np.stack([f[key] for f in chain.forced])[leaf, ar] for key in KEYS if key != 'leaf'} | {'leaf': leaf.astype(np.int32)}


def occurring_taus(chain, fraction=1 / 8):
    """Per exit, a confidence that OCCURS there (bit for bit) -- the one with which `fraction` of the batch leaves."""
    n = len(chain.x0)
    alive, taus = np.ones(n, bool), []
    for k in range(7):
        c = chain.forced[k]['conf']
        idx = np.flatnonzero(alive)
        tau = np.sort(c[idx])[::-1][int(round(fraction * n)) - 1]
        taus.append(float(tau))
        alive[idx[c[idx] >= tau]] = False
    return taus + [None]


@pytest.mark.parametrize('which', ['per-exit', 'scalar', 'entry-for-the-last-exit'])
def test_thresholds_dense_and_routed(chain, which):
    if which == 'per-exit':
        taus = occurring_taus(chain)
        call = taus
    elif which == 'scalar':                                   # one occurring value for every exit; the last entry is ignored
        call = float(np.sort(chain.forced[0]['conf'])[::-1][49])
        taus = [call] * 7 + [None]
    else:
        taus = occurring_taus(chain, 1 / 10)
        call = taus[:7] + [0.0]                               # (an entry for the last exit, which nothing gates: ignored)
    want = expected(chain, taus)
    hist = np.bincount(want['leaf'], minlength=8)
    assert (hist > 0).sum() >= 2 and not np.array_equal(want['leaf'], chain.base['leaf']), hist
    if which == 'per-exit':
        assert np.array_equal(hist, [25] * 8), hist           # (conf == tau leaves: the 25th image is the one whose conf is tau)
    for mode in (False, True, 1, 3, 'auto'):
        got = host(chain.net.predict(chain.x0, routed=mode, probs=True, exit_conf=call))
        same(got, want, (which, mode))
    assert (want['ops'] == np.array([path_ops(chain.net.engine(), l) for l in want['leaf']])).all()
    assert chain.net.predict(chain.x0, exit_conf=call).probs is None
    same(host(chain.net.predict(chain.x0, routed=False, probs=True)), chain.base, 'the ungated answer afterwards')


def test_zero_always_leaves_and_above_one_never(chain):
    got = host(chain.net.predict(chain.x0, probs=True, exit_conf=0.0))
    same(got, chain.forced[0], 'tau = 0')
    got = host(chain.net.predict(chain.x0, probs=True, exit_conf=-1))
    same(got, chain.forced[0], 'tau < 0')
    got = host(chain.net.predict(chain.x0, probs=True, exit_conf=np.nextafter(np.float32(1), np.float32(2))))
    same(got, chain.forced[7], 'tau > 1')
    got = host(chain.net.predict(chain.x0, probs=True, exit_conf=float('nan')))
    same(got, chain.forced[7], 'tau = NaN')


def test_eval_predict_eval(chain):
    net, feed = chain.net, {chain.net.x0: chain.x0, chain.net.y: chain.y}
    for mode in (False, 3):
        net.eval(feed, routed=mode)
        torch.cuda.synchronize()
        first = snapshot(net)
        net.predict(chain.x0, routed=mode, exit_conf=occurring_taus(chain))
        with pytest.raises(RuntimeError, match='predict'):
            net.state()
        net.eval(feed, routed=mode)
        torch.cuda.synchronize()
        same_snapshot(first, snapshot(net))


# ---------------------------------------------------------------------------------- B: against the float64 oracle
# Seed picked on the CPU (the oracle alone, on the parameters of make('ac', seed) + randomise_routers with the heads'
# LinTrans weights times HEAD_SCALE, thresholds as below): the images of the 200 with an oracle confidence on their path
# within 1e-3 of its threshold or a top-two class gap <= 1e-3 -- seeds 1 .. 12 give 2 to 34 of them; seed 11 gives 2 = 1.0 %.
ORACLE_SEED = 11
HEAD_SCALE = 4.0                # (the heads of an untrained net are close to uniform: spread the confidences, 0.19 .. 0.95)


def test_against_the_oracle():
    from oracle.ref_net import RefNet
    net = make('ac', seed=ORACLE_SEED, k_cpt=1e-9)
    randomise_routers(net)
    for ℓ in net.leaves:
        w = ℓ.comps[1].params.w
        w.assign(w.numpy() * HEAD_SCALE)
    x0, _ = batch(200, seed=3)
    n = len(x0)
    ref = RefNet(net)
    ref.load_params()
    res = ref.forward(x0, np.zeros((n, 10)), 'ev')
    leaves = list(net.leaves)
    probs = np.stack([res['out'][id(ℓ.comps[2])]['x'].detach().numpy() for ℓ in leaves])        # [leaf, image, class]
    conf = probs.max(2)
    # each threshold midway between two neighbouring oracle confidences: one eighth of the batch leaves per exit
    alive, taus, want = np.ones(n, bool), [], n // 8
    for k in range(7):
        idx = np.flatnonzero(alive)
        c = np.sort(conf[k][idx])[::-1]
        taus.append(0.5 * (c[want - 1] + c[want]))
        alive[idx[conf[k][idx] >= taus[k]]] = False
    leaf = np.full(n, 7)
    for k in range(6, -1, -1):
        leaf[conf[k] >= taus[k]] = k
    assert np.array_equal(np.bincount(leaf, minlength=8), [25] * 8)
    margin = np.full(n, np.inf)
    for k in range(7):
        margin = np.where(leaf >= k, np.minimum(margin, np.abs(conf[k] - taus[k])), margin)
    p_ref = probs[leaf, np.arange(n)]
    top = np.sort(p_ref, 1)
    sure = np.minimum(margin, top[:, -1] - top[:, -2]) > 1e-3
    print('oracle: %d of 200 images within 1e-3 of a decision' % (~sure).sum())
    assert (~sure).mean() <= 0.02
    for routed in (False, True):
        got = host(net.predict(x0, routed=routed, probs=True, exit_conf=[float(t) for t in taus] + [None]))
        assert np.array_equal(got['leaf'][sure], leaf[sure]) and np.array_equal(got['cls'][sure], p_ref.argmax(1)[sure])
        hit = got['leaf'] == leaf
        err = np.abs(got['probs'][hit] - p_ref[hit]).max()
        print('routed=%r: max |probs - oracle| %.3g' % (routed, err))
        assert err <= 2e-4 * (1 + np.abs(p_ref).max())


# ---------------------------------------------------------------------------------- C: other nets, against a walk on the host
def ungated_parts(net, x0, y, k_cpt=None, extra=None):
    """What the UNGATED programs compute, for every image: each switch's router outputs (the labelled evaluation) and
    every head's own answer (a dense predict runs every exit on every image and keeps the answers by leaf)."""
    eng = net.engine()
    n = len(x0)
    net.eval({net.x0: x0, net.y: y, **(extra or {})})
    torch.cuda.synchronize()
    r = {id(ℓ): ℓ.router.x.cpu().numpy().copy() for ℓ in net.layers if ℓ.router is not None}
    base = host(net.predict(x0, routed=False, probs=True, k_cpt=k_cpt))
    nl, cap, w = len(eng.leaves), eng.n_max, eng.n_cls_max
    heads = dict(cls=eng.pr_cls.view(nl, cap)[:, :n].cpu().numpy().copy(), conf=eng.pr_conf.view(nl, cap)[:, :n].cpu().numpy().copy(),
                 probs=eng.pr_p.view(nl, cap, w)[:, :n].cpu().numpy().copy())
    return r, heads, base


def walk(net, r, heads, taus, n):
    """The policy on the host: at a switch whose exit has a threshold, leave if conf >= tau, else the router's arg-max
    among the other sinks; at any other switch the router's arg-max; first index on ties."""
    eng = net.engine()
    index = {id(ℓ): k for k, ℓ in enumerate(net.leaves)}
    node = {id(nd.layer): nd for nd in eng.nodes}
    out = dict(leaf=np.zeros(n, np.int32), cls=np.zeros(n, np.int32), conf=np.zeros(n, np.float32), ops=np.zeros(n, np.int64),
               probs=np.zeros((n, eng.n_cls_max), np.float32))
    for s in range(n):
        ℓ, ops = net.root, 0
        while True:
            ops += int(round(eng.node_ops_host[node[id(ℓ)].idx]))
            if not ℓ.sinks:
                break
            if len(ℓ.sinks) == 1:
                ℓ = ℓ.sinks[0]
                continue
            row = r[id(ℓ)][s]
            exits = [i for i, k in enumerate(ℓ.sinks) if not k.sinks]
            cand = list(range(len(ℓ.sinks)))
            if exits and taus[index[id(ℓ.sinks[exits[0]])]] is not None:
                L = index[id(ℓ.sinks[exits[0]])]
                if heads['conf'][L][s] >= np.float32(taus[L]):
                    ℓ = ℓ.sinks[exits[0]]
                    continue
                cand.remove(exits[0])
            best = cand[0]
            for i in cand[1:]:
                if row[i] > row[best]:
                    best = i
            ℓ = ℓ.sinks[best]
        L = index[id(ℓ)]
        out['leaf'][s], out['cls'][s], out['conf'][s], out['ops'][s] = L, heads['cls'][L][s], heads['conf'][L][s], ops
        out['probs'][s] = heads['probs'][L][s]
    return out


def median_taus(net, heads, skip=()):
    """Per gateable exit a confidence that occurs there (the median over the batch); None for the others and for `skip`."""
    gate = set(net.gateable_leaves) - set(skip)
    return [float(np.sort(heads['conf'][k])[len(heads['conf'][k]) // 2]) if k in gate else None for k in range(len(heads['conf']))]


def check_gate(net, x0, y, modes, taus=None, skip=(), k_cpt=None, extra=None, min_leaves=2):
    n = len(x0)
    feed = {net.x0: x0, net.y: y, **(extra or {})}
    r, heads, base = ungated_parts(net, x0, y, k_cpt, extra)
    same(walk(net, r, heads, [None] * len(heads['conf']), n), base, 'the walk with no threshold is the ungated predict')
    taus = median_taus(net, heads, skip) if taus is None else taus
    want = walk(net, r, heads, taus, n)
    assert len(set(want['leaf'].tolist())) >= min_leaves and not np.array_equal(want['leaf'], base['leaf'])
    net.eval(feed)
    torch.cuda.synchronize()
    first = snapshot(net)
    for mode in (False,) + tuple(modes):
        got = host(net.predict(x0, routed=mode, probs=True, k_cpt=k_cpt, exit_conf=taus))
        same(got, want, mode)
    net.eval(feed)
    torch.cuda.synchronize()
    same_snapshot(first, snapshot(net))
    same(host(net.predict(x0, routed=False, probs=True, k_cpt=k_cpt)), base, 'ungated afterwards')
    return want, taus, heads, r


def test_tree_with_three_sink_switches():
    """ac_tree: under a gated 3-sink switch the router still picks the child -- both children of such switches are taken."""
    from test_predict_nets import spread_over_leaves, tree_net
    net = tree_net()
    eng = net.engine()
    eng.init_params(13)
    rng = np.random.default_rng(14)
    for p in net._all_params:
        if not p.trainable:
            p.assign(rng.random(p.shape) * 0.5 + (0.75 if p.name == 'v_avg' else -0.25))
    randomise_routers(net, seed=3, scale=1.0)
    x0, y = batch(96, seed=12)
    net.eval({net.x0: x0, net.y: y})
    r0 = {id(ℓ): ℓ.router.x.cpu().numpy().copy() for ℓ in net.switches}
    spread_over_leaves(net, lambda ℓ: r0[id(ℓ)], 96)
    want, taus, heads, r = check_gate(net, x0, y, modes=(True, 1, 2), min_leaves=5)
    root = net.root.sinks[0]
    assert len(root.sinks) == 3 and not root.sinks[0].sinks
    stay = want['leaf'] != 0                                   # images the root switch's threshold does not take
    right_of = lambda s: r[id(root)][s, 2] > r[id(root)][s, 1]
    sides = {bool(right_of(s)) for s in np.flatnonzero(stay)}
    assert 5 < stay.sum() < 96 and sides == {False, True}


def small_chain(monkeypatch, blocks=3, n_cls=10, seed=1234, **hyp):
    import arch_and_hypers as A
    from test_net_parity import perturb_routers
    monkeypatch.setattr(A, 'arch', A.arch[:blocks])
    net = A.ac_chain(**({'k_cpt': 1.6e-8} | hyp))((32, 32, 3), (n_cls,))
    net.engine().init_params(seed)
    perturb_routers(net)
    return net


def test_any_width_exits_24_classes(monkeypatch):
    from test_net_parity import batch as batch_c
    net = small_chain(monkeypatch, n_cls=24)
    assert net.engine().generic_exits
    x0, y = batch_c(70, 3, 24, seed=2)
    want, *_ = check_gate(net, x0, y, modes=(True, 1, 2, 'auto'), min_leaves=3)
    assert want['probs'].shape == (70, 24)


def test_general_conv_kernels_supp_5(monkeypatch):
    import arch_and_hypers as A
    from test_conv_gen_nets import _net5
    monkeypatch.setattr(A, 'conv_supp', 5)
    monkeypatch.setattr(A, 'arch', A.arch[:4])
    net = _net5(A)
    assert net.engine().generic_convs
    x0, y = batch(40, seed=3)
    check_gate(net, x0, y, modes=(True, 1, 3), min_leaves=3)


def test_dyn_k_cpt(monkeypatch):
    net = small_chain(monkeypatch, dyn_k_cpt=True, k_cpt=0.0, seed=3)
    x0, y = batch(70, seed=6)
    kc = np.random.default_rng(1).choice([1e-9, 6.4e-8], 70).astype(np.float32)
    check_gate(net, x0, y, modes=(True, 1), k_cpt=kc, extra={net.k_cpt: kc}, min_leaves=3)
    with pytest.raises(ValueError, match='k_cpt'):
        net.predict(x0, exit_conf=0.5)


def test_gated_beside_ungated_switches(monkeypatch):
    """None leaves a switch to its router: the gated program holds records for the other switches only."""
    net = small_chain(monkeypatch, blocks=4)
    x0, y = batch(64, seed=5)
    calibrate_exit_fractions(net, x0, y, [1 / 4] * 3)
    want, taus, *_ = check_gate(net, x0, y, modes=(True, 1, 2), skip=(1,), min_leaves=3)
    assert taus[1] is None and taus[3] is None and taus[0] is not None and taus[2] is not None
    eng = net.engine()
    for routed in (False, 1, 2):
        prog = eng.program('pr', 64, routed, gate=frozenset({0, 2}))
        gates = [q for op in prog['fwd'] if op.what == 'conf_gate' for q in op.host]
        assert len(gates) == 2 and prog['gate'] == frozenset({0, 2})
        recs = [e for op in prog['fwd'] if op.what == 'exit_ev' for e in op.host]
        plain = [e for op in eng.program('pr', 64, routed)['fwd'] if op.what == 'exit_ev' for e in op.host]
        assert len(recs) == len(plain) == 4
        for j, (e, p) in enumerate(zip(recs, plain)):
            if j in (0, 2):                                    # gated: the exit record lost its child lists to the gate record
                assert not any(e.child_idx) and not any(e.child_cnt)
                q = gates[j // 2]
                assert list(q.child_idx) == list(p.child_idx) and list(q.child_cnt) == list(p.child_cnt)
                assert (q.idx, q.cnt, q.r, q.exit_sink, q.n_sinks) == (p.idx, p.cnt, p.r, 0, 2)
            else:
                assert bytes(e) == bytes(p)


def test_superclass_and_squared_exits(monkeypatch):
    """Exit 0 squared (softmax), exit 1 two superclasses, exit 2 squared-linear (the comparison is on the raw output that
    predict reports as conf), exit 3 plain."""
    import arch_and_hypers as A
    from lib import _hip
    from test_squared_error_nets import kinds_of, squared_net
    net = squared_net(A, monkeypatch, 'ac-mixed')
    assert kinds_of(net) == [_hip.LOSS_SQ, _hip.LOSS_CE, _hip.LOSS_SQ_LIN, _hip.LOSS_CE] and net.leaf_n_cls == [10, 2, 10, 10]
    x0, y = batch(64, seed=3)
    want, taus, heads, _ = check_gate(net, x0, y, modes=(True, 1, 2), min_leaves=3)
    raw = heads['conf'][2]
    assert (want['leaf'] == 2).any() and (np.abs(heads['probs'][2].astype(np.float64).sum(1) - 1) > 1e-3).any()
    assert np.array_equal(want['leaf'] == 2, (want['leaf'] >= 2) & (raw >= np.float32(taus[2])))


# ---------------------------------------------------------------------------------- D: graphs, streams, the driver, launch lists
def test_graph_replay_with_changed_thresholds():
    """The thresholds are values in device memory: ONE captured program serves a sweep, and gives a fresh engine's bits."""
    def build():
        net = make(seed=31)
        randomise_routers(net, seed=3, scale=1.0)
        return net
    net = build()
    eng = net.engine()
    assert eng.use_graph
    xa, xb = batch(256, seed=1)[0], batch(256, seed=2)[0]
    # thresholds from the first exit's own confidences (tau = 0: everybody leaves there): three quarters, half, a quarter leave
    c0 = np.sort(host(net.predict(xb, routed=False, exit_conf=0.0))['conf'])
    t1, t2, t3 = (float(c0[i]) for i in (64, 128, 192))
    got = []
    for x, tau in zip((xa, xb, xa, xb), (0.5, t1, t2, t3)):                        # (eager, capture, replay, replay)
        got.append(host(net.predict(x, routed=True, probs=True, exit_conf=tau)))
    full = frozenset(range(7))
    keys = [k for k, g in eng._graphs.items() if k[0] == 'pr+p' and not isinstance(g, str)]
    assert len(keys) == 1 and keys[0][-1] == full and len([k for k in eng._progs if k[0] == 'pr+p']) == 1
    fresh = build()
    for g, x, tau in zip(got[1:], (xb, xa, xb), (t1, t2, t3)):
        same(g, host(fresh.predict(x, routed=True, probs=True, exit_conf=tau)), tau)
    assert [int((g['leaf'] == 0).sum()) for g in (got[1], got[3])] == [192, 64] and len(set(got[3]['leaf'].tolist())) >= 2
    # another gated set (another program) and the ungated program live beside it
    some = [t2, None, t2, t2, None, t2, t2, None]
    mixed = host(net.predict(xb, routed=True, probs=True, exit_conf=some))
    same(mixed, host(fresh.predict(xb, routed=True, probs=True, exit_conf=some)), 'mixed')
    same(host(net.predict(xb, routed=True, probs=True)), host(fresh.predict(xb, routed=True, probs=True)), 'ungated')
    same(host(net.predict(xb, routed=True, probs=True, exit_conf=t3)), got[3], 'replay after the others')


def test_predict_all_from_bytes_equals_chunked_predict():
    net = make(seed=31)
    randomise_routers(net, seed=3, scale=1.0)
    x = np.random.default_rng(4).integers(0, 256, (150, 32, 32, 3), dtype=np.uint8)
    m = float(np.median(host(net.predict(x[:64], decode='unit', exit_conf=0.0))['conf']))      # (a confidence that occurs at exit 0)
    tau = [m, m, None, m, m, m, m, 0.5]
    parts = [host(net.predict(x[i:i + 64], probs=True, decode='unit', exit_conf=tau)) for i in range(0, 150, 64)]
    want = {k: np.concatenate([p[k] for p in parts]) for k in KEYS}
    got = host(net.predict_all(x, batch=64, probs=True, decode='unit', exit_conf=tau))
    same(got, want)
    plain = host(net.predict_all(x, batch=64, probs=True, decode='unit'))
    assert not np.array_equal(plain['leaf'], got['leaf']) and len(set(got['leaf'].tolist())) >= 2


def test_classify_images_exit_conf(tmp_path):
    from lib.serdes import read_net, write_net
    net = make(seed=31)
    randomise_routers(net, seed=3, scale=1.0)
    ckpt = str(tmp_path / 'net.npy')
    write_net(ckpt, net)
    x = np.random.default_rng(5).random((100, 32, 32, 3)).astype(np.float32)
    np.savez(str(tmp_path / 'images.npz'), x=x)
    pred = str(tmp_path / 'pred.npz')
    tau = float(np.median(host(net.predict(x, exit_conf=0.0))['conf']))          # (a confidence that occurs at exit 0)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'multipath-nn_amd', 'classify-images'), ckpt, str(tmp_path / 'images.npz'),
                          '--out', pred, '--batch', '64', '--probs', '--exit-conf', repr(tau)], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    text = res.stdout.decode()
    hist = [int(v) for v in text.split('exit histogram:')[1].splitlines()[0].split()]
    got = np.load(pred)
    want = host(read_net(ckpt).predict_all(x, batch=64, probs=True, exit_conf=tau))
    same(got, want)
    assert np.array_equal(np.bincount(got['leaf'], minlength=8), hist) and (np.array(hist) > 0).sum() >= 2
    assert not np.array_equal(want['leaf'], host(net.predict(x, probs=True))['leaf'])


def test_launch_lists_of_the_default_path(chain):
    """exit_conf=None: the programs hold no gate launch and are the cached ungated ones; a gated program is the ungated one
    with one gate launch behind each exit launch that holds a gated switch."""
    eng = chain.net.engine()
    for mode in ('pr', 'pr+p'):
        for routed in (False, 1, 3, 8):
            plain = eng.program(mode, 200, routed)
            assert plain is eng.program(mode, 200, routed, gate=frozenset()) and plain['gate'] == frozenset()
            whats = [op.what for op in plain['fwd']]
            assert 'conf_gate' not in whats
            gated = eng.program(mode, 200, routed, gate=frozenset(range(7)))
            gw = [op.what for op in gated['fwd']]
            assert [w for w in gw if w != 'conf_gate'] == whats
            exits = [i for i, w in enumerate(gw) if w == 'exit_ev']
            # (the last block's exit has no router: an exit launch that holds only that one gets no gate launch)
            follow = [gw[i + 1] == 'conf_gate' for i in exits]
            assert sum(follow) == gw.count('conf_gate') >= 1 and all(follow[:-1])
            assert sum(len(op.host) for op in gated['fwd'] if op.what == 'conf_gate') == 7
            assert gw.index('route') > max(i for i, w in enumerate(gw) if w == 'conf_gate')
            if 'ev_prefix_walk' in gw:
                assert gw[gw.index('ev_prefix_walk') - 1] == 'conf_gate'
    assert not any(op.what == 'conf_gate' for op in eng.program('ev', 200, 3)['fwd'])
