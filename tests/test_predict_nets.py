"""GPU: Net.predict -- the label-free evaluation -- on whole nets.

  * consistent with the labelled evaluation, per sample and exactly: (cls == arg-max y) is `acc`, leaf is the leaf whose
    p_ev is 1, ops is the float64 sum behind `moc`; the engine's label buffer holds NaN while predict runs;
  * routed == dense, bit for bit, in cls, leaf, ops, conf, probs, at every gather depth the test names;
  * eval -> predict -> eval gives the first eval's bits again; state() after predict raises;
  * against the float64 oracle: leaf and cls equal wherever the oracle's router margins on the sample's path and its
    top-two class gap at its leaf exceed 1e-3 (at most 2 % of the batch may fall short), the softmax row at the taken
    leaf within 2e-4 * (1 + max|ref|) (the bound of tests/test_routed_eval.py:check_vs_oracle);
  * tuned and general conv kernels, tuned and any-width exits, chains and a tree, dyn_k_cpt, a statically routed chain,
    hipGraph replay on new images, and the classify-images driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_routed_eval import batch, calibrate_exit_fractions, make, randomise_routers, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('cls', 'leaf', 'ops', 'conf', 'probs')


def host(res):
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy().copy() for k in KEYS if getattr(res, k) is not None}


def same_snapshot(a, b):
    for grp in ('p_ev', 'c_err', 'd_cor', 'r', 'state'):
        assert a[grp].keys() == b[grp].keys()
        for k in a[grp]:
            assert np.array_equal(a[grp][k], b[grp][k]), (grp, k)


def predict_poisoned(net, x0, **kw):
    """predict with NaN in the engine's label buffer: nothing of the result may come from it."""
    eng = net.engine()
    eng.ensure_capacity(len(x0), train=False)
    eng.y.fill_(float('nan'))
    return host(net.predict(x0, **kw))


def check_consistent(net, x0, y, modes, every_leaf=True, min_leaves=2, extra=None, k_cpt=None):
    """The checks of a whole net: predict against the labelled evaluation, routed against dense, eval -> predict -> eval."""
    eng = net.engine()
    feed = {net.x0: x0, net.y: y, **(extra or {})}
    n = len(x0)
    net.eval(feed)
    torch.cuda.synchronize()
    first = snapshot(net)
    acc = net.state()[(net, 'acc')].cpu().numpy()
    pev = np.stack([first['p_ev'][nd.idx] for nd in eng.nodes])
    leaf_rows = pev[[nd.idx for nd in eng.leaves]]
    assert ((leaf_rows == 1).sum(0) == 1).all()                   # (dynamic nets: every sample leaves at exactly one exit)
    want_leaf = leaf_rows.argmax(0)
    taken = len(set(want_leaf.tolist()))
    assert taken == len(eng.leaves) if every_leaf else taken >= min_leaves, np.bincount(want_leaf, minlength=len(eng.leaves))
    want_ops = (pev.astype(np.float64) * np.array(eng.node_ops_host, np.float64)[:, None]).sum(0)

    dense = predict_poisoned(net, x0, routed=False, probs=True, k_cpt=k_cpt)
    assert np.array_equal(dense['cls'] == y.argmax(1), acc == 1) and set(np.unique(acc)) <= {0.0, 1.0}
    assert np.array_equal(dense['leaf'], want_leaf)
    assert dense['ops'].dtype == np.int64 and np.array_equal(dense['ops'].astype(np.float64), want_ops)
    assert dense['cls'].dtype == np.int32 and dense['leaf'].dtype == np.int32
    ar = np.arange(n)
    assert np.array_equal(dense['conf'], dense['probs'][ar, dense['cls']])
    assert np.array_equal(dense['probs'].argmax(1), dense['cls'])
    assert np.abs(dense['probs'].astype(np.float64).sum(1) - 1).max() < 1e-5
    with pytest.raises(RuntimeError, match='predict'):
        net.state()
    assert net.predict(x0, routed=False, k_cpt=k_cpt).probs is None
    for mode in modes:
        got = predict_poisoned(net, x0, routed=mode, probs=True, k_cpt=k_cpt)
        for k in KEYS:
            assert np.array_equal(got[k], dense[k]), (mode, k)
    net.eval(feed)
    torch.cuda.synchronize()
    same_snapshot(first, snapshot(net))
    return dense


# ---------------------------------------------------------------------------------- A: the chains on the tuned kernels
@pytest.fixture(scope='module')
def chains():
    """kind -> (net, x0, y): 200 images, one eighth of them leaving at each exit (built once, shared, left unchanged)."""
    out = {}
    for kind in ('ac', 'cr'):
        net = make(kind, k_cpt=1e-9)
        randomise_routers(net)
        x0, y = batch(200, seed=3)
        calibrate_exit_fractions(net, x0, y, [1 / 8] * 7)
        out[kind] = (net, x0, y)
    return out


@pytest.mark.parametrize('kind', ['ac', 'cr'])
def test_chain_predict_is_consistent_with_eval(chains, kind):
    net, x0, y = chains[kind]
    dense = check_consistent(net, x0, y, modes=(True, 1, 3, 'auto'))
    assert np.array_equal(np.bincount(dense['leaf'], minlength=8), [25] * 8)


# ---------------------------------------------------------------------------------- B: against the float64 oracle
# Seeds picked on the CPU (the oracle alone, on the parameters of make(kind, seed) + randomise_routers, calibrated as
# below): the images of the 200 whose smallest margin is <= 1e-3 -- seeds 1 .. 59 give 4 to 27 of them (mostly near-ties of
# the top two classes: the heads of an untrained net are close to uniform); seed 33 gives 4 = 2.0 %, for both net types
# (the actor and the critic chain draw the same parameters from a seed).
ORACLE_SEED = {'ac': 33, 'cr': 33}


def oracle_calibrate(net, ref, x0, fractions):
    """calibrate_exit_fractions from the ORACLE's router outputs (a router's output does not depend on the routing above
    it, so one forward pass serves every exit): the decision thresholds sit midway between two samples' margins."""
    res = ref.forward(x0, np.zeros((len(x0), 10)), 'ev')
    alive = np.ones(len(x0), bool)
    for k, ℓ in enumerate(net.switches):
        r = res['out'][id(ℓ.router)]['x'].detach().numpy()
        want = int(round(fractions[k] * len(x0)))
        margin = r[:, 1] - r[:, 0]
        idx = np.flatnonzero(alive)
        order = idx[np.argsort(margin[idx], kind='stable')]
        shift = 0.5 * (margin[order[want - 1]] + margin[order[want]])
        b = ℓ.router.comps[-1].params.b
        v = b.numpy().copy()
        v[0] += shift
        b.assign(v)
        alive[order[:want]] = False
    ref.load_params()


def oracle_answer(net, ref, x0):
    """leaf, cls, softmax row at the leaf and the smallest margin (routers on the path, top-two class gap), per image."""
    res = ref.forward(x0, np.zeros((len(x0), 10)), 'ev')
    R = lambda ℓ: res['out'][id(ℓ)]
    n = len(x0)
    leaves = list(net.leaves)
    leaf = np.full(n, -1)
    for l in range(len(leaves) - 1, -1, -1):
        leaf[R(leaves[l])['p_ev'].numpy() == 1] = l
    probs = np.stack([R(ℓ.comps[2])['x'].detach().numpy() for ℓ in leaves])[leaf, np.arange(n)]
    top = np.sort(probs, 1)
    margin = top[:, -1] - top[:, -2]
    for ℓ in net.switches:
        r = np.sort(R(ℓ.router)['x'].detach().numpy(), 1)
        on_path = R(ℓ)['p_ev'].numpy() == 1
        margin = np.where(on_path, np.minimum(margin, r[:, -1] - r[:, -2]), margin)
    return leaf, probs.argmax(1), probs, margin


@pytest.mark.parametrize('kind', ['ac', 'cr'])
def test_chain_predict_against_the_oracle(kind):
    from oracle.ref_net import RefNet
    net = make(kind, seed=ORACLE_SEED[kind], k_cpt=1e-9)
    randomise_routers(net)
    x0, _ = batch(200, seed=3)
    ref = RefNet(net)
    ref.load_params()
    oracle_calibrate(net, ref, x0, [1 / 8] * 7)
    leaf, cls, probs, margin = oracle_answer(net, ref, x0)
    sure = margin > 1e-3
    print('oracle: %d of 200 images within 1e-3 of a decision' % (~sure).sum())
    assert (~sure).mean() <= 0.02
    for routed in (False, True):
        got = predict_poisoned(net, x0, routed=routed, probs=True)
        assert np.array_equal(got['leaf'][sure], leaf[sure]) and np.array_equal(got['cls'][sure], cls[sure])
        same = got['leaf'] == leaf
        err = np.abs(got['probs'][same] - probs[same]).max()
        print('routed=%r: max |probs - oracle| %.3g' % (routed, err))
        assert err <= 2e-4 * (1 + np.abs(probs).max())


# ---------------------------------------------------------------------------------- C: any-width exits
def test_wide_exits_100_classes():
    from lib.net_types import ActorNet
    from test_net_parity import _wide_chain, batch as batch_c, perturb_routers
    net = _wide_chain(ActorNet, (32, 32), k_cpt=1.6e-8)((32, 32, 3), (100,))
    eng = net.engine()
    assert eng.generic_exits
    eng.init_params(5)
    perturb_routers(net)
    rng = np.random.default_rng(8)
    for p in net._all_params:
        if not p.trainable:
            p.assign(rng.random(p.shape) * 0.5 + (0.75 if p.name == 'v_avg' else -0.25))
    for ℓ in net.switches:
        last = ℓ.router.comps[-1].params
        last.w.assign(rng.standard_normal(last.w.shape) * 2.0)
    x0, y = batch_c(70, 3, 100, seed=2)
    calibrate_exit_fractions(net, x0, y, [1 / 4] * 3)
    dense = check_consistent(net, x0, y, modes=(True, 1, 3, 'auto'))
    assert dense['probs'].shape == (70, 100)


# ---------------------------------------------------------------------------------- D: the general conv kernels
def _calibrated(net, x0, y):
    randomise_routers(net)
    calibrate_exit_fractions(net, x0, y, [1 / 8] * 7)


def test_conv_supp_5_chain(monkeypatch):
    import arch_and_hypers as A
    from test_conv_gen_nets import _net5
    monkeypatch.setattr(A, 'conv_supp', 5)
    net = _net5(A)
    assert net.engine().generic_convs and not net.engine().anymap_convs
    x0, y = batch(40, seed=3)
    _calibrated(net, x0, y)
    check_consistent(net, x0, y, modes=(True, 1, 3, 'auto'))


def test_24x40_chain(monkeypatch):
    import arch_and_hypers as A
    from test_rect_nets import SHAPE, _batch, _net5
    monkeypatch.setattr(A, 'conv_supp', 5)
    net = _net5(A)
    assert net.engine().anymap_convs
    x0, y = _batch(SHAPE, 40, seed=3)
    _calibrated(net, x0, y)
    check_consistent(net, x0, y, modes=(True, 1, 3, 'auto'))


# ---------------------------------------------------------------------------------- E: a tree
def spread_over_leaves(net, r_of, n):
    """Shift the routers' last biases so that EVERY leaf of a tree is taken: top-down, each switch sends the samples that
    reach it on in proportion to the leaves below each sink (r_of(ℓ): the router outputs [n, sinks] of switch ℓ for every
    sample -- they do not depend on the routing above).  Per switch the shifts are found sink by sink, cyclically: the
    shift of sink i is put midway between two samples' margins so that exactly its quota of samples prefers it."""
    from lib.net_types import n_leaves

    def visit(ℓ, reach):
        if len(ℓ.sinks) < 2:
            for s in ℓ.sinks:
                visit(s, reach)
            return
        r = np.asarray(r_of(ℓ), np.float64)[reach]
        m, S = len(reach), len(ℓ.sinks)
        w = np.array([n_leaves(s) for s in ℓ.sinks], np.float64)
        assert m >= w.sum(), (m, w)
        quota = np.floor(m * w / w.sum()).astype(int)
        for i in np.argsort(-(m * w / w.sum() - quota), kind='stable')[:m - quota.sum()]:
            quota[i] += 1
        shift = np.zeros(S)
        for _ in range(200):
            if np.array_equal(np.bincount((r + shift).argmax(1), minlength=S), quota):
                break
            for i in range(S):
                others = np.delete(r + shift, i, 1).max(1)
                margin = np.sort(r[:, i] - others)[::-1]               # sample prefers sink i iff margin + shift_i > 0
                shift[i] = -0.5 * (margin[quota[i] - 1] + margin[quota[i]])
        arg = (r + shift).argmax(1)
        assert np.array_equal(np.bincount(arg, minlength=S), quota), (quota, np.bincount(arg, minlength=S))
        b = ℓ.router.comps[-1].params.b
        b.assign(b.numpy() + shift)
        for i, s in enumerate(ℓ.sinks):
            visit(s, reach[arg == i])
    visit(net.root, np.arange(n))


def tree_net():
    import arch_and_hypers as A
    net = A.ac_tree(k_cpt=1e-9)((32, 32, 3), (10,))
    return net


def test_tree():
    """ac_tree: 47 leaves, 96 samples -- the routers are arranged so that every leaf is taken (two samples each, three at
    two of them)."""
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
    r = {id(ℓ): ℓ.router.x.cpu().numpy().copy() for ℓ in net.switches}
    spread_over_leaves(net, lambda ℓ: r[id(ℓ)], 96)
    dense = check_consistent(net, x0, y, modes=(True, 2))
    assert len(eng.leaves) == 47 and np.bincount(dense['leaf'], minlength=47).min() >= 1


# ---------------------------------------------------------------------------------- F: dyn_k_cpt
def _calibrate_with_feed(net, feed, fractions):
    """calibrate_exit_fractions for a net whose feed holds more than x0 and y (the per-sample k_cpt)."""
    net.eval(feed)
    n = len(feed[net.x0])
    alive = np.ones(n, bool)
    for k, ℓ in enumerate(net.switches):
        r = ℓ.router.x.cpu().numpy().astype(np.float64)
        want = int(round(fractions[k] * n))
        margin = r[:, 1] - r[:, 0]
        idx = np.flatnonzero(alive)
        order = idx[np.argsort(margin[idx], kind='stable')]
        b = ℓ.router.comps[-1].params.b
        v = b.numpy().copy()
        v[0] += 0.5 * (margin[order[want - 1]] + margin[order[want]])
        b.assign(v)
        alive[order[:want]] = False


def test_dyn_k_cpt():
    import arch_and_hypers as A
    net = A.ac_chain(dyn_k_cpt=True)((32, 32, 3), (10,))
    net.engine().init_params(3)
    randomise_routers(net, seed=4, scale=1.0)
    # (the k_cpt column of the routers' first map starts at zero: give it weight, so that k_cpt moves the routing)
    rng = np.random.default_rng(6)
    for ℓ in net.switches:
        w = ℓ.router.comps[1].params.w
        v = w.numpy().copy()
        v[-1] = rng.standard_normal(v.shape[1]) * 3.0
        w.assign(v)
    x0, y = batch(70, seed=6)
    _calibrate_with_feed(net, {net.x0: x0, net.y: y, net.k_cpt: np.full(70, 1e-9, np.float32)}, [1 / 8] * 7)
    leaves = []
    for v, spread in ((1e-9, 8), (6.4e-8, 1)):                    # (calibrated at the first value: one eighth per exit there)
        kc = np.full(70, v, np.float32)
        dense = check_consistent(net, x0, y, modes=(True, 1), every_leaf=False, min_leaves=spread, extra={net.k_cpt: kc}, k_cpt=v)
        leaves.append(dense['leaf'])
    assert not np.array_equal(*leaves)                            # (the two values route differently: k_cpt is really read)
    with pytest.raises(ValueError, match='k_cpt'):
        net.predict(x0)
    static = make()
    with pytest.raises(ValueError, match='k_cpt'):
        static.predict(x0, k_cpt=1e-9)


# ---------------------------------------------------------------------------------- G: a statically routed chain
def test_sr_chain():
    import arch_and_hypers as A
    net = A.sr_chain(3)((32, 32, 3), (10,))
    eng = net.engine()
    eng.init_params(2)
    x0, y = batch(37, seed=1)
    net.eval({net.x0: x0, net.y: y})
    acc = net.state()[(net, 'acc')].cpu().numpy()
    ops = sum(eng.node_ops_host)
    for routed in (False, True, 'auto'):
        got = predict_poisoned(net, x0, routed=routed, probs=True)
        assert (got['leaf'] == 0).all() and (got['ops'] == int(ops)).all()
        assert np.array_equal(got['cls'] == y.argmax(1), acc == 1)


def test_conv_engine_refuses():
    from test_conv_layer import conv_net
    net = conv_net()((16, 16, 3), (10,))
    assert type(net.engine()).__name__ == 'ConvEngine'
    with pytest.raises(NotImplementedError, match='predict'):
        net.predict(np.zeros((4, 16, 16, 3), np.float32))


# ---------------------------------------------------------------------------------- H: hipGraph replay
def test_graph_replay_on_new_images():
    def build():
        net = make(seed=31)
        randomise_routers(net, seed=3, scale=1.0)
        calibrate_exit_fractions(net, *batch(256, seed=1), [1 / 8] * 7)
        return net
    net = build()
    xa, xb = batch(256, seed=1)[0], batch(256, seed=2)[0]
    assert net.engine().use_graph
    for x in (xa, xb, xa):                                        # (eager, capture, replay)
        net.predict(x, routed=True, probs=True)
    got = host(net.predict(xb, routed=True, probs=True))
    assert any(k[0] == 'pr+p' and not isinstance(g, str) for k, g in net.engine()._graphs.items())
    fresh = host(build().predict(xb, routed=True, probs=True))
    for k in KEYS:
        assert np.array_equal(got[k], fresh[k]), k
    assert len(set(got['leaf'].tolist())) >= 2


# ---------------------------------------------------------------------------------- I: the driver
def test_classify_images_cli(tmp_path):
    out = str(tmp_path / 'nets')
    pkg = os.path.join(ROOT, 'multipath-nn_amd')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '8', '--nets', '0',
                          '--out', out], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    ckpt = os.path.join(out, 'cifar10-ac', '0000.npy')
    x = np.random.default_rng(5).random((100, 32, 32, 3)).astype(np.float32)
    np.savez(str(tmp_path / 'images.npz'), x=x)
    pred = str(tmp_path / 'pred.npz')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'classify-images'), ckpt, str(tmp_path / 'images.npz'), '--out', pred,
                          '--batch', '64', '--probs'], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    text = res.stdout.decode()
    hist = [int(v) for v in text.split('exit histogram:')[1].splitlines()[0].split()]
    assert len(hist) == 8 and sum(hist) == 100
    got = np.load(pred)
    from lib.serdes import read_net
    net = read_net(ckpt)
    want = host(net.predict(x, routed='auto', probs=True))
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(np.bincount(got['leaf'], minlength=8), hist)
    assert 'mean operations per image: %.1f' % got['ops'].mean() in text
