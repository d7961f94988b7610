"""GPU: Net.exit_conf_curve -- the threshold curve in one dense pass -- on whole nets.  Everything is exact (integers).

  * the central check: for every point t, correct[t], ops[t] and hist[t] are the aggregate of predict(x, exit_conf=row t)
    -- the exit taken and the operations of every image -- joined with the per-leaf hits of the dense labelled eval; on the
    actor chain, a critic chain with dyn_k_cpt, the 15-block tree with 3-sink switches, a net with superclass and
    squared-linear exits (raw confidences), an any-width net (24 classes) and a net on the general conv kernels (24x40);
    200 images, 9 points: -inf, +inf and NaN rows, per-exit quantiles of the
    confidences that occur, a staircase row on which a third of the images that reach an exit leave there, a row with some
    exits left to their routers; every gateable exit is taken at some point;
  * the same numbers from tests/exit_curve_ref.py on the downloaded confidences, hits and router outputs;
  * an all-NaN row is the learnt policy of eval: sum p_ev d_cor and sum p_ev n_ops;
  * a hand-built deeply supervised SRNet chain (no router anywhere) against the numpy reference; -inf, +inf;
  * chunking, bytes with a decode table, repeated calls, a used engine against a fresh one, eval / predict untouched by a
    curve call, launch lists, the driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exit_curve_ref as R
from test_predict_nets import KEYS, host, same_snapshot
from test_routed_eval import batch, make, randomise_routers, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')


def parts(net, x0, y, k_cpt=None, extra=None):
    """What the dense programs leave per image: hits [leaves, n] (eval), router outputs [switches, n, MS] (eval; zero rows for
    static forks) and confidences [leaves, n] (a dense predict runs every head on every image)."""
    eng, n = net.engine(), len(x0)
    net.eval({net.x0: x0, net.y: y, **(extra or {})})
    torch.cuda.synchronize()
    d_cor = np.stack([ℓ.δ_cor.cpu().numpy() for ℓ in net.leaves])
    MS = eng.max_sinks
    r = np.zeros((max(len(eng.switches), 1), n, MS), np.float32)
    for nd in eng.switches:
        if nd.layer.router is not None:
            r[nd.switch_id, :, :len(nd.layer.sinks)] = nd.layer.router.x.cpu().numpy()
    net.predict(x0, routed=False, k_cpt=k_cpt)
    torch.cuda.synchronize()
    conf = eng.pr_conf.view(len(eng.leaves), eng.n_max)[:, :n].cpu().numpy().copy()
    return conf, d_cor, r


def rows_for(net, conf, r, n):
    """At most 9 threshold rows [T, leaves] from confidences that occur: see the module docstring."""
    tree, ops = R.tree_of_net(net)
    nl, exits = conf.shape[0], net.threshold_exits
    q = lambda l, f: np.sort(conf[l])[min(int(f * n), n - 1)]
    rows = [np.full(nl, v, np.float32) for v in (-INF, INF, NAN)]
    rows += [np.array([q(l, f) for l in range(nl)], np.float32) for f in (0.25, 0.5, 0.8)]
    # the staircase: top-down, a third of the images that reach an exit's block leave there (the later exits still at +inf)
    stair = np.full(nl, INF, np.float32)
    for nd in tree:
        if nd['exit'] < 0:
            continue
        l = tree[nd['sinks'][nd['exit']]]['leaf']
        stair[l] = -INF                             # (everybody who reaches the block leaves: that is who reaches it)
        here = [s for s in range(n) if R.walk(tree, ops, conf, r, stair, s)[0] == l]
        stair[l] = np.sort(conf[l, here])[::-1][max(len(here) // 3 - 1, 0)] if here else INF
    rows.append(stair)
    some = rows[4].copy()
    some[exits[::2]] = NAN                          # every other exit left to its router
    rows.append(some)
    rows.append(np.where(np.arange(nl) % 2 == 0, rows[3], rows[5]).astype(np.float32))
    taus = np.stack(rows)
    keep = np.zeros(nl, bool)
    keep[exits] = True
    taus[:, ~keep] = NAN
    return taus, tree, ops


def central(net, x0, y, k_cpt=None, extra=None):
    n = len(x0)
    conf, d_cor, r = parts(net, x0, y, k_cpt, extra)
    taus, tree, ops = rows_for(net, conf, r, n)
    assert len(taus) <= 9
    got = net.exit_conf_curve(x0, y, taus, batch=n, k_cpt=k_cpt)
    assert got.n == n and got.correct.dtype == got.ops.dtype == got.hist.dtype == np.int64
    assert np.array_equal(got.taus.view(np.uint32), taus.view(np.uint32))
    nl = conf.shape[0]
    gate = net.gateable_leaves
    for t, row in enumerate(taus):
        call = [None if np.isnan(v) else float(v) for v in row]
        res = host(net.predict(x0, routed=False, k_cpt=k_cpt, exit_conf=call if any(v is not None for v in call) else None))
        leaf = res['leaf']
        print('point %d: hist %s correct %d ops %d' % (t, np.bincount(leaf, minlength=nl).tolist(), got.correct[t], got.ops[t]))
        assert np.array_equal(got.hist[t], np.bincount(leaf, minlength=nl)), t
        assert got.ops[t] == res['ops'].sum(), t
        assert got.correct[t] == int((d_cor[leaf, np.arange(n)] == 1).sum()), t
    want = R.curve(tree, ops, conf, d_cor, r, taus, n, nl)
    for g, w in zip((got.correct, got.ops, got.hist), want):
        assert np.array_equal(g, w)
    assert (got.hist[:, gate].max(0) > 0).all(), got.hist.max(0)           # every gateable exit is taken at some point
    assert np.array_equal(got.acc, got.correct / n) and np.array_equal(got.moc, got.ops / n) and got.acc.dtype == np.float64
    # the all-NaN row (point 2) is the learnt policy of eval
    net.eval({net.x0: x0, net.y: y, **(extra or {})})
    torch.cuda.synchronize()
    eng = net.engine()
    p_ev = np.stack([nd.layer.p_ev.cpu().numpy() for nd in eng.nodes])
    assert set(np.unique(p_ev).tolist()) <= {0.0, 1.0}
    leaves = np.stack([nd.layer.p_ev.cpu().numpy() for nd in eng.leaves])
    assert got.correct[2] == int((leaves * d_cor).sum()) and np.array_equal(got.hist[2], leaves.sum(1).astype(np.int64))
    assert got.ops[2] == sum(int(p_ev[nd.idx].sum()) * ops[nd.idx] for nd in eng.nodes)
    return got


def test_actor_chain():
    net = make('ac', k_cpt=1e-9)
    randomise_routers(net)
    x0, y = batch(200, seed=3)
    got = central(net, x0, y)
    assert got.hist.shape == (9, 8) and (got.hist[0] == [200] + [0] * 7).all() and (got.hist[1] == [0] * 7 + [200]).all()
    # the 1-D form: one threshold for every exit a threshold applies to
    one = net.exit_conf_curve(x0, y, [0.0, 2.0, float(got.taus[4, 0])], batch=200)
    assert np.array_equal(one.hist[0], got.hist[0]) and np.array_equal(one.hist[1], got.hist[1])
    assert np.isnan(one.taus[:, 7]).all() and (one.taus[2, :7] == got.taus[4, 0]).all()
    best = one.tau_for_ops(float(one.moc.max()))
    assert best.index == int(np.argmax(one.acc)) and one.tau_for_ops(float(one.moc.min()) - 1) is None


def test_critic_chain_dyn_k_cpt():
    net = make('cr', dyn_k_cpt=True, k_cpt=0.0)
    randomise_routers(net)
    x0, y = batch(200, seed=4)
    kc = np.random.default_rng(1).choice([1e-9, 6.4e-8], 200).astype(np.float32)
    central(net, x0, y, k_cpt=kc, extra={net.k_cpt: kc})


def test_tree_with_three_sink_switches(monkeypatch):
    import arch_and_hypers as A
    from test_squared_error_nets import squared_net
    net = squared_net(A, monkeypatch, 'tree-ac')
    assert len(list(net.leaves)) == 15 and len(net.gateable_leaves) == 7
    x0, y = batch(200, seed=12)
    # the perturbed routers of this tree send nearly everybody down one side: shift their biases so that every leaf is taken
    from test_predict_nets import spread_over_leaves
    net.eval({net.x0: x0, net.y: y})
    r0 = {id(ℓ): ℓ.router.x.cpu().numpy().copy() for ℓ in net.switches}
    spread_over_leaves(net, lambda ℓ: r0[id(ℓ)], 200)
    got = central(net, x0, y)
    below = [k for k in range(15) if k not in net.gateable_leaves]
    assert (got.hist[1][below] > 0).sum() >= 2 and got.hist[1][below].sum() == 200      # (+inf: the routers pick among the children)


def test_superclass_and_squared_linear_exits(monkeypatch):
    import arch_and_hypers as A
    from test_squared_error_nets import squared_net
    net = squared_net(A, monkeypatch, 'ac-mixed')
    assert net.leaf_n_cls == [10, 2, 10, 10]
    x0, y = batch(200, seed=3)
    central(net, x0, y)


def test_any_width_exits_24_classes(monkeypatch):
    from test_exit_conf_nets import small_chain
    from test_net_parity import batch as batch_c
    net = small_chain(monkeypatch, n_cls=24)
    assert net.engine().generic_exits
    x0, y = batch_c(200, 3, 24, seed=2)
    central(net, x0, y)


def test_general_conv_kernels_24x40(monkeypatch):
    import arch_and_hypers as A
    from test_net_parity import perturb_routers
    from test_rect_nets import _batch
    monkeypatch.setattr(A, 'arch', A.arch[:4])
    net = A.ac_chain(k_cpt=1.6e-8)((24, 40, 3), (10,))
    net.engine().init_params(1234)
    perturb_routers(net)
    assert net.engine().generic_convs
    x0, y = _batch((24, 40, 3), 200, seed=3)
    central(net, x0, y)


# ---------------------------------------------------------------------------------- statically forked nets
def ds_net(seed=7):
    net = R.ds_chain(3)
    net.engine().init_params(seed)
    rng = np.random.default_rng(seed + 1)
    for p in net._all_params:
        if not p.trainable:
            p.assign(rng.random(p.shape) * 0.5 + (0.75 if p.name == 'v_avg' else -0.25))
    for ℓ in net.leaves:                            # (the heads of an untrained net are close to uniform: spread the confidences)
        w = ℓ.comps[1].params.w
        w.assign(w.numpy() * 4.0)
    return net


def test_deeply_supervised_static_chain():
    net = ds_net()
    assert net.threshold_exits == [0, 1] and net.gateable_leaves == []
    x0, y = batch(200, seed=5)
    conf, d_cor, r = parts(net, x0, y)
    tree, ops = R.tree_of_net(net)
    assert [nd['switch'] for nd in tree] == [-1] * 7
    q = lambda l, f: float(np.sort(conf[l])[int(f * 200)])
    taus = np.array([[-INF] * 3, [INF] * 3, [NAN] * 3, [q(0, 0.5), q(1, 0.5), NAN], [q(0, 0.7), q(1, 0.2), 0.0],
                     [NAN, q(1, 0.6), NAN], [q(0, 0.3), NAN, NAN]], np.float32)
    got = net.exit_conf_curve(x0, y, taus, batch=200)
    want = R.curve(tree, ops, conf, d_cor, r, taus, 200, 3)
    for g, w in zip((got.correct, got.ops, got.hist), want):
        assert np.array_equal(g, w)
    assert got.hist[0].tolist() == [200, 0, 0] and got.hist[1].tolist() == got.hist[2].tolist() == [0, 0, 200]
    assert got.correct[0] == int(d_cor[0].sum()) and got.correct[1] == int(d_cor[2].sum())
    assert got.ops[0] == 200 * sum(ops[j] for j in (0, 1, 2)) and got.ops[1] == 200 * sum(ops[j] for j in (0, 1, 3, 5, 6))
    assert (got.hist.max(0) > 0).all() and got.hist[3][0] == int((conf[0] >= taus[3, 0]).sum()) == 100
    assert np.isnan(got.taus[:, 2]).all()                                  # (no threshold applies to the last exit)
    one = net.exit_conf_curve(x0, y, [q(0, 0.5)], batch=64)                # the 1-D form, in chunks
    assert one.hist[0, 0] == 100 and one.hist.sum() == 200 and np.array_equal(one.hist[0], R.curve(tree, ops, conf, d_cor, r, [q(0, 0.5)], 200, 3)[2][0])
    with pytest.raises(ValueError, match='nothing to gate'):               # (predict itself still has no gate for them)
        net.predict(x0, exit_conf=0.5)


# ---------------------------------------------------------------------------------- chunks, bytes, state
@pytest.fixture(scope='module')
def small():
    """The actor chain with randomised routers, 300 images of bytes and their floats, three points; shared, unchanged."""
    from types import SimpleNamespace as Ns
    from lib.decode import decode_table

    def build():
        net = make(seed=31)
        randomise_routers(net, seed=3, scale=1.0)
        return net
    rng = np.random.default_rng(4)
    xb = rng.integers(0, 256, (300, 32, 32, 3), dtype=np.uint8)
    y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 300)]
    xf = decode_table('gamma')[xb]
    net = build()
    c0 = np.sort(host(net.predict(xf[:128], exit_conf=0.0))['conf'])
    taus = [float(c0[32]), float(c0[64]), float(c0[100]), -INF, INF]
    return Ns(build=build, net=net, xb=xb, xf=xf, y=y, taus=taus, want=net.exit_conf_curve(xf, y, taus, batch=512))


def same_curve(a, b):
    for k in ('correct', 'ops', 'hist'):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.n == b.n and np.array_equal(a.taus.view(np.uint32), b.taus.view(np.uint32))


def test_chunks_and_bytes(small):
    net = small.net
    assert small.want.hist.sum(1).tolist() == [300] * 5 and len({tuple(h) for h in small.want.hist.tolist()}) == 5
    same_curve(net.exit_conf_curve(small.xf, small.y, small.taus, batch=128), small.want)      # 128 + 128 + 44
    same_curve(net.exit_conf_curve(small.xb, small.y, small.taus, batch=128, decode='gamma'), small.want)
    same_curve(net.exit_conf_curve(torch.from_numpy(small.xf).to('cuda:0'), torch.from_numpy(small.y), small.taus, batch=100), small.want)
    empty = net.exit_conf_curve(small.xf[:0], small.y[:0], small.taus)
    assert empty.n == 0 and not empty.hist.any() and empty.hist.shape == (5, 8)


def test_repeated_calls_replay_one_graph(small):
    net, eng = small.net, small.net.engine()
    for _ in range(3):                                                     # (eager, capture, replay -- per chunk size)
        same_curve(net.exit_conf_curve(small.xf, small.y, small.taus, batch=128), small.want)
    keys = [k for k, g in eng._graphs.items() if k[0] == 'ev+c' and not isinstance(g, str)]
    assert {k[1] for k in keys} >= {128, 44} and all(k[-1] == 5 for k in keys)
    # other thresholds, the same number of points: the same programs and graphs
    before = (len(eng._progs), len(eng._graphs))
    other = net.exit_conf_curve(small.xf, small.y, [0.3, 0.5, 0.7, 0.9, NAN], batch=128)
    assert (len(eng._progs), len(eng._graphs)) == before
    same_curve(other, small.build().exit_conf_curve(small.xf, small.y, [0.3, 0.5, 0.7, 0.9, NAN], batch=300))


def test_used_engine_equals_fresh_and_leaves_eval_and_predict_alone(small):
    net = small.build()
    x, y = small.xf[:128], small.y[:128]
    feed = {net.x0: x, net.y: y}
    net.eval(feed)
    torch.cuda.synchronize()
    first = snapshot(net)
    pred = host(net.predict(x, probs=True, exit_conf=small.taus[0]))
    plain = host(net.predict(x, probs=True))
    got = net.exit_conf_curve(small.xf, small.y, small.taus, batch=128)
    same_curve(got, small.want)
    with pytest.raises(RuntimeError, match='exit_conf_curve'):
        net.state()
    net.eval(feed)
    torch.cuda.synchronize()
    same_snapshot(first, snapshot(net))
    for k in KEYS:
        assert np.array_equal(host(net.predict(x, probs=True, exit_conf=small.taus[0]))[k], pred[k]), k
        assert np.array_equal(host(net.predict(x, probs=True))[k], plain[k]), k
    # an engine that has just trained a step, predicted under another gate and evaluated: a fresh engine's curve, bit for bit
    used, fresh = small.build(), small.build()
    step = {used.x0: x, used.y: y, used.mode: 'tr', used.λ_lrn: 0.05, used.τ: 1.0}
    used.train.run(step)
    fresh.train.run({fresh.x0: x, fresh.y: y, fresh.mode: 'tr', fresh.λ_lrn: 0.05, fresh.τ: 1.0})
    used.predict(x, routed=True, exit_conf=[0.2, None, 0.9, None, 0.5, None, 0.1, None])
    used.eval({used.x0: small.xf[128:200], used.y: small.y[128:200]}, routed=True)
    same_curve(used.exit_conf_curve(small.xf, small.y, small.taus, batch=128), fresh.exit_conf_curve(small.xf, small.y, small.taus, batch=128))


def test_launch_lists(small):
    eng = small.net.engine()
    for mode, routed in (('ev', False), ('ev', 1), ('pr', False), ('pr', 3), ('pr+p', False)):
        whats = [op.what for op in eng.program(mode, 128, routed)['fwd']]
        assert 'exit_curve' not in whats and 'route' in whats
    cv = eng.program('ev+c', 128, False, points=5)
    whats = [op.what for op in cv['fwd']]
    ev = [op.what for op in eng.program('ev', 128, False)['fwd']]
    assert whats == ev[:-1] + ['exit_curve'] and ev[-1] == 'route' and cv['points'] == 5
    recs = [e for op in cv['fwd'] if op.what == 'exit_ev' for e in op.host]
    assert all(e.y and e.c_err and e.d_cor and e.cls and e.conf and not e.p_cls for e in recs if e.w_head)
    assert eng.curve_tree_dev.data_ptr() == cv['fwd'][-1].host.tree


# ---------------------------------------------------------------------------------- the driver
def test_classify_images_curve(small, tmp_path):
    from lib.serdes import write_net
    ckpt, images, out = (str(tmp_path / f) for f in ('net.npy', 'images.npz', 'curve.npz'))
    write_net(ckpt, small.net)
    np.savez(images, x=small.xb, y=small.y)
    tool = os.path.join(ROOT, 'multipath-nn_amd', 'classify-images')
    res = subprocess.run([sys.executable, tool, ckpt, images, '--curve', '0.2:0.9:6', '--decode', 'gamma', '--batch', '128', '--out', out],
                         cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    got = np.load(out)
    want = small.net.exit_conf_curve(small.xb, small.y, np.linspace(0.2, 0.9, 6), batch=128, decode='gamma')
    assert np.array_equal(got['taus'], np.linspace(0.2, 0.9, 6)) and int(got['n']) == 300
    for k in ('acc', 'moc', 'hist'):
        assert np.array_equal(got[k], getattr(want, k)), k
    assert len({tuple(h) for h in got['hist'].tolist()}) >= 3
    np.savez(images, x=small.xb)                                           # no labels: refused loudly
    res = subprocess.run([sys.executable, tool, ckpt, images, '--curve', '0.2:0.9:6', '--decode', 'gamma', '--out', out],
                         cwd=str(tmp_path), capture_output=True)
    assert res.returncode != 0 and 'y' in res.stderr.decode() and 'label' in res.stderr.decode()
