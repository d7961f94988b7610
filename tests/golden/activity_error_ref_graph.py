"""ActivityError: the REFERENCE'S OWN `ActivityError.link` (scripts/lib/layer_types.py:287-293, imported unmodified) over
tests/golden/tf_standin.py -- alone, on a [n, nc] row and on a [n, h, w, c] map, with positive and negative α -- and inside a
small SRNet, a small actor net and a small critic net (use_cls_err) built from the reference's own layer and net classes,
with the layer behind Select (the block's coarsest map), behind the LinTrans (the logits) and behind the Softmax (the
probabilities): the vectors that tests/activity_error_ref.py (the float64 restatement the GPU tests are held to) is checked
against in tests/test_activity_error_ref_cpu.py.

As with every stand-in op this pins the Python the reference writes on top of the operators (the cost, and how the nets'
costs and gradients consume a per-sample c_mod), not TensorFlow's own operator semantics.

    python tests/golden/activity_error_ref_graph.py --emit tests/golden/activity_error_ref_graph.npz      # REFERENCE side (build container only)

FIXTURE TOOLING.  Nothing here is on the product path; only the --emit child reads the reference tree.  The inputs are
regenerated from the seeds by `layer_input` / `net_inputs`; the file holds outputs only.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_graph_golden as M

REF = M.REF

# the layer alone: a row of outputs and an activation map
LAYER_CASES = {
    'row': dict(shape=(8, 10), α=0.25, seed=91),
    'row_negative': dict(shape=(6, 3), α=-1.5, seed=92),
    'map': dict(shape=(5, 4, 4, 6), α=1e-2, seed=93),
    'map_one': dict(shape=(1, 2, 3, 5), α=-0.5, seed=94),
}
# the nets: a 3-block chain (the SRNet: its one exit under block 2), the layer at all three positions of every exit, with
# different α per block and per position, one of them negative
ACT = {0: dict(map=2e-3, logits=5e-2, probs=0.5), 1: dict(map=-1e-3, logits=2e-2, probs=-0.25), 2: dict(map=1e-3, logits=-1e-2, probs=1.0)}
NETS = {
    'sr': dict(type='SRNet', tau=None, n=4, seed=95, hypers=dict()),
    'actor': dict(type='ActorNet', tau=0.7, n=4, seed=96, hypers=dict(k_cpt=1.6e-8)),
    'critic': dict(type='CriticNet', tau=0.1, n=4, seed=97, hypers=dict(k_cpt=8e-9, use_cls_err=True)),
}


def layer_input(case):
    """x of a layer case."""
    return np.random.RandomState(4000 + case['seed']).standard_normal(case['shape']) * 1.5


def activity_chain(A, NT, spec):
    """A 3-block chain through the LAYER CLASSES of the side that runs (the module A imported them from)."""
    L = sys.modules[A.Chain.__module__]

    def reg(nc, i):
        a = ACT[i]
        return L.Chain(name='LogReg', comps=[L.Select(i=-1), L.ActivityError(α=a['map']), L.LinTrans(n_chan=nc, k_l2=A.k_l2, σ_w=1),
                                             L.ActivityError(α=a['logits']), L.Softmax(), L.ActivityError(α=a['probs']),
                                             L.CrossEntropyError()])

    def make_net(x0_shape, y_shape):
        nc = y_shape[0]
        if spec['type'] == 'SRNet':
            root = A.pyr(A.rcm(0, A.rcm(1, A.rcm(2, reg(nc, 2)))))
        else:
            root = A.pyr(A.rcm(0, reg(nc, 0), A.rcm(1, reg(nc, 1), A.rcm(2, reg(nc, 2)))))
        return getattr(NT, spec['type'])(x0_shape=x0_shape, y_shape=y_shape, root=root, **spec['hypers'])
    return make_net


def net_inputs(spec):
    rng = np.random.RandomState(1000 + spec['seed'])
    n = spec['n']
    return rng.random_sample((n, 32, 32, 3)), np.eye(10)[rng.randint(0, 10, n)]


def feed_of(net, spec, x0, y, mode, more=()):
    feed = {net.x0: x0, net.y: y, net.mode: mode, **dict(more)}
    if spec['tau'] is not None:
        feed[net.τ] = spec['tau']
    return feed


def emit(path):
    import tf_standin
    sys.modules['tensorflow'] = tf_standin
    sys.path.insert(0, REF)
    import lib.layer_types as LT                      # the REFERENCE's modules
    import lib.net_types as NT
    import arch_and_hypers as A
    assert LT.__file__.startswith(REF) and NT.__file__.startswith(REF) and A.__file__.startswith(REF)
    out = {}
    for key, case in sorted(LAYER_CASES.items()):
        tf_standin.reset()
        x = tf_standin.placeholder(tf_standin.float32, (None,) + tuple(case['shape'][1:]))
        ℓ = LT.ActivityError(α=case['α'])
        ℓ.link(x, None, None)
        assert ℓ.x is x and vars(ℓ.params) == {}                                       # (x passes through; no parameters)
        c_mod, c_err, n_ops = tf_standin.run([ℓ.c_mod, ℓ.c_err, ℓ.n_ops], {x: layer_input(case)})
        assert np.asarray(c_err).shape == () and float(c_err) == 0 and float(n_ops) == 0   # (no error, no work)
        out['layer/%s/c_mod' % key] = np.asarray(c_mod, np.float64)
        print(key, 'ok:', np.asarray(c_mod))
    for key, spec in sorted(NETS.items()):
        tf_standin.reset()
        net = activity_chain(A, NT, spec)((32, 32, 3), (10,))
        rng = np.random.RandomState(spec['seed'])
        params = M.ordered_params(net, NT.params_list_rec)
        for name, var in params:
            var.load(M.param_value(name, var.data.shape, rng))
        x0, y = net_inputs(spec)
        layers = list(net.layers)
        leaves = [ℓ for ℓ in layers if len(ℓ.sinks) == 0]
        for mode in ('ev', 'tr'):
            feed = feed_of(net, spec, x0, y, mode)
            snap = [(v, v.data.detach().clone()) for _, v in params]       # (a 'tr' run moves the moving averages)
            # per leaf: c_err, and c_mod of its chain = the LinTrans's L2 term (a scalar) + the three per-sample penalties
            fetch = {'c_err': [ℓ.c_err for ℓ in leaves], 'c_mod': [ℓ.c_mod for ℓ in leaves]}
            if spec['type'] != 'SRNet':
                fetch.update(p_ev=[ℓ.p_ev for ℓ in layers], p_tr=[ℓ.p_tr for ℓ in layers])
            for k, nodes in fetch.items():
                vals = tf_standin.run(nodes, feed)
                out['%s/%s/%s' % (key, mode, k)] = np.stack([np.broadcast_to(np.asarray(v, np.float64), (len(x0),)) for v in vals])
            for v, d in snap:
                v.load(d.numpy())
        # one training step (momentum 0.9 from zero accumulators): every variable moves by its own (TALR-scaled) gradient
        net.train.run(feed_of(net, spec, x0, y, 'tr', {net.λ_lrn: M.LR}))
        out['%s/after' % key] = np.array([M.digest(v.data.detach().numpy()) for _, v in params])
        out['%s/names' % key] = np.array([n for n, _ in params])
        print(key, 'ok:', len(layers), 'nodes,', len(leaves), 'leaves,', len(params), 'variables')
    np.savez_compressed(path, **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--emit', required=True)
    emit(ap.parse_args().emit)
