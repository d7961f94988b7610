"""SuperclassCrossEntropyError: the REFERENCE'S OWN `SuperclassCrossEntropyError.link` (scripts/lib/layer_types.py:274-285,
imported unmodified) over tests/golden/tf_standin.py, alone and inside a small actor net built from the reference's own
layer and net classes -- the vectors that tests/superclass_ref.py (the float64 restatement the GPU tests are held to) is
checked against in tests/test_superclass_ref_cpu.py.

As with every stand-in op this pins the Python the reference writes on top of the operators (the projection of the
labels, the divisor ϵ / n_sup, the cost, the two arg-maxes, and how the net's routing and costs consume them), not
TensorFlow's own operator semantics (arg-max: first index on ties, the stand-in's stated assumption).

    python tests/golden/superclass_ref_graph.py --emit tests/golden/superclass_ref_golden.npz      # REFERENCE side (build container only)

FIXTURE TOOLING.  Nothing here is on the product path; only the --emit child reads the reference tree.  The inputs are
regenerated from the seeds by `layer_input` / `net_inputs`; the file holds outputs only.
"""
import argparse
import os
import sys
import unicodedata

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_graph_golden as M

REF = M.REF


def hard(n_cls, n_sup):
    w = np.zeros((n_cls, n_sup))
    w[np.arange(n_cls), np.arange(n_cls) * n_sup // n_cls] = 1
    return w


def soft(n_cls, n_sup):
    w = 0.75 * hard(n_cls, n_sup)
    w[np.arange(n_cls), (np.arange(n_cls) * n_sup // n_cls + 1) % n_sup] += 0.25
    return w


# the layer alone: a 0/1 map 10>3, a 0/1 map 10>2, a soft map (rows [0.75, 0.25]), outputs that tie for the maximum
LAYER_CASES = {
    'hard3': dict(w=hard(10, 3), hypers={}, n=6, seed=51),
    'hard2': dict(w=hard(10, 2), hypers={'ϵ': 1e-3}, n=6, seed=52),
    'soft2': dict(w=soft(10, 2), hypers={}, n=6, seed=53, soft_labels=True),
    'tie3': dict(w=hard(10, 3), hypers={}, n=6, seed=54, tie=True),
}
NET = dict(tau=0.7, n=4, seed=61, hypers=dict(k_cpt=1.6e-8))


def layer_input(case):
    """(x [n, n_sup] softmax rows, y [n, n_cls] labels) of a layer case."""
    rng = np.random.RandomState(3000 + case['seed'])
    n, (n_cls, n_sup) = case['n'], case['w'].shape
    z = rng.standard_normal((n, n_sup))
    x = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    if case.get('tie'):
        # the two largest outputs equal, at every pair of positions: [3, 3, 2] / 8 and its rotations
        x = np.array([np.roll([0.375, 0.375, 0.25], k) for k in range(n)])
    y = np.eye(n_cls)[rng.randint(0, n_cls, n)]
    if case.get('soft_labels'):
        y = 0.5 * y + 0.5 * np.eye(n_cls)[rng.randint(0, n_cls, n)]
    return x, y


def coarse_chain(A, NT):
    """A 3-block actor chain through the LAYER CLASSES of the side that runs (the module A imported them from): the exit of
    block 0 on a 10>2 map, that of block 1 on a soft 10>5 map, that of block 2 fine."""
    L = sys.modules[A.Chain.__module__]

    def reg(nc, w=None):
        last = L.CrossEntropyError() if w is None else L.SuperclassCrossEntropyError(w_cls=w)
        return L.Chain(name='LogReg', comps=[L.Select(i=-1), L.LinTrans(n_chan=nc if w is None else w.shape[1], k_l2=A.k_l2, σ_w=1),
                                             L.Softmax(), last])

    def make_net(x0_shape, y_shape):
        nc = y_shape[0]
        b2 = A.rcm(2, reg(nc))
        b1 = A.rcm(1, reg(nc, soft(nc, 5)), b2)
        b0 = A.rcm(0, reg(nc, hard(nc, 2)), b1)
        return NT.ActorNet(x0_shape=x0_shape, y_shape=y_shape, root=A.pyr(b0), **NET['hypers'])
    return make_net


def net_inputs():
    rng = np.random.RandomState(1000 + NET['seed'])
    n = NET['n']
    return rng.random_sample((n, 32, 32, 3)), np.eye(10)[rng.randint(0, 10, n)]


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
        n_cls, n_sup = case['w'].shape
        x = tf_standin.placeholder(tf_standin.float32, (None, n_sup))
        y = tf_standin.placeholder(tf_standin.float32, (None, n_cls))
        # (Python NFKC-normalises identifiers but not string keys: {'ϵ': ..} must land on the attribute that `hypers.ϵ` reads)
        ℓ = LT.SuperclassCrossEntropyError(w_cls=case['w'], **{unicodedata.normalize('NFKC', k): v for k, v in case['hypers'].items()})
        ℓ.link(x, y, None)
        xv, yv = layer_input(case)
        c_err, d_cor = tf_standin.run([ℓ.c_err, ℓ.δ_cor], {x: xv, y: yv})
        out['layer/%s/c_err' % key] = np.asarray(c_err, np.float64)
        out['layer/%s/d_cor' % key] = np.asarray(d_cor, np.float64)
        print(key, 'ok:', np.asarray(d_cor))
    tf_standin.reset()
    net = coarse_chain(A, NT)((32, 32, 3), (10,))
    rng = np.random.RandomState(NET['seed'])
    for name, var in M.ordered_params(net, NT.params_list_rec):
        var.load(M.param_value(name, var.data.shape, rng))
    x0, y = net_inputs()
    layers = list(net.layers)
    leaves = [ℓ for ℓ in layers if len(ℓ.sinks) == 0]
    for mode in ('ev', 'tr'):
        feed = {net.x0: x0, net.y: y, net.τ: NET['tau'], net.mode: mode}
        p = 'p_tr' if mode == 'tr' else 'p_ev'
        # (the cost a leaf adds to the net's: its routing probability times its c_err -- net_types.py:167 in 'tr')
        cost = sum(getattr(ℓ, p) * ℓ.c_err for ℓ in leaves)
        fetch = {'p_ev': [ℓ.p_ev for ℓ in layers], 'p_tr': [ℓ.p_tr for ℓ in layers], 'c_err': [ℓ.c_err for ℓ in leaves],
                 'd_cor': [ℓ.δ_cor for ℓ in leaves], 'cost': [cost]}
        for k, nodes in fetch.items():
            vals = tf_standin.run(nodes, feed)
            out['net/%s/%s' % (mode, k)] = np.stack([np.broadcast_to(np.asarray(v, np.float64), (len(x0),)) for v in vals])
    print('net ok:', len(layers), 'nodes,', len(leaves), 'leaves')
    np.savez_compressed(path, **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--emit', required=True)
    emit(ap.parse_args().emit)
