"""Dropout: the REFERENCE'S OWN `Dropout.link` (scripts/lib/layer_types.py:212-217, imported unmodified) over
tests/golden/tf_standin.py -- alone, on a [n, nc] row and on a [n, h, w, c] map -- and inside a small SRNet and a small
actor net built from the reference's own layer and net classes with the layer in front of every head's LinTrans: the vectors
that tests/dropout_ref.py (the restatement the GPU tests are held to) is checked against in tests/test_dropout_ref_cpu.py.

The stand-in has no `tf.nn.dropout`; this script registers one from outside, without editing it: TF 0.12's
`x / keep_prob * floor(keep_prob + u)`, as a stand-in op (a torch expression: it carries its gradient), with the uniforms u
INJECTED -- u = r / 2^32 of the words tests/dropout_ref.py: words() draws for (seed, t = 0, leaf, n, K), so that both sides
see the same random numbers.  As with every stand-in op this pins the Python the reference writes on top of the operator (that
the layer's output replaces x in the chain, in EVERY mode: the reference's line has no mode test), not TensorFlow's own sampler.

    python tests/golden/dropout_ref_graph.py --emit tests/golden/dropout_ref_graph.npz      # REFERENCE side (build container only)

FIXTURE TOOLING.  Nothing here is on the product path; only the --emit child reads the reference tree.  The inputs are
regenerated from the seeds by `layer_input` / `net_inputs`; the file holds outputs only.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_ref_graph_golden as M

REF = M.REF

# the layer alone: a row of outputs and an activation map (leaf: the counter's third word)
LAYER_CASES = {
    'row': dict(shape=(8, 10), λ=0.5, seed=91, leaf=0),
    'row_rare': dict(shape=(6, 7), λ=0.125, seed=2 ** 40 + 92, leaf=3),
    'map': dict(shape=(5, 4, 4, 6), λ=0.75, seed=93, leaf=1),
    'map_one': dict(shape=(1, 2, 3, 5), λ=0.5, seed=94, leaf=46),
}
# the nets: a 3-block chain (the SRNet: its one exit under block 2) with the layer in front of every head's LinTrans
DROP = {0: dict(λ=0.5, seed=7), 1: dict(λ=0.75, seed=7), 2: dict(λ=0.5, seed=7)}
NETS = {
    'sr': dict(type='SRNet', tau=None, n=4, seed=95, hypers=dict()),
    'actor': dict(type='ActorNet', tau=0.7, n=4, seed=96, hypers=dict(k_cpt=1.6e-8)),
}


def layer_input(case):
    return np.random.RandomState(5000 + case['seed'] % 1000).standard_normal(case['shape']) * 1.5


def dropout_chain(A, NT, spec):
    """A 3-block chain through the LAYER CLASSES of the side that runs (the module A imported them from)."""
    L = sys.modules[A.Chain.__module__]

    def reg(nc, i):
        return L.Chain(name='LogReg', comps=[L.Select(i=-1), L.Dropout(**DROP[i]), L.LinTrans(n_chan=nc, k_l2=A.k_l2, σ_w=1),
                                             L.Softmax(), L.CrossEntropyError()])

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


def register_dropout(tf_standin, meta):
    """tf.nn.dropout for the stand-in: op j (in creation order) draws with meta[j] = (seed, leaf) at step 0."""
    import torch
    import dropout_ref as R
    made = []

    def dropout(x, keep_prob):
        j = len(made)
        made.append(j)

        def fn(ev):
            xv = tf_standin._t(ev(x))
            seed, leaf = meta[j] if j < len(meta) else (0, 0)      # (the stand-in evaluates an op once while the graph is built)
            n, K = int(xv.shape[0]), int(np.prod(xv.shape[1:]))
            u = R.words(seed, 0, leaf, n, K).astype(np.float64) / 4294967296.0
            u = torch.as_tensor(u.reshape(tuple(xv.shape)), dtype=xv.dtype)
            return xv / keep_prob * torch.floor(keep_prob + u)
        return tf_standin.T(fn)
    tf_standin._NN.dropout = staticmethod(dropout)
    return made


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
        made = register_dropout(tf_standin, [(case['seed'], case['leaf'])])
        x = tf_standin.placeholder(tf_standin.float32, (None,) + tuple(case['shape'][1:]))
        ℓ = LT.Dropout(λ=case['λ'])
        ℓ.link(x, None, None)
        assert made == [0] and vars(ℓ.params) == {}                                    # (one op; no parameters)
        xd, c_err, c_mod, n_ops = tf_standin.run([ℓ.x, ℓ.c_err, ℓ.c_mod, ℓ.n_ops], {x: layer_input(case)})
        assert float(c_err) == 0 and float(c_mod) == 0 and float(n_ops) == 0            # (no cost, no work)
        out['layer/%s/x' % key] = np.asarray(xd, np.float64)
        print(key, 'ok: kept', float((np.asarray(xd) != 0).mean()))
    assert vars(LT.Dropout().hypers) == {'λ': 1}                                        # (the reference's default: the identity)
    for key, spec in sorted(NETS.items()):
        tf_standin.reset()
        meta = []
        made = register_dropout(tf_standin, meta)
        net = dropout_chain(A, NT, spec)((32, 32, 3), (10,))
        layers = list(net.layers)
        leaves = [ℓ for ℓ in layers if len(ℓ.sinks) == 0]
        for i, ℓ in enumerate(leaves):                       # (the ops were made in link order: leaf after leaf)
            meta += [(c.hypers.seed, i) for c in ℓ.comps if type(c).__name__ == 'Dropout']
        assert len(made) == len(meta) == len(leaves)
        rng = np.random.RandomState(spec['seed'])
        params = M.ordered_params(net, NT.params_list_rec)
        for name, var in params:
            var.load(M.param_value(name, var.data.shape, rng))
        x0, y = net_inputs(spec)
        for mode in ('ev', 'tr'):
            feed = feed_of(net, spec, x0, y, mode)
            snap = [(v, v.data.detach().clone()) for _, v in params]       # (a 'tr' run moves the moving averages)
            fetch = {'c_err': [ℓ.c_err for ℓ in leaves]}
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
