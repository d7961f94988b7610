"""SquaredError: the REFERENCE'S OWN `SquaredError.link` (scripts/lib/layer_types.py:255-260, imported unmodified) over
tests/golden/tf_standin.py -- alone, on softmax rows and on raw outputs, with one-hot and real-valued targets and with tied
maxima -- and inside a small actor net and a small critic net (use_cls_err) built from the reference's own layer and net
classes: the vectors that tests/squared_error_ref.py (the float64 restatement the GPU tests are held to) is checked
against in tests/test_squared_error_ref_cpu.py.

As with every stand-in op this pins the Python the reference writes on top of the operators (the cost, the two arg-maxes,
and how the nets' routing, costs and gradients consume them), not TensorFlow's own operator semantics (arg-max: first
index on ties, the stand-in's stated assumption).

    python tests/golden/squared_error_ref_graph.py --emit tests/golden/squared_error_ref_graph.npz      # REFERENCE side (build container only)

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

# the layer alone: form 'sq' -- x a softmax row; 'lin' -- x any float row (outputs of a LinTrans)
LAYER_CASES = {
    'sq_onehot': dict(form='sq', target='onehot', n=8, nc=3, seed=71),
    'sq_real': dict(form='sq', target='real', n=6, nc=10, seed=72),
    'lin_onehot': dict(form='lin', target='onehot', n=8, nc=3, seed=73),
    'lin_real': dict(form='lin', target='real', n=6, nc=4, seed=74),
    'lin_negative': dict(form='lin', target='onehot', n=6, nc=3, seed=75, shift=-5.0),       # every output below -1
    'sq_tie': dict(form='sq', target='onehot', n=6, nc=3, seed=76, tie=True),
    'lin_tie': dict(form='lin', target='real', n=6, nc=3, seed=77, tie=True),
}
# the nets: a 3-block chain, the exit of block 0 squared on the softmax, that of block 1 squared on the raw outputs, that
# of block 2 a cross-entropy; real-valued targets for the critic
NETS = {
    'actor': dict(type='ActorNet', tau=0.7, n=4, seed=81, target='onehot', hypers=dict(k_cpt=1.6e-8)),
    'critic': dict(type='CriticNet', tau=0.1, n=4, seed=82, target='real', hypers=dict(k_cpt=8e-9, use_cls_err=True)),
}


def layer_input(case):
    """(x [n, nc], y [n, nc]) of a layer case."""
    rng = np.random.RandomState(3000 + case['seed'])
    n, nc = case['n'], case['nc']
    x = rng.standard_normal((n, nc)) * 2
    if 'shift' in case:
        x = np.clip(x, -3, 3) + case['shift']
    if case['form'] == 'sq':
        x = np.exp(x) / np.exp(x).sum(1, keepdims=True)
    y = np.eye(nc)[rng.randint(0, nc, n)] if case['target'] == 'onehot' else rng.standard_normal((n, nc))
    if case.get('tie'):
        # the two largest outputs equal, at every pair of positions; in the real-valued targets two equal maxima too
        base = [0.375, 0.375, 0.25] if case['form'] == 'sq' else [-1.5, -1.5, -4.0]
        x = np.array([np.roll(base, k) for k in range(n)])
        if case['target'] == 'real':
            y = np.array([np.roll([0.5, 2.0, 2.0], k // 2) for k in range(n)])
    return x, y


def squared_chain(A, NT, spec):
    """A 3-block chain through the LAYER CLASSES of the side that runs (the module A imported them from)."""
    L = sys.modules[A.Chain.__module__]

    def reg(nc, form=None):
        tail = {None: [L.Softmax(), L.CrossEntropyError()], 'sq': [L.Softmax(), L.SquaredError()], 'lin': [L.SquaredError()]}[form]
        return L.Chain(name='LogReg', comps=[L.Select(i=-1), L.LinTrans(n_chan=nc, k_l2=A.k_l2, σ_w=1)] + tail)

    def make_net(x0_shape, y_shape):
        nc = y_shape[0]
        b2 = A.rcm(2, reg(nc))
        b1 = A.rcm(1, reg(nc, 'lin'), b2)
        b0 = A.rcm(0, reg(nc, 'sq'), b1)
        return getattr(NT, spec['type'])(x0_shape=x0_shape, y_shape=y_shape, root=A.pyr(b0), **spec['hypers'])
    return make_net


def net_inputs(spec):
    rng = np.random.RandomState(1000 + spec['seed'])
    n = spec['n']
    x0 = rng.random_sample((n, 32, 32, 3))
    y = np.eye(10)[rng.randint(0, 10, n)] if spec['target'] == 'onehot' else rng.standard_normal((n, 10))
    return x0, y


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
        x = tf_standin.placeholder(tf_standin.float32, (None, case['nc']))
        y = tf_standin.placeholder(tf_standin.float32, (None, case['nc']))
        ℓ = LT.SquaredError()
        ℓ.link(x, y, None)
        assert ℓ.x is x                                # (the layer passes x through)
        xv, yv = layer_input(case)
        c_err, d_cor = tf_standin.run([ℓ.c_err, ℓ.δ_cor], {x: xv, y: yv})
        out['layer/%s/c_err' % key] = np.asarray(c_err, np.float64)
        out['layer/%s/d_cor' % key] = np.asarray(d_cor, np.float64)
        print(key, 'ok:', np.asarray(d_cor))
    for key, spec in sorted(NETS.items()):
        tf_standin.reset()
        net = squared_chain(A, NT, spec)((32, 32, 3), (10,))
        rng = np.random.RandomState(spec['seed'])
        params = M.ordered_params(net, NT.params_list_rec)
        for name, var in params:
            var.load(M.param_value(name, var.data.shape, rng))
        x0, y = net_inputs(spec)
        layers = list(net.layers)
        leaves = [ℓ for ℓ in layers if len(ℓ.sinks) == 0]
        for mode in ('ev', 'tr'):
            feed = {net.x0: x0, net.y: y, net.τ: spec['tau'], net.mode: mode}
            snap = [(v, v.data.detach().clone()) for _, v in params]       # (a 'tr' run moves the moving averages)
            fetch = {'p_ev': [ℓ.p_ev for ℓ in layers], 'p_tr': [ℓ.p_tr for ℓ in layers], 'c_err': [ℓ.c_err for ℓ in leaves],
                     'd_cor': [ℓ.δ_cor for ℓ in leaves]}
            for k, nodes in fetch.items():
                vals = tf_standin.run(nodes, feed)
                out['%s/%s/%s' % (key, mode, k)] = np.stack([np.broadcast_to(np.asarray(v, np.float64), (len(x0),)) for v in vals])
            for v, d in snap:
                v.load(d.numpy())
        # one training step (momentum 0.9 from zero accumulators): every variable moves by its own (TALR-scaled) gradient
        net.train.run({net.x0: x0, net.y: y, net.τ: spec['tau'], net.mode: 'tr', net.λ_lrn: M.LR})
        out['%s/after' % key] = np.array([M.digest(v.data.detach().numpy()) for _, v in params])
        out['%s/names' % key] = np.array([n for n, _ in params])
        print(key, 'ok:', len(layers), 'nodes,', len(leaves), 'leaves,', len(params), 'variables')
    np.savez_compressed(path, **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--emit', required=True)
    emit(ap.parse_args().emit)
