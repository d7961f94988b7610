"""Rectangular and non-power-of-two images: the REFERENCE'S OWN graph code (over tests/golden/tf_standin.py) on
x0_shape (24, 40, 3) with the shipped four-scale table and on (28, 28, 1) with a three-scale table -- shapes that
make_ref_graph_golden.py and fuzz_ref_graph.py (32x32 throughout) never ran.  Same vectors as make_ref_graph_golden.py: the
forward values in both modes and the digest of every variable after one training step.

The two sides cannot share a process (both packages are called `lib`):

    python tests/golden/rect_ref_graph.py --emit out.npz       # REFERENCE side (build container only)
    tests/test_conv_hw_cpu.py                                   # oracle side, against rect_ref_graph_golden.npz

FIXTURE TOOLING.  Nothing here is on the product path; only the --emit child reads the reference tree.  Its results are
stored in rect_ref_graph_golden.npz:

    python tests/golden/rect_ref_graph.py --emit tests/golden/rect_ref_graph_golden.npz
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_graph_golden as M

REF = M.REF
ARCH3 = [3 * [16], 3 * [16], 2 * [32], 2 * [32]]       # a three-scale table: 28x28 -> 28, 14, 7

CASES = {
    'ac_24x40': dict(ctor='ac_chain', hypers=dict(k_cpt=1.6e-8), tau=0.7, n=3, shape=(24, 40, 3), seed=31),
    'sr_24x40': dict(ctor='sr_chain', args=(3,), hypers={}, tau=None, n=3, shape=(24, 40, 3), seed=32),
    'ac_28x28': dict(ctor='ac_chain', hypers=dict(k_cpt=4e-9), tau=0.9, n=3, shape=(28, 28, 1), arch=ARCH3, seed=33),
    'sr_28x28': dict(ctor='sr_chain', args=(4,), hypers={}, tau=None, n=3, shape=(28, 28, 1), arch=ARCH3, seed=34),
}


def build(A, NT, case):
    """The case's net from a spec module A (whose `arch` the constructors read when they are called)."""
    saved = A.arch
    try:
        A.arch = case.get('arch', saved)
        return M.make_case(A, NT, case)(case['shape'], (10,))
    finally:
        A.arch = saved


def case_inputs(case):
    rng = np.random.RandomState(1000 + case['seed'])
    n = case['n']
    x0 = rng.random_sample((n,) + tuple(case['shape']))
    y = np.eye(10)[rng.randint(0, 10, n)]
    return x0, y


def emit(path):
    import tf_standin
    sys.modules['tensorflow'] = tf_standin
    sys.path.insert(0, REF)
    import lib.net_types as NT                       # the REFERENCE's modules
    import arch_and_hypers as A
    assert NT.__file__.startswith(REF) and A.__file__.startswith(REF)
    out = {}
    for key, case in sorted(CASES.items()):
        tf_standin.reset()
        net = build(A, NT, case)
        rng = np.random.RandomState(case['seed'])
        params = M.ordered_params(net, NT.params_list_rec)
        for name, var in params:
            var.load(M.param_value(name, var.data.shape, rng))
        x0, y = case_inputs(case)
        layers = list(net.layers)
        leaves = [ℓ for ℓ in layers if len(ℓ.sinks) == 0]
        switches = [ℓ for ℓ in layers if len(ℓ.sinks) > 1]
        feed = {net.x0: x0, net.y: y}
        if case['tau'] is not None:
            feed[net.τ] = case['tau']
        fetch = {'p_ev': [ℓ.p_ev for ℓ in layers], 'c_err': [ℓ.c_err for ℓ in leaves], 'd_cor': [ℓ.δ_cor for ℓ in leaves]}
        if hasattr(layers[0], 'p_tr'):
            fetch['p_tr'] = [ℓ.p_tr for ℓ in layers]
            fetch['r'] = [ℓ.router.x for ℓ in switches]
        for mode in ('ev', 'tr'):
            f = dict(feed)
            f[net.mode] = mode
            snap = [(v, v.data.detach().clone()) for _, v in params]       # (a 'tr' run moves the moving averages)
            for k, nodes in fetch.items():
                vals = tf_standin.run(nodes, f)
                out['%s/%s/%s' % (key, mode, k)] = np.stack([np.asarray(v, np.float64) if k == 'r' else
                                                            np.broadcast_to(np.asarray(v, np.float64), (case['n'],)) for v in vals])
            for v, d in snap:
                v.load(d.numpy())
        f = dict(feed)
        f[net.mode] = 'tr'
        f[net.λ_lrn] = M.LR
        net.train.run(f)
        out['%s/after' % key] = np.array([M.digest(v.data.detach().numpy()) for _, v in params])
        out['%s/names' % key] = np.array([n for n, _ in params])
        print(key, 'ok:', len(params), 'variables,', len(layers), 'nodes')
    np.savez_compressed(path, **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--emit', required=True)
    emit(ap.parse_args().emit)
