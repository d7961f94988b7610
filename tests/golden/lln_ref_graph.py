"""MultiscaleLLN: the REFERENCE'S OWN `MultiscaleLLN.link` (scripts/lib/layer_types.py:127-147, imported unmodified) behind
its own `ToPyramid.link`, over tests/golden/tf_standin.py -- the vectors that tests/lln_ref.py (the float64 restatement
the GPU tests are held to) is checked against in tests/test_lln_ref_cpu.py.

The stand-in has no `tf.pad`, which only this layer calls: the --emit child adds it to the stand-in MODULE OBJECT at run
time (zeros, the paddings given per axis); the stand-in file is not edited.  As with every stand-in op this pins the
Python the reference writes on top of the operators (filter, pad, crop, density, division), not TensorFlow's own
operator semantics.

    python tests/golden/lln_ref_graph.py --emit tests/golden/lln_ref_golden.npz      # REFERENCE side (build container only)

FIXTURE TOOLING.  Nothing here is on the product path; only the --emit child reads the reference tree.  The inputs are
regenerated from the seeds by `case_input`; the file holds the outputs, one array per case and scale.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_graph_golden as M

REF = M.REF

CASES = {
    '8x8': dict(shape=(8, 8, 3), n_scales=2, hypers={'σ': 3}, n=2, seed=41),
    '24x40': dict(shape=(24, 40, 3), n_scales=4, hypers={'σ': 1.5}, n=2, seed=42),
}


def case_input(case):
    rng = np.random.RandomState(2000 + case['seed'])
    return rng.random_sample((case['n'],) + tuple(case['shape']))


def emit(path):
    import torch
    import tf_standin
    # tf.pad(x, paddings): zeros, paddings[d] = [before, after] of axis d
    tf_standin.pad = lambda x, paddings: tf_standin.T(lambda ev: torch.nn.functional.pad(
        tf_standin._t(ev(x)), [p for before_after in reversed(paddings) for p in before_after]))
    sys.modules['tensorflow'] = tf_standin
    sys.path.insert(0, REF)
    import lib.layer_types as LT                      # the REFERENCE's module
    assert LT.__file__.startswith(REF)
    out = {}
    for key, case in sorted(CASES.items()):
        tf_standin.reset()
        x0 = tf_standin.placeholder(tf_standin.float32, (None,) + tuple(case['shape']))
        pyr = LT.ToPyramid(n_scales=case['n_scales'])
        pyr.link(x0, None, None)
        ℓ = LT.MultiscaleLLN(**case['hypers'])
        ℓ.link(pyr.x, None, None)
        vals = tf_standin.run(list(ℓ.x), {x0: case_input(case)})
        for i, v in enumerate(vals):
            out['%s/%d' % (key, i)] = np.asarray(v, np.float64)
        print(key, 'ok:', [v.shape for v in vals])
    np.savez_compressed(path, **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--emit', required=True)
    emit(ap.parse_args().emit)
