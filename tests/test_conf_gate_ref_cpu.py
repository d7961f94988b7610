"""CPU: the confidence-threshold exits without a GPU --

  * tests/conf_gate_ref.py (the numpy restatement of mpnn_conf_gate the GPU tests compare with) on cases written out by
    hand: ties, conf == tau, NaN and infinite thresholds, NaN confidences, exit_sink first, middle and last, sample lists;
  * the ctypes mirror of mpnn_conf_gate_args against the header as gcc lays it out, and the record check
    mpnn_conf_gate_check (pure host code: the library loads without a device);
  * the refusals of Net.predict / Net.predict_all(exit_conf=), which come before an engine is needed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import conf_gate_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')


# ---------------------------------------------------------------------------------- the reference, by hand
def test_threshold_and_equality():
    conf = np.array([0.2, 0.5, 0.7, 0.5], np.float32)
    r = np.array([[3, -1], [3, -1], [-2, 5], [0, 0]], np.float32)
    out = G.gate(conf, 0.5, r, 2, 0)
    assert [out['d'][i] for i in range(4)] == [1, 0, 0, 0]                       # (conf == tau leaves: >=)
    assert np.array_equal(out['rows'], [[0, 1], [1, 0], [1, 0], [1, 0]])
    assert np.array_equal(out['children'][0], [1, 2, 3]) and np.array_equal(out['children'][1], [0])
    # the threshold one float32 step above an occurring confidence: that image stays
    up = np.nextafter(np.float32(0.5), np.float32(1))
    assert [G.gate(conf, up, r, 2, 0)['d'][i] for i in range(4)] == [1, 1, 0, 1]


def test_router_chooses_among_the_children_first_index_on_ties():
    conf = np.zeros(5, np.float32)
    r = np.array([[9, 1, 2, 2],          # exit sink has the largest output: it is not a candidate; tie of 2 and 3 -> 2
                  [0, 0, 0, 0],          # all equal -> the first non-exit sink
                  [5, 7, -1, 7],         # tie of 1 and 3 -> 1
                  [0, -0.0, 0.0, -0.0],  # zeros of both signs are equal
                  [1, 2, 3, 4]], np.float32)
    out = G.gate(conf, 0.5, r, 4, 0)
    assert [out['d'][i] for i in range(5)] == [2, 1, 1, 1, 3]
    out = G.gate(conf, 0.5, r, 4, 1)                                              # exit_sink in the middle
    assert [out['d'][i] for i in range(5)] == [0, 0, 3, 0, 3]
    out = G.gate(conf, 0.5, r, 4, 3)                                              # exit_sink last
    assert [out['d'][i] for i in range(5)] == [0, 0, 1, 0, 2]
    out = G.gate(conf, 0.5, r, 3, 2)                                              # three sinks of a row of four: column 3 stays
    assert [out['d'][i] for i in range(5)] == [0, 0, 1, 0, 1]
    assert np.array_equal(out['rows'][:, 3], r[:, 3]) and np.array_equal(out['rows'][0, :3], [1, 0, 0])
    # every row is one-hot over the sinks, finite
    assert (out['rows'][:, :3].sum(1) == 1).all() and np.isfinite(out['rows']).all()


def test_nan_and_infinite_thresholds_and_confidences():
    conf = np.array([0.1, 0.9, NAN, INF, -INF], np.float32)
    r = np.tile(np.array([[0.0, 1.0, 2.0]], np.float32), (5, 1))
    d = lambda tau, ex=0: [G.gate(conf, tau, r, 3, ex)['d'][i] for i in range(5)]
    assert d(NAN) == [2, 2, 2, 2, 2]                                              # a NaN threshold: nobody leaves
    assert d(-INF) == [0, 0, 2, 0, 0]                                             # everybody but the NaN confidence
    assert d(INF) == [2, 2, 2, 0, 2]                                              # only an infinite confidence
    assert d(0.5) == [2, 0, 2, 0, 2]
    assert d(0.5, ex=2) == [1, 2, 1, 2, 1]
    # a NaN router output: as the first candidate it stays the maximum, as a later one it never wins
    rn = np.array([[0, NAN, 5], [0, 5, NAN]], np.float32)
    out = G.gate(np.zeros(2, np.float32), 0.5, rn, 3, 0)
    assert [out['d'][0], out['d'][1]] == [1, 1]
    assert np.isfinite(out['rows']).all()


def test_sample_list_count_and_untouched_rows():
    rng = np.random.default_rng(0)
    conf = rng.random(10).astype(np.float32)
    r = rng.standard_normal((10, 4)).astype(np.float32)
    idx = np.array([7, 2, 9, 4, 0, 1], np.int32)
    out = G.gate(conf, 0.5, r, 2, 0, idx=idx, cnt=4, n=6)
    assert out['imgs'] == [7, 2, 9, 4]
    rest = [i for i in range(10) if i not in out['imgs']]
    assert np.array_equal(out['rows'][rest], r[rest]) and np.array_equal(out['rows'][:, 2:], r[:, 2:])
    assert sorted(np.concatenate(out['children']).tolist()) == [2, 4, 7, 9]
    for img in out['imgs']:
        assert out['d'][img] == (0 if conf[img] >= np.float32(0.5) else 1)
    assert G.gate(conf, 0.5, r, 2, 0, idx=idx, cnt=9, n=6)['imgs'] == idx.tolist()          # (a count beyond the capacity)
    assert G.gate(conf, 0.5, r, 2, 0, idx=idx, cnt=0, n=6)['imgs'] == []
    assert G.gate(conf, 0.5, r, 2, 0, n=3)['imgs'] == [0, 1, 2]


# ---------------------------------------------------------------------------------- the C ABI boundary
def test_ctypes_record_matches_the_c_layout():
    from lib import _hip
    cls, cname = _hip.ConfGateArgs, 'mpnn_conf_gate_args'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpnn_hip.h"', 'int main(void){',
             'printf("%%zu", sizeof(%s));' % cname]
    lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f, _ in cls._fields_]
    lines.append('printf(" %d\\n", MPNN_MAX_SINKS); return 0;}')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'a.c'), os.path.join(d, 'a.out')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        nums = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert nums[0] == C.sizeof(cls)
    assert nums[1:-1] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert nums[-1] == _hip.MAX_SINKS == len(cls().child_idx) == len(cls().child_cnt)
    assert {'mpnn_conf_gate', 'mpnn_conf_gate_check'} <= set(_hip.EXPORTS)


def good_record():
    from lib import _hip
    a = _hip.ConfGateArgs()
    a.conf, a.tau, a.r, a.r_stride, a.n_sinks, a.exit_sink, a.n = 64, 128, 256, 4, 3, 1, 16
    return a


def test_record_check_refusals():
    from lib import _hip
    lib = _hip.load()
    chk = lambda a: lib.mpnn_conf_gate_check(C.byref(a))
    assert lib.mpnn_conf_gate_check(None) == _hip.E_ARG
    assert chk(good_record()) == 0
    for name in ('conf', 'tau', 'r'):
        a = good_record()
        setattr(a, name, None)
        assert chk(a) == _hip.E_ARG, name
    a = good_record(); a.r_stride = 2
    assert chk(a) == _hip.E_ARG                                   # rows narrower than the sinks
    a = good_record(); a.idx = 512
    assert chk(a) == _hip.E_ARG                                   # a list without its count
    a.cnt = 1024
    assert chk(a) == 0
    for which in ('child_idx', 'child_cnt'):                      # an unpaired child list, at any sink
        for i in range(_hip.MAX_SINKS):
            a = good_record()
            getattr(a, which)[i] = 2048
            assert chk(a) == _hip.E_ARG, (which, i)
            a.child_idx[i] = a.child_cnt[i] = 2048
            assert chk(a) == 0
    for S, ex in ((1, 0), (0, 0), (_hip.MAX_SINKS + 1, 0), (3, 3), (3, -1), (2, 2)):
        a = good_record(); a.n_sinks, a.exit_sink, a.r_stride = S, ex, 8
        assert chk(a) == _hip.E_SHAPE, (S, ex)
    for S in range(2, _hip.MAX_SINKS + 1):
        for ex in range(S):
            a = good_record(); a.n_sinks, a.exit_sink = S, ex
            assert chk(a) == 0
    # the launcher: nothing to do is no launch (and no error without a device), a NULL table is refused
    assert lib.mpnn_conf_gate(None, 0, 16, None) == 0 and lib.mpnn_conf_gate(None, 1, 0, None) == 0
    assert lib.mpnn_conf_gate(None, 1, 16, None) == _hip.E_ARG


# ---------------------------------------------------------------------------------- Net.predict(exit_conf=): refusals
def test_predict_refuses_bad_exit_conf_before_an_engine_is_needed():
    import arch_and_hypers as A
    net = A.ac_chain(k_cpt=1e-9)((32, 32, 3), (10,))
    x = np.zeros((2, 32, 32, 3), np.float32)
    assert net.gateable_leaves == list(range(7))                  # (every exit of the chain but the last)
    for call in (net.predict, net.predict_all):
        with pytest.raises(ValueError, match='8 leaves'):
            call(x, exit_conf=[0.5] * 7)
        with pytest.raises(ValueError, match='8 leaves'):
            call(x, exit_conf=np.full(9, 0.5))
        with pytest.raises(ValueError, match='real number'):
            call(x, exit_conf=[0.5] * 7 + ['0.5'])
        with pytest.raises(ValueError, match='real number'):
            call(x, exit_conf=[0.5, 1j] + [None] * 6)
        with pytest.raises(ValueError, match='real number'):
            call(x, exit_conf='0.5')
        with pytest.raises(ValueError, match='real number'):
            call(x, exit_conf=[[0.5] * 8])
    assert net._engine is None                                    # (none of the refusals built one)
    sr = A.sr_chain(2)((32, 32, 3), (10,))
    assert sr.gateable_leaves == []
    for call in (sr.predict, sr.predict_all):
        with pytest.raises(ValueError, match='nothing to gate'):
            call(x, exit_conf=0.5)
        with pytest.raises(ValueError, match='nothing to gate'):
            call(x, exit_conf=[None])
    assert sr._engine is None
    tree = A.ac_tree(k_cpt=1e-9)((32, 32, 3), (10,))
    leaves = list(tree.leaves)
    assert len(leaves) == 47
    # a leaf is gateable iff a router sits on the layer above it: in the tree every exit but the last of each of its 8 chains
    parent = {id(s): ℓ for ℓ in tree.layers for s in ℓ.sinks}
    assert tree.gateable_leaves == [k for k, ℓ in enumerate(leaves) if parent[id(ℓ)].router is not None]
    assert len(tree.gateable_leaves) == 47 - 8
    with pytest.raises(ValueError, match='47 leaves'):
        tree.predict(x, exit_conf=[0.5] * 8)


def test_checked_thresholds_one_entry_per_leaf():
    """What the engine receives: a float per gated leaf, None for the others -- ungateable leaves' entries are dropped."""
    import arch_and_hypers as A
    net = A.ac_chain(k_cpt=1e-9)((32, 32, 3), (10,))
    assert net._check_exit_conf('predict', None) is None
    assert net._check_exit_conf('predict', 0.5) == (0.5,) * 7 + (None,)
    assert net._check_exit_conf('predict', np.float32(0.25)) == (0.25,) * 7 + (None,)
    assert net._check_exit_conf('predict', 1) == (1.0,) * 7 + (None,)
    got = net._check_exit_conf('predict', [None, 0.5, -INF, INF, None, 2, np.float64(0.125), 0.9])
    assert got == (None, 0.5, -INF, INF, None, 2.0, 0.125, None)
    got = net._check_exit_conf('predict', np.array([0.5] * 8))
    assert got == (0.5,) * 7 + (None,)
    assert np.isnan(net._check_exit_conf('predict', NAN)[0])
