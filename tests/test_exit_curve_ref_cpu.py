"""CPU: the threshold curve without a GPU --

  * tests/exit_curve_ref.py (the numpy restatement of mpnn_exit_curve the GPU tests compare with) on cases whose answers are
    written out here: a 3-exit chain, a static 3-exit chain, a 3-sink switch whose "no" branch picks among two children,
    conf == tau, NaN confidences, infinite and NaN thresholds, a router tie;
  * the ctypes mirrors of mpnn_exit_curve_args / mpnn_curve_node against the header as gcc lays it out, and the refusals of
    mpnn_exit_curve_check and of the launcher (pure host code: the library loads without a device);
  * the refusals of Net.exit_conf_curve, which come before an engine is needed; Net.threshold_exits; tau_for_ops."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import exit_curve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
N = R.node


def chain3(static=False):
    """root -> A{exit 0, B{exit 1, C -> exit 2}}; node_ops 1, 10, 100, 1000, 10000, 100000, 1000000."""
    sw = (lambda k: -1) if static else (lambda k: k)
    tree = [N([1]), N([2, 3], sw(0), exit=0), N(leaf=0), N([4, 5], sw(1), exit=0), N(leaf=1), N([6]), N(leaf=2)]
    return tree, [10 ** k for k in range(7)]


OPS0, OPS1, OPS2 = 111, 11011, 1101011            # (the paths root-A-exit0, root-A-B-exit1, root-A-B-C-exit2)


# ---------------------------------------------------------------------------------- the reference, by hand
@pytest.mark.parametrize('static', [False, True])
def test_three_exit_chain(static):
    tree, ops = chain3(static)
    conf = np.array([[0.9, 0.4, 0.4, 0.2], [0.3, 0.8, 0.5, 0.1], [0.0, 0.0, 0.0, 0.0]], np.float32)
    d_cor = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [1, 1, 0, 1]], np.float32)
    r = np.zeros((2, 4, 2), np.float32)
    r[:, :, 1] = 1                                  # the learnt routers send everybody on (never read below: all gated)
    taus = [0.5, 0.95, 0.0]
    correct, o, hist = R.curve(tree, ops, conf, d_cor, r, taus, 4)
    # tau 0.5 : image 0 leaves at 0 (right), 1 at 1 (right), 2 at 1 (conf == tau leaves; right), 3 at 2 (right)
    # tau 0.95: everybody at 2: right are images 0, 1, 3;   tau 0: everybody at 0: right are images 0 and 2
    assert hist.tolist() == [[1, 2, 1], [0, 0, 4], [4, 0, 0]]
    assert correct.tolist() == [4, 3, 2]
    assert o.tolist() == [OPS0 + 2 * OPS1 + OPS2, 4 * OPS2, 4 * OPS0]
    # per-leaf rows: NaN leaves a switch to its router (which sends everybody on) and passes a static fork by
    rows = np.array([[NAN, 0.5, NAN], [0.5, NAN, NAN]], np.float32)
    correct, o, hist = R.curve(tree, ops, conf, d_cor, r, rows, 4)
    assert hist.tolist() == [[0, 2, 2], [1, 0, 3]]
    assert correct.tolist() == [4, 3]              # row 0: 1 and 2 right at exit 1, 0 and 3 at exit 2; row 1: 0 at exit 0, 1 and 3 at exit 2
    assert o.tolist() == [2 * OPS1 + 2 * OPS2, OPS0 + 3 * OPS2]


def test_learnt_policy_of_a_chain_and_a_router_that_leaves():
    tree, ops = chain3()
    conf = np.full((3, 3), 0.5, np.float32)
    d_cor = np.array([[1, 1, 1], [0, 0, 0], [0, 1, 0]], np.float32)
    r = np.array([[[2, 1], [0, 1], [0, 1]],        # switch A: image 0 leaves (sink 0 is the exit), 1 and 2 go on
                  [[0, 0], [5, 1], [1, 5]]], np.float32)      # switch B: image 1 leaves at exit 1, image 2 goes to exit 2
    correct, o, hist = R.curve(tree, ops, conf, d_cor, r, np.full((1, 3), NAN), 3)
    assert hist.tolist() == [[1, 1, 1]] and correct.tolist() == [1] and o.tolist() == [OPS0 + OPS1 + OPS2]
    # gated and refused, the router's own wish for the exit sink does not count: image 0 goes on to B, where it ties -> sink 0
    correct, o, hist = R.curve(tree, ops, conf, d_cor, r, [0.75], 3)
    assert hist.tolist() == [[0, 0, 3]]            # (B is gated too: its "no" is the one other sink)
    correct, o, hist = R.curve(tree, ops, conf, d_cor, r, np.array([[0.75, NAN, NAN]]), 3)
    assert hist.tolist() == [[0, 2, 1]]            # (B by its router: image 0's tie takes the first index, the exit)


def tree3():
    """root -> S{exit 0, X -> exit 1, Y -> exit 2}: a 3-sink switch with its exit in the MIDDLE sink."""
    tree = [N([1]), N([2, 3, 4], 0, exit=1), N([5]), N(leaf=0), N([6]), N(leaf=1), N(leaf=2)]
    return tree, [1, 10, 100, 1000, 10000, 100000, 1000000]


def test_three_sink_switch_no_branch_picks_among_the_children_and_ties():
    tree, ops = tree3()
    # leaves in node order: node 3 = leaf 0 (the exit, sink 1), node 5 = leaf 1 (below X, sink 0), node 6 = leaf 2 (below Y, sink 2)
    conf = np.array([[0.9, 0.1, 0.1, 0.1, NAN], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
    d_cor = np.array([[1, 1, 1, 1, 1], [0, 1, 0, 1, 0], [0, 0, 1, 0, 0]], np.float32)
    r = np.array([[[1, 9, 2],                       # leaves by confidence
                   [1, 9, 2],                       # refused: the exit's 9 is no candidate, sink 2 (Y) wins
                   [3, 9, 3],                       # refused: tie of the children -> the first, sink 0 (X)
                   [4, 9, 3],                       # refused: X
                   [0, 9, 5]]], np.float32)         # NaN confidence: refused at any threshold, Y
    correct, o, hist = R.curve(tree, ops, conf, d_cor, r, [0.5, -INF, INF, NAN], 5)
    X, Y, E = 1 + 10 + 100 + 100000, 1 + 10 + 10000 + 1000000, 1 + 10 + 1000
    assert hist.tolist() == [[1, 2, 2], [4, 0, 1], [0, 2, 3], [5, 0, 0]]
    #  0.5 : E, Y, X, X, Y     -inf: E E E E, Y (the NaN confidence stays)    +inf: Y Y X X Y    NaN: the router, sink 1 = E for all
    assert o.tolist() == [E + 2 * X + 2 * Y, 4 * E + Y, 2 * X + 3 * Y, 5 * E]
    assert correct.tolist() == [1 + 0 + 0 + 1 + 0, 4, 0 + 0 + 0 + 1 + 0, 5]


def test_thresholds_at_and_one_step_above_a_confidence():
    tree, ops = chain3(static=True)
    conf = np.array([[0.5], [0.25], [0]], np.float32)
    d_cor = np.ones((3, 1), np.float32)
    r = np.zeros((0, 1, 2), np.float32)
    up = np.nextafter(np.float32(0.5), np.float32(1))
    _, _, hist = R.curve(tree, ops, conf, d_cor, r, [0.5, up, 0.25], 1)
    assert hist.tolist() == [[1, 0, 0], [0, 0, 1], [1, 0, 0]]
    _, _, hist = R.curve(tree, ops, conf, d_cor, r, np.array([[up, 0.25, NAN], [NAN, NAN, NAN], [INF, -INF, 0]]), 1)
    assert hist.tolist() == [[0, 1, 0], [0, 0, 1], [0, 1, 0]]          # (an all-NaN row passes every static fork by)


# ---------------------------------------------------------------------------------- the C ABI boundary
@pytest.mark.parametrize('name,cname', [('ExitCurveArgs', 'mpnn_exit_curve_args'), ('CurveNode', 'mpnn_curve_node')])
def test_ctypes_records_match_the_c_layout(name, cname):
    from lib import _hip
    cls = getattr(_hip, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpnn_hip.h"', 'int main(void){',
             'printf("%%zu", sizeof(%s));' % cname]
    lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f, _ in cls._fields_]
    lines.append('printf(" %d %d\\n", MPNN_MAX_SINKS, MPNN_MAX_NODES); return 0;}')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'a.c'), os.path.join(d, 'a.out')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        nums = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert nums[0] == C.sizeof(cls)
    assert nums[1:-2] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert nums[-2] == _hip.MAX_SINKS == len(_hip.CurveNode().sink) and nums[-1] == _hip.MAX_NODES
    assert {'mpnn_exit_curve', 'mpnn_exit_curve_check'} <= set(_hip.EXPORTS)


def host_tree(tree):
    from lib import _hip
    arr = (_hip.CurveNode * len(tree))()
    for q, nd in zip(arr, tree):
        q.n_sinks, q.switch_id, q.leaf_id, q.exit_sink = len(nd['sinks']), nd['switch'], nd['leaf'], nd['exit']
        for i, s in enumerate(nd['sinks'][:4]):
            q.sink[i] = s
    return arr


def good_record(tree, n=16):
    from lib import _hip
    a = _hip.ExitCurveArgs()
    a.n, a.n_nodes, a.n_leaves = n, len(tree), sum(1 for nd in tree if not nd['sinks'])
    a.n_switches, a.n_points, a.tau_per_leaf = 1 + max([nd['switch'] for nd in tree]), 3, 1
    a.tree, a.node_ops, a.conf, a.d_cor, a.r, a.taus, a.correct, a.ops, a.hist = (64 * k for k in range(1, 10))
    a.conf_stride, a.dcor_stride, a.r_stride, a.r_switch_stride = n, n + 3, 4, 4 * n
    return a


def test_record_check_refusals():
    from lib import _hip
    lib = _hip.load()
    chk = lambda a, t: lib.mpnn_exit_curve_check(C.byref(a), host_tree(t))
    tree, _ = tree3()
    assert lib.mpnn_exit_curve_check(None, host_tree(tree)) == _hip.E_ARG
    assert lib.mpnn_exit_curve_check(C.byref(good_record(tree)), None) == _hip.E_ARG
    for t in (tree, chain3()[0], chain3(static=True)[0]):
        assert chk(good_record(t), t) == 0
    for name in ('tree', 'node_ops', 'conf', 'd_cor', 'r', 'taus', 'correct', 'ops', 'hist'):
        a = good_record(tree)
        setattr(a, name, None)
        assert chk(a, tree) == _hip.E_ARG, name
    st = chain3(static=True)[0]
    a = good_record(st); a.r = None
    assert chk(a, st) == 0                                          # (no switch: no router outputs)
    for name, v in (('n_nodes', 0), ('n_nodes', _hip.MAX_NODES + 1), ('n_leaves', 0), ('n_leaves', 8), ('n_switches', -1),
                    ('n_switches', _hip.MAX_NODES // 2 + 1), ('n_points', 0), ('n', -1)):
        a = good_record(tree)
        setattr(a, name, v)
        assert chk(a, tree) == _hip.E_SHAPE, (name, v)
    for name, v in (('conf_stride', 15), ('dcor_stride', 15), ('r_stride', 2), ('r_switch_stride', 63)):
        a = good_record(tree)
        setattr(a, name, v)
        assert chk(a, tree) == _hip.E_ARG, (name, v)
    a = good_record(tree); a.n = 0; a.conf_stride = a.dcor_stride = 0; a.r_switch_stride = 0
    assert chk(a, tree) == 0

    def broken(edit):
        t = [dict(nd, sinks=list(nd['sinks'])) for nd in tree3()[0]]
        edit(t)
        return chk(good_record(tree), t)
    assert broken(lambda t: t[1]['sinks'].__setitem__(0, 1)) == _hip.E_SHAPE       # a sink that is the node itself
    assert broken(lambda t: t[1]['sinks'].__setitem__(0, 7)) == _hip.E_SHAPE       # ... beyond the table
    assert broken(lambda t: t[4]['sinks'].__setitem__(0, 2)) == _hip.E_SHAPE       # ... in front of its parent
    assert broken(lambda t: t[1]['sinks'].extend([5, 6])) == _hip.E_SHAPE          # five sinks
    assert broken(lambda t: t[3].update(leaf=-1)) == _hip.E_SHAPE                  # a leaf without its id
    assert broken(lambda t: t[3].update(leaf=3)) == _hip.E_SHAPE
    assert broken(lambda t: t[5].update(leaf=0)) == _hip.E_SHAPE                   # two leaves with one id
    assert broken(lambda t: t[2].update(leaf=1)) == _hip.E_SHAPE                   # an inner node with a leaf id
    assert broken(lambda t: t[1].update(switch=1)) == _hip.E_SHAPE                 # a switch id beyond n_switches
    assert broken(lambda t: t[2].update(switch=0)) == _hip.E_SHAPE                 # a router on a node with one sink
    assert broken(lambda t: t[1].update(exit=3)) == _hip.E_SHAPE
    assert broken(lambda t: t[1].update(exit=0)) == _hip.E_SHAPE                   # an exit sink that is no leaf
    assert broken(lambda t: t[2].update(exit=0)) == _hip.E_SHAPE                   # ... on a node with one sink
    assert broken(lambda t: t[1].update(exit=-1)) == 0                             # a switch without an exit: its router decides
    # static nodes with two or more sinks: only "one leaf + one other"
    assert broken(lambda t: t[1].update(switch=-1)) == _hip.E_SHAPE                # three sinks
    two = lambda ex: [N([1]), N([2, 3], -1, exit=ex), N(leaf=0), N([4]), N(leaf=1)]
    assert chk(good_record(two(0)), two(0)) == 0
    assert chk(good_record(two(0)), two(-1)) == _hip.E_SHAPE                       # nothing decides
    both = [N([1]), N([2, 3], -1, exit=0), N(leaf=0), N(leaf=1)]
    assert chk(good_record(both), both) == _hip.E_SHAPE                            # two leaves
    # the launcher: nothing to do is no launch (and no error without a device); what it can see it refuses itself
    a = good_record(tree); a.n = 0
    assert lib.mpnn_exit_curve(C.byref(a), None) == 0
    assert lib.mpnn_exit_curve(None, None) == _hip.E_ARG
    a = good_record(tree); a.hist = None
    assert lib.mpnn_exit_curve(C.byref(a), None) == _hip.E_ARG
    a = good_record(tree); a.n_points = 0
    assert lib.mpnn_exit_curve(C.byref(a), None) == _hip.E_SHAPE
    a = good_record(tree); a.conf_stride = 3
    assert lib.mpnn_exit_curve(C.byref(a), None) == _hip.E_ARG


# ---------------------------------------------------------------------------------- Net.exit_conf_curve: the host side
def test_threshold_exits():
    import arch_and_hypers as A
    net = A.ac_chain(k_cpt=1e-9)((32, 32, 3), (10,))
    assert net.threshold_exits == list(range(7)) == net.gateable_leaves
    ds = R.ds_chain(3)
    assert ds.threshold_exits == [0, 1] and ds.gateable_leaves == []           # (the last exit hangs under a block with one sink)
    assert R.ds_chain(1).threshold_exits == []
    assert A.sr_chain(2)((32, 32, 3), (10,)).threshold_exits == []
    tree = A.ac_tree(k_cpt=1e-9)((32, 32, 3), (10,))
    assert tree.threshold_exits == tree.gateable_leaves


def test_refusals_come_before_an_engine():
    import arch_and_hypers as A
    from lib.layer_types import Chain, Conv, CrossEntropyError, LinTrans, Rect, Softmax
    from lib.net_types import SRNet
    net = A.ac_chain(k_cpt=1e-9)((32, 32, 3), (10,))
    x = np.zeros((4, 32, 32, 3), np.float32)
    y = np.eye(10, dtype=np.float32)[[0, 1, 2, 3]]
    for taus, match in ((0.5, r'\[T\]'), (np.zeros((2, 7)), '8'), (np.zeros((2, 9)), '8'), (np.zeros((2, 8, 1)), r'\[T\]'),
                        (np.zeros(0), 'T = 0'), (np.zeros((0, 8)), 'T = 0'), (['0.5'], 'real'), ([0.5, 1j], 'real'),
                        ([None, 0.5], 'real'), ([True, False], 'real'), ('0.5', 'real')):
        with pytest.raises(ValueError, match=match):
            net.exit_conf_curve(x, y, taus)
    for yy in (None, y[:3], y[:, :9], np.zeros(4, np.int64)):
        with pytest.raises(ValueError, match='labels'):
            net.exit_conf_curve(x, yy, [0.5])
    with pytest.raises(ValueError):
        net.exit_conf_curve(x, y, [0.5], decode='gamma')                       # float images with a decode table
    with pytest.raises(ValueError, match='batch'):
        net.exit_conf_curve(x, y, [0.5], batch=0)
    with pytest.raises(ValueError, match='k_cpt'):
        net.exit_conf_curve(x, y, [0.5], k_cpt=1e-9)                           # (a fixed k_cpt)
    dyn = A.cr_chain(dyn_k_cpt=True)((32, 32, 3), (10,))
    with pytest.raises(ValueError, match='k_cpt'):
        dyn.exit_conf_curve(x, y, [0.5])
    assert net._engine is None and dyn._engine is None
    sr = A.sr_chain(2)((32, 32, 3), (10,))
    with pytest.raises(ValueError, match='no exit a threshold applies to'):
        sr.exit_conf_curve(x, y, [0.5])
    assert sr._engine is None
    # a static fork with several child blocks: nothing chooses among them
    blk = lambda i, *s: Chain(name='ReConvMax', sinks=s, comps=A.rcm(i).comps)
    fork = SRNet(x0_shape=(32, 32, 3), y_shape=(10,),
                 root=A.pyr(blk(0, A.reg(10), blk(1, A.reg(10)), blk(1, A.reg(10)))))
    with pytest.raises(ValueError, match='static fork'):
        fork.exit_conf_curve(x, y, [0.5])
    fork2 = SRNet(x0_shape=(32, 32, 3), y_shape=(10,), root=A.pyr(blk(0, blk(1, A.reg(10)), blk(1, A.reg(10)))))
    with pytest.raises(ValueError, match='static fork'):
        fork2.exit_conf_curve(x, y, [0.5])
    assert fork._engine is None and fork2._engine is None
    conv = SRNet(x0_shape=(8, 8, 3), y_shape=(10,),
                 root=Chain(comps=[Conv(n_chan=16, supp=3), Rect()],
                            sinks=[Chain(comps=[LinTrans(n_chan=10), Softmax(), CrossEntropyError()])]))
    with pytest.raises(NotImplementedError, match='ConvEngine'):
        conv.exit_conf_curve(np.zeros((4, 8, 8, 3), np.float32), y, [0.5])
    assert conv._engine is None


def test_tau_for_ops():
    from lib.net_types import _Curve
    taus = np.array([0.1, 0.5, 0.7, 0.9, 0.99], np.float32)
    c = _Curve(n=100, taus=None, correct=None, ops=None, hist=None, _points=taus,
               acc=np.array([0.60, 0.80, 0.80, 0.85, 0.84]), moc=np.array([10.0, 20.0, 30.0, 40.0, 50.0]))
    best = c.tau_for_ops(100.0)
    assert (best.index, best.acc, best.moc) == (3, 0.85, 40.0) and best.tau == float(taus[3])
    assert c.tau_for_ops(40.0).index == 3 and c.tau_for_ops(39.9).index == 1          # (a tie: the first, the cheaper point)
    assert c.tau_for_ops(10.0).index == 0 and c.tau_for_ops(9.9) is None
    rows = _Curve(n=1, taus=None, correct=None, ops=None, hist=None, _points=None, acc=np.ones(1), moc=np.ones(1))
    with pytest.raises(ValueError, match='per-leaf'):
        rows.tau_for_ops(1.0)
