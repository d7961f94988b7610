"""CPU: what the engine decides about a net before its first launch (lib/_eng_structure.py: Structure) -- the tree
classification with its refusals, the conv and exit families, and the layout tables the device buffers are filled from.
Structure(net) is built here on a machine without a GPU; it loads the kernel library for its host-only *_check / *_tiles
entry points.

* The tables of every case of CASES equal tests/golden/engine_layout_golden.json, field by field and digest by digest.  The
  file was recorded from commit ecbe7d0 -- the last one whose Allocation._classify / Allocation._alloc_params interleaved
  this arithmetic with the device allocations -- by a throw-away script that ran those two methods on the CPU: an Engine
  made with object.__new__, given net, lib = _hip.load(), dev = torch.device('cpu') and _keep = [], with ValueRing of
  lib._eng_alloc replaced by a stub (the two upload rings were the only calls that needed a GPU).  The script put the
  tensors' numpy copies under the host names Structure uses and called record() of this module.  Per case the file holds
  the scalars, the per-block rows and a SHA-1 of every table; for sr_chain(3) on 32x32x3 the tables themselves as well.
* The flag tuples of tests/test_chan_nets.py::test_dispatch_is_decided_per_net, and the refusals of tests/test_rect_nets.py
  (pyramid step), tests/test_chan_nets.py (600 channels) and tests/test_harness_gpu.py (BatchNorm decays), without a GPU.
* One case for every other refusal of _classify / _layout, and for those of _kind / refuse_activity they call; nets that
  the constructors of arch_and_hypers.py cannot make are made by editing a built net's root / comps / sinks / router.

Two refusals of _classify cannot be reached, because an earlier one of the same function catches their nets:
  'block below a %s node'           -- a block's parent that is neither the pyramid nor a block is a head, and a head with
                                       sinks is refused by the first loop ('LogReg with sinks');
  'more than %d sinks under one switch' -- a switch with more than MAX_SINKS sinks makes max_sinks > MAX_SINKS, which
                                       'routing tree too large for mpnn_route' refuses."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from lib import _hip
from lib._eng_structure import Structure

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from chan_ref_graph import NARROW, ODD
from superclass_ref import hard_map

GOLDEN = os.path.join(HERE, 'golden', 'engine_layout_golden.json')
FULL = 'sr3_32x32x3'                                  # the case whose tables the file holds in full
TABLES = ('seg', 'pack_desc', 'bn_table', 'node_tab', 'kid_tab', 'node_ops', 'leaf_node_tab', 'curve_tree', 'w_eq')

AC = dict(ctor='ac_chain', hypers=dict(k_cpt=1.6e-8))
SR3 = dict(ctor='sr_chain', args=(3,))
# case -> ctor (of arch_and_hypers), args / hypers of the constructor, shape, classes, knobs (module variables of
# arch_and_hypers, read when the constructor is called), env (read by Structure)
CASES = {
    'sr3_32x32x3': dict(SR3),
    'sr3_24x24x3': dict(SR3, shape=(24, 24, 3)),
    'sr3_32x32x2': dict(SR3, shape=(32, 32, 2)),
    'ac_32x32x3': dict(AC),
    'ac_24x40x3': dict(AC, shape=(24, 40, 3)),
    'ac_100_classes': dict(AC, n_cls=100),
    'ac_tree': dict(ctor='ac_tree', hypers=dict(k_cpt=1e-9)),
    'cr_tree': dict(ctor='cr_tree', hypers=dict(k_cpt=1e-9)),
    'ac_dp_buckets_3': dict(AC, env={'MPNN_DP_BUCKETS': '3'}),
    'ac_dp_buckets_2': dict(AC, env={'MPNN_DP_BUCKETS': '2'}),
    'ac_dp_buckets_3_no_overlap': dict(AC, env={'MPNN_DP_BUCKETS': '3', 'MPNN_DP_OVERLAP': '0'}),
    'ac_supp_5': dict(AC, knobs=dict(conv_supp=5)),
    'ac_24x40x3_supp_5': dict(AC, shape=(24, 40, 3), knobs=dict(conv_supp=5)),
    'ac_odd_16x16x2': dict(AC, shape=(16, 16, 2), knobs=dict(arch=ODD)),
    'sr_narrow_8x8x5': dict(SR3, shape=(8, 8, 5), knobs=dict(arch=NARROW)),
    'ac_superclass_heads': dict(AC, knobs=dict(arch=4, coarse_exits={1: hard_map(10, 2), 2: hard_map(10, 5), 3: hard_map(10, 2)})),
    'ac_squared_heads': dict(AC, knobs=dict(arch=4, exit_loss={0: 'squared', 2: 'squared-linear'})),
    'ac_lln': dict(AC, knobs=dict(lln={})),
    'sr3_generic_convs': dict(SR3, env={'MPNN_GENERIC_CONVS': '1'}),
    'sr3_anymap_convs': dict(SR3, env={'MPNN_ANYMAP_CONVS': '1'}),
    'sr3_anychan_convs': dict(SR3, env={'MPNN_ANYCHAN_CONVS': '1'}),
    'sr3_generic_exits': dict(SR3, env={'MPNN_GENERIC_EXITS': '1'}),
}
ENV = ('MPNN_DP_BUCKETS', 'MPNN_DP_OVERLAP', 'MPNN_GENERIC_CONVS', 'MPNN_ANYMAP_CONVS', 'MPNN_ANYCHAN_CONVS', 'MPNN_GENERIC_EXITS')


def make(case, mp):
    """The net of a case, built under its knobs, with the case's environment set on the monkeypatch `mp` (a Structure of
    the net must be built before `mp` is undone)."""
    import arch_and_hypers as A
    c = CASES[case] if isinstance(case, str) else case
    for name in ENV:
        mp.delenv(name, raising=False)
    for name, v in c.get('env', {}).items():
        mp.setenv(name, v)
    for name, v in c.get('knobs', {}).items():
        mp.setattr(A, name, A.arch[:v] if name == 'arch' and isinstance(v, int) else v)
    ctor = getattr(A, c['ctor'])(*c.get('args', ()), **c.get('hypers', {}))
    return ctor(tuple(c.get('shape', (32, 32, 3))), (c.get('n_cls', 10),))


def flags(s):
    return (s.generic_convs, s.anymap_convs, s.anychan_convs, s.generic_exits)


def tables(s):
    """name -> the host table as a numpy array in the element type of its device tensor."""
    return {'seg': s.seg_host, 'pack_desc': s.pack_desc_host, 'bn_table': s.bn_table_host, 'node_tab': s.node_tab_host,
            'kid_tab': s.kid_tab_host, 'node_ops': np.asarray(s.node_ops_host, np.float32), 'leaf_node_tab': s.leaf_node_tab_host,
            'curve_tree': np.frombuffer(bytes(s.curve_tree), np.int32),
            'w_eq': s.w_eq_host if s.w_eq_host is not None else np.zeros(0, np.float32)}


def record(s, full=False):
    """What the golden file holds of a Structure (or of anything with its attributes), as JSON gives it back."""
    tabs = tables(s)
    want = {'seg': np.int32, 'pack_desc': np.int32, 'bn_table': np.int32, 'node_tab': np.int32, 'kid_tab': np.int32,
            'node_ops': np.float32, 'leaf_node_tab': np.int32, 'curve_tree': np.int32, 'w_eq': np.float32}
    assert tuple(tabs) == TABLES and all(tabs[k].dtype == want[k] and tabs[k].ndim == 1 for k in TABLES)
    rec = dict(flags=flags(s), n_params=s.n_params, stat_pad=s.stat_pad, n_seg=s.n_seg, n_pack=s.n_pack, n_bn=s.n_bn,
               dp_cut_block=s.dp_cut_block, dp_buckets=s.dp_buckets, seg_range=s.seg_range, bn_decay=s.bn_decay,
               max_sinks=s.max_sinks,
               blocks=[[b.C, b.H, b.W, b.in_map, b.in_shift, b.has_dz, b.sum_off, b.n_out, b.lmap, b.loss] for b in s.blocks],
               sha1={k: hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in tabs.items()})
    if full:
        rec['tables'] = {k: v.tolist() for k, v in tabs.items()}
    return json.loads(json.dumps(rec, default=int))


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES) and 'tables' in golden[FULL]


@pytest.mark.parametrize('case', list(CASES))
def test_tables_equal_the_recorded_ones(case, golden, monkeypatch):
    got, want = record(Structure(make(case, monkeypatch)), full=case == FULL), golden[case]
    assert sorted(got) == sorted(want)
    for field in want:
        if field in ('sha1', 'tables'):
            for name in TABLES:
                assert got[field][name] == want[field][name], (field, name)
        else:
            assert got[field] == want[field], field


def test_structure_is_a_function_of_the_net_and_the_environment(monkeypatch):
    """A second Structure of the same net writes the same offset / node / is_router on the net's parameters."""
    net = make('ac_dp_buckets_3', monkeypatch)
    a = Structure(net)
    first = [(p.offset, getattr(p, 'node', None), getattr(p, 'is_router', None)) for p in net._all_params]
    b = Structure(net)
    assert first == [(p.offset, getattr(p, 'node', None), getattr(p, 'is_router', None)) for p in net._all_params]
    assert record(a) == record(b)


def test_structure_calls_nothing_of_torch():
    with open(os.path.join(os.path.dirname(HERE), 'multipath-nn_amd', 'lib', '_eng_structure.py')) as f:
        assert 'torch' not in f.read()


# ------------------------------------------------------------------ dispatch
def test_dispatch_is_decided_per_net(monkeypatch):
    """The flag tuples of tests/test_chan_nets.py::test_dispatch_is_decided_per_net."""
    f = lambda **c: flags(Structure(make(dict(SR3, **c), monkeypatch)))[:3]
    assert f(shape=(32, 32, 3)) == (False, False, False)
    assert f(shape=(32, 32, 1)) == (False, False, False)
    assert f(shape=(24, 24, 3)) == (True, True, False)
    assert f(shape=(32, 32, 2)) == (True, True, True)              # the image's channels count
    assert f(shape=(16, 16, 3), knobs=dict(arch=ODD)) == (True, True, True)


# ------------------------------------------------------------------ refusals
def refused(net, match):
    with pytest.raises(NotImplementedError, match=match):
        Structure(net)


def _blocks(net):
    return [ℓ for ℓ in net.layers if ℓ.name == 'ReConvMax']


def _heads(net):
    return [ℓ for ℓ in net.layers if ℓ.name == 'LogReg']


def test_image_that_is_no_multiple_of_the_pyramid_step_is_refused(monkeypatch):
    for shape in [(30, 30, 3), (24, 30, 3), (30, 24, 3), (36, 36, 3)]:
        refused(make(dict(SR3, shape=shape), monkeypatch),
                r'pyramid of 4 scales .* multiples of 8 .* %dx%d image' % shape[:2])
    refused(make(dict(SR3, shape=(512, 512, 3)), monkeypatch), r'at most 256')


def test_a_600_channel_block_is_refused(monkeypatch):
    net = make(dict(ctor='sr_chain', args=(2,), shape=(16, 16, 3), knobs=dict(arch=[[16, 16, 600], [16, 16, 32]])), monkeypatch)
    refused(net, r'600 channels.*1\.\.512 channels')


def test_conv_batchnorms_with_different_decays_are_refused(monkeypatch):
    net = make(dict(AC, hypers=dict(k_cpt=1e-9, seed=3)), monkeypatch)
    _blocks(net)[1].comps[1].comps[0].hypers.d = 0.5
    refused(net, r'different moving-average decays \[0\.5, 0\.9\].*one decay per net')


def test_tree_too_large_for_the_route_kernel(monkeypatch):
    import arch_and_hypers as A
    from lib.net_types import ActorNet
    make(dict(AC), monkeypatch)
    five = A.rcm(0, *[A.reg(10) for _ in range(_hip.MAX_SINKS + 1)])
    refused(ActorNet(x0_shape=(32, 32, 3), y_shape=(10,), root=A.pyr(five)), 'routing tree too large for mpnn_route')
    # ... and a chain of more than MAX_NODES nodes
    monkeypatch.setattr(A, 'arch', [[16]] * _hip.MAX_NODES)
    refused(A.sr_chain(_hip.MAX_NODES)((8, 8, 3), (10,)), 'routing tree too large for mpnn_route')


def test_router_in_an_srnet_or_on_one_sink(monkeypatch):
    import arch_and_hypers as A
    net = make(dict(SR3), monkeypatch)
    _blocks(net)[0].router = A.router(2)
    refused(net, r'router on a node with < 2 sinks / in an SRNet')
    net = make(dict(AC), monkeypatch)
    _blocks(net)[-1].router = A.router(2)                  # (the last block of the chain has one sink)
    refused(net, r'router on a node with < 2 sinks / in an SRNet')


def test_router_chain_of_another_shape(monkeypatch):
    net = make(dict(AC), monkeypatch)
    r = _blocks(net)[2].router
    r.comps = r.comps[:4] + r.comps[7:]                    # one hidden layer
    refused(net, 'router chain outside the MI355X hot path')


def test_activity_error_in_a_router_or_a_block(monkeypatch):
    from lib.layer_types import ActivityError
    net = make(dict(AC), monkeypatch)
    r = _blocks(net)[1].router
    r.comps = list(r.comps) + [ActivityError(α=0.1)]
    refused(net, r"the router of layer 'ReConvMax': ActivityError runs in a LogReg chain only")
    net = make(dict(AC), monkeypatch)
    b = _blocks(net)[1]
    b.comps = list(b.comps) + [ActivityError(α=0.1)]
    refused(net, r"layer 'ReConvMax': ActivityError runs in a LogReg chain only")


def test_layer_that_is_no_node_of_the_hot_path(monkeypatch):
    net = make(dict(AC), monkeypatch)
    b = _blocks(net)[3]
    b.comps = b.comps[:2]                                  # (no MultiscaleRect)
    refused(net, r"layer 'ReConvMax' \(Chain\) is outside the MI355X hot path: supported tree nodes")


def test_router_on_the_pyramid(monkeypatch):
    import arch_and_hypers as A
    from lib.net_types import ActorNet
    make(dict(AC), monkeypatch)
    root = A.pyr(A.rcm(0, A.reg(10)), A.rcm(0, A.reg(10)))
    refused(ActorNet(x0_shape=(32, 32, 3), y_shape=(10,), root=root), 'router on a pyramid node')


def test_switch_without_router(monkeypatch):
    net = make(dict(AC), monkeypatch)
    _blocks(net)[0].router = None
    refused(net, 'switch without router')


def test_head_with_sinks(monkeypatch):
    import arch_and_hypers as A
    net = make(dict(SR3), monkeypatch)
    _heads(net)[0].sinks = (A.reg(10),)
    refused(net, 'LogReg with sinks')


def test_root_that_is_no_pyramid(monkeypatch):
    net = make(dict(SR3), monkeypatch)
    net.root = net.root.sinks[0]
    refused(net, 'root must be the ToPyramid chain')


def test_lln_on_other_than_three_channels(monkeypatch):
    """(MultiscaleLLN.link itself refuses both for a net built through the constructors.)"""
    net = make(dict(SR3, knobs=dict(lln={})), monkeypatch)
    net.hypers.x0_shape = (32, 32, 1)
    refused(net, 'MultiscaleLLN on other than the scales of a 3-channel ToPyramid')
    net = make(dict(SR3, knobs=dict(lln={})), monkeypatch)
    net.root.comps[1].in_shifts = [1, 2, 3, 4]
    refused(net, 'MultiscaleLLN on other than the scales of a 3-channel ToPyramid')


def test_two_heads_under_one_block(monkeypatch):
    import arch_and_hypers as A
    from lib.net_types import ActorNet
    make(dict(AC), monkeypatch)
    root = A.pyr(A.rcm(0, A.reg(10), A.reg(10)))
    refused(ActorNet(x0_shape=(32, 32, 3), y_shape=(10,), root=root), 'more than one LogReg under a block')


def test_exit_beyond_the_any_width_kernels(monkeypatch):
    refused(make(dict(SR3, n_cls=2000), monkeypatch),
            r'exit on a 4x4x32 map with 2000 classes and a 0-0 router: outside the any-width exit kernels too')
    monkeypatch.setattr('arch_and_hypers.router_n_chan', 300)
    refused(make(dict(AC), monkeypatch), r'a 300-300 router: outside the any-width exit kernels too .*<= 256 units')


def test_head_under_the_pyramid(monkeypatch):
    import arch_and_hypers as A
    from lib.net_types import SRNet
    make(dict(SR3), monkeypatch)
    net = SRNet(x0_shape=(32, 32, 3), y_shape=(10,), root=A.pyr(A.rcm(0, A.reg(10))))
    net.root.sinks = (_heads(net)[0],)
    refused(net, 'LogReg must hang off a ReConvMax block')
