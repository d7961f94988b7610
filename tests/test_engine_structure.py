"""GPU: the engine's device tables are the host tables of lib/_eng_structure.py (no kernel runs).  For three nets -- sr_chain(3)
on 32x32x3, the actor chain on the ODD table over 16x16x2 images, the shipped actor chain under MPNN_DP_BUCKETS=3 -- every
table of net.engine(), copied back, equals the table of a fresh Structure built on a twin net (whose own values
tests/test_engine_structure_cpu.py holds against the recorded ones); the views p.data, p.grad and p.accum start at p.offset
in P, G and A; and a Structure built beside a live engine leaves the parameters' offset / node / is_router as they are."""
import ctypes as C

import numpy as np
import pytest

from lib._eng_structure import Structure
from test_engine_structure_cpu import make

pytestmark = pytest.mark.gpu

NETS = ['sr3_32x32x3', 'ac_odd_16x16x2', 'ac_dp_buckets_3']
# device tensor of the engine -> host table of the Structure
PAIRS = {'seg': 'seg_host', 'pack_desc': 'pack_desc_host', 'bn_table': 'bn_table_host', 'node_tab': 'node_tab_host',
         'kid_tab': 'kid_tab_host', 'node_ops': 'node_ops_host', 'node_ops_i64': 'node_ops_i64_host',
         'leaf_node_tab': 'leaf_node_tab_host', 'w_eq': 'w_eq_host'}


def _placed(net):
    return [(p.offset, getattr(p, 'node', None), getattr(p, 'is_router', None)) for p in net._all_params]


@pytest.mark.parametrize('case', NETS)
def test_device_tables_are_the_host_tables(case, monkeypatch):
    net, twin = make(case, monkeypatch), make(case, monkeypatch)
    eng, s = net.engine(), Structure(twin)
    for dev_name, host_name in PAIRS.items():
        dev, host = getattr(eng, dev_name), getattr(s, host_name)
        if host is None:
            assert dev is None, dev_name
            continue
        host = np.asarray(host, np.float32) if isinstance(host, list) else host
        got = dev.cpu().numpy()
        assert dev.is_cuda and got.dtype == host.dtype and np.array_equal(got, host), dev_name
    assert eng.curve_tree_dev.cpu().numpy().tobytes() == bytes(s.curve_tree) == bytes(eng.curve_tree)
    assert len(s.curve_tree) == len(eng.nodes) and C.sizeof(s.curve_tree) == eng.curve_tree_dev.numel()
    assert (eng.n_params, eng.n_state, eng.pack_size, eng.n_dsum, eng.n_seg, eng.n_pack, eng.n_bn) == \
        (s.n_params, s.n_state, s.pack_size, s.n_dsum, s.n_seg, s.n_pack, s.n_bn)
    assert (eng.dp_buckets, eng.seg_range, eng.dp_cut_block) == (s.dp_buckets, s.seg_range, s.dp_cut_block)
    assert eng.P.numel() == eng.A.numel() == eng.G.numel() == s.n_params and eng.S.numel() == max(s.n_state, 1)
    assert eng.packs.numel() == max(s.pack_size, 1) and eng.dsum.numel() == eng.dred.numel() == eng.dsum_last.numel() == s.n_dsum
    assert _placed(net) == _placed(twin)
    # the views of every parameter start at its offset
    for p in net._all_params:
        if p.trainable:
            for view, flat in ((p.data, eng.P), (p.grad, eng.G), (p.accum, eng.A)):
                assert view.numel() == p.size and view.data_ptr() == flat.data_ptr() + 4 * p.offset, (p.owner.name, p.name)
        else:
            assert p.data.numel() == p.size and p.data.data_ptr() == eng.S.data_ptr() + 4 * p.offset, (p.owner.name, p.name)
    assert eng.node_stat.data_ptr() == eng.G.data_ptr() and eng.node_stat.numel() == 2 * len(eng.nodes)


@pytest.mark.parametrize('case', NETS)
def test_structure_beside_a_live_engine_leaves_the_parameters_alone(case, monkeypatch):
    net = make(case, monkeypatch)
    eng = net.engine()
    before, ptrs = _placed(net), [p.data.data_ptr() for p in net._all_params]
    s = Structure(net)
    assert _placed(net) == before and [p.data.data_ptr() for p in net._all_params] == ptrs
    assert np.array_equal(eng.seg.cpu().numpy(), s.seg_host) and (eng.dp_buckets, eng.seg_range) == (s.dp_buckets, s.seg_range)
