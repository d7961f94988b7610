"""GPU: the backward launch records of a training program are its plan (lib/_eng_planner.py: Planner._bwd_plan, kept under
'bwd_plan' in the program; its values: tests/test_bwd_plan_cpu.py).  No kernel runs.  For three nets -- sr_chain(3) on 32x32x3,
the actor tree, the shipped actor chain under MPNN_DP_BUCKETS=3 with a stand-in for the collective -- at 16 samples: every
WgradArgs has the planned n_split and split_stride, and its dwa / dwv / db point 4 x the planned offset behind the slab base or
at the parameter's own gradient; every DgradHorzArgs has the planned accumulate, and the parent's exit dX as dy_extra where
planned; the device item table and item_seg, copied back, equal the plan's; the 'mid' bucket marker follows the planned group.
The slab base is read from the FinishNet record or the first argument of the finishing launch."""
import numpy as np
import pytest
import torch

from lib import _hip
from test_engine_structure_cpu import make

pytestmark = pytest.mark.gpu

N = 16
NETS = ['sr3_32x32x3', 'ac_tree', 'ac_dp_buckets_3']


def _read(eng, ptr, count):
    """`count` int32 at device address `ptr`, through the tensor of the engine that holds them."""
    for t in eng._keep:
        if isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.data_ptr() <= ptr and ptr + 4 * count <= t.data_ptr() + 4 * t.numel():
            first = (ptr - t.data_ptr()) // 4
            return t.cpu().numpy()[first:first + count]
    raise AssertionError('no table of the engine at %#x' % ptr)


def _members(op):
    """(horz, vert, wgrad) records of a backward conv launch, None where it has none: the BwdMember table of a level launch,
    the three byref arguments of mpnn_msconv_bwd_scale."""
    if op.host is not None:
        return [tuple(p.contents if p else None for p in (m.horz, m.vert, m.wgrad)) for m in op.host]
    return [tuple(a._obj if a is not None else None for a in op.args[:3])]


@pytest.mark.parametrize('case', NETS)
def test_records_are_the_plan(case, monkeypatch):
    net = make(case, monkeypatch)
    eng = net.engine()
    rev = list(reversed(eng.blocks))
    if case == 'ac_dp_buckets_3':
        eng.allreduce = lambda view: view
    prog = eng.program('tr', N)
    plan, ops = prog['bwd_plan'], prog['bwd']
    convs = [k for k, op in enumerate(ops) if op.what == 'bwd_scale']
    # the records in launch order are the triples in group order
    walk = [(kb, i) for grp in plan['groups'] for kb, i, _ in grp]
    recs = [m for k in convs for m in _members(ops[k])]
    assert list(plan['triples']) == walk and len(recs) == len(walk)
    assert [len(_members(ops[k])) for k in convs] == [len(grp) for grp in plan['groups']]
    fin = ops[-2] if ops[-1].what == 'bucket' else ops[-1]
    assert fin.what == 'backward_finish'
    fused = isinstance(fin.host, _hip.FinishNet)
    slab = fin.host.slabs if fused else fin.args[0]
    n_slab = 0
    for (kb, i), (h, v, w) in zip(walk, recs):
        b, t, cp = rev[kb], plan['triples'][(kb, i)], rev[kb].conv.params
        assert (w.n, w.H, w.W, w.Cout) == (N, b.H[i], b.W[i], b.C[i]) and w.g == b.dzg[i].data_ptr(), (kb, i)
        assert (w.n_split, w.split_stride) == (t['split'], t['split_stride']), (kb, i)
        prms = dict(dwa=getattr(cp, 'w_horz_%i' % i), dwv=getattr(cp, 'w_vert_%i' % (i - 1)) if i > 0 else None, db=getattr(cp, 'b_%i' % i))
        for f, prm in prms.items():
            if prm is None:
                assert getattr(w, f) is None and (t['slab'] is None or f not in t['slab'])
            elif t['slab'] is None:
                assert t['split'] == 1 and getattr(w, f) == prm.grad.data_ptr(), (kb, i, f)
            else:
                assert t['split'] > 1 and getattr(w, f) == slab + 4 * t['slab'][f], (kb, i, f)
                assert t['slab'][f] + (t['split'] - 1) * t['split_stride'] + prm.size <= plan['slab_size']
                assert prm.offset in plan['slab_params']
                n_slab += 1
        if b.parent is None:
            assert h is None and t['accumulate'] is None and t['dy_extra'] is None
        else:
            assert h.out == b.parent.dzg[b.in_map[i]].data_ptr() and h.accumulate == t['accumulate'], (kb, i)
            assert h.dy_extra == (b.parent.dx.data_ptr() if t['dy_extra'] else None), (kb, i)
    assert n_slab == len(plan['slab_params']) > 0
    if case == 'ac_tree':
        assert {t['accumulate'] for t in plan['triples'].values()} == {None, 0, 1}
    # the device tables
    n_items, n_cut = len(plan['items']), plan['n_cut']
    assert fused == plan['fused_opt'] == prog['fused_opt'] == (case != 'ac_dp_buckets_3')
    if fused:
        assert fin.host.n_items == n_items and n_cut == 0
        assert np.array_equal(_read(eng, fin.host.slab_table, 6 * n_items), plan['items'].reshape(-1))
        assert np.array_equal(_read(eng, fin.host.item_seg, _hip.SEG_INTS * n_items), plan['item_seg'].reshape(-1))
    else:
        assert fin.args[3] == n_items - n_cut
        assert np.array_equal(_read(eng, fin.args[2], 6 * (n_items - n_cut)), plan['items'][n_cut:].reshape(-1))
    # the 'mid' marker: behind the launch of the planned group, the reduction of the cut blocks' items in front of it
    marks = [k for k, op in enumerate(ops) if op.what == 'bucket' and op.tag == 'mid']
    if case != 'ac_dp_buckets_3':
        assert plan['mid_after'] is None and not plan['mid_reduce'] and not marks
    else:
        assert len(marks) == 1 and [k for k in convs if k < marks[0]] == convs[:plan['mid_after'] + 1]
        red = ops[marks[0] - 1]
        assert plan['mid_reduce'] and red.what == 'slab_reduce' and red.args[0] == slab and red.args[3] == n_cut > 0
        assert np.array_equal(_read(eng, red.args[2], 6 * n_cut), plan['items'][:n_cut].reshape(-1))
        assert marks[0] - 2 == convs[plan['mid_after']]
