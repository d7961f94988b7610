"""CPU: what the planner decides about the backward pass of a training step before it builds a launch record
(lib/_eng_planner.py: Planner._bwd_plan) -- launch groups with their workgroup budgets, weight-gradient splits, the slab
layout with its item and optimizer tables, which dgrad-horz writes a shared parent map and which add to it, the place of the
data-parallel 'mid' bucket marker.  The plan is host arithmetic over a Structure and the planner settings; of the device it
needs only the resident-slot counts of mpnn_msconv_bwd_level_slots and mpnn_msconv_bwd_scale_slots.

* The plan of every case of PLANS equals tests/golden/bwd_plan_golden.json, field by field and digest by digest.  The file was
  recorded on an MI355X from commit d8a122d -- the last one whose Planner._bwd_launches made these decisions while it filled
  the launch records -- by a throw-away script: a copy of that commit with lines added to _bwd_launches that kept the groups,
  every WgradArgs / DgradHorzArgs record under its (block, scale), the slab tensor, the two table row lists, the index of the
  group in front of the 'mid' marker and whether a slab reduction went with it.  Per case the script made net.engine(), set
  the settings of the case on it (for the data-parallel cases a stand-in callable as allreduce), put a recorder of this
  module's Replay shape in place of eng.lib -- it noted every call of the two *_slots entry points with its answer and the
  compute-unit reservation in force -- ran eng.program('tr', n), turned the records' pointers into offsets from the slab base
  (or 'G': the parameter's own gradient) and called record() of this module.  For sr_chain(3) at n = 16 the file holds the
  two tables in full, for the other cases their SHA-1.
* Here the plan is made by a Host(Structure, Planner) whose lib is a Replay: it answers the two *_slots calls from the file
  -- a query that was not recorded fails, and the set of distinct queries must be the recorded one -- and passes every other
  call to the real library.  While a plan is made the planner module's `torch` is None.
* The two 'does not fit the resident slots' refusals of _bwd_schedule, reached with libs that answer too few slots."""
import hashlib
import json
import os

import numpy as np
import pytest

from lib import _eng_planner, _hip
from lib._eng_planner import Planner
from lib._eng_structure import Structure
from test_engine_structure_cpu import CASES, make

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bwd_plan_golden.json')
FULL = 'sr3_n16'                                      # the case whose tables the file holds in full
SETTINGS = dict(multi_stream=False, bwd_levels=True, fuse_opt=True, co_share=1)     # (as Engine.__init__ leaves them)
AC_DP = lambda buckets: dict(CASES['ac_32x32x3'], env={'MPNN_DP_BUCKETS': str(buckets)})
# name -> case (of test_engine_structure_cpu.CASES, or its dict), batch, dp, reserve (compute units left to the collective
# of a bucketed data-parallel step), planner settings other than SETTINGS
PLANS = {
    'ac_n16': dict(case='ac_32x32x3', n=16),
    'ac_n128': dict(case='ac_32x32x3', n=128),
    'ac_n1024': dict(case='ac_32x32x3', n=1024),
    'sr3_n16': dict(case='sr3_32x32x3', n=16),
    'ac_24x40x3': dict(case='ac_24x40x3', n=128),
    'ac_tree': dict(case='ac_tree', n=128),
    'cr_tree': dict(case='cr_tree', n=128),
    'ac_co_share_8': dict(case='ac_32x32x3', n=128, co_share=8),
    'ac_dp_buckets_1': dict(case=AC_DP(1), n=128, dp=True),
    'ac_dp_buckets_3': dict(case=AC_DP(3), n=128, dp=True),
    'ac_dp_buckets_3_reserve_16': dict(case=AC_DP(3), n=128, dp=True, reserve=16),
    'ac_multi_stream': dict(case='ac_32x32x3', n=128, multi_stream=True),
    'ac_no_levels': dict(case='ac_32x32x3', n=128, bwd_levels=False),
    'ac_no_fused_opt': dict(case='ac_32x32x3', n=128, fuse_opt=False),
    'sr3_generic_convs': dict(case='sr3_generic_convs', n=16),
    'sr3_anymap_convs': dict(case='sr3_anymap_convs', n=16),
    'sr3_anychan_convs': dict(case='sr3_anychan_convs', n=16),
    'ac_supp_5': dict(case='ac_supp_5', n=128),
    'ac_odd_16x16x2': dict(case='ac_odd_16x16x2', n=128),
    'sr_narrow_8x8x5': dict(case='sr_narrow_8x8x5', n=16),
}


class Host(Structure, Planner):
    """A Structure with the planner settings: everything _bwd_plan reads."""
    def __init__(self, net, lib, **settings):
        Structure.__init__(self, net)
        self.real_lib, self.lib = self.lib, lib(self.lib)
        self.__dict__.update(SETTINGS)
        self.__dict__.update(settings)


class Replay:
    """The kernel library with the two *_slots entry points answered from recorded queries [[name, args, reserve, answer],
    ...] under the reservation `reserve`; `asked`: the distinct queries so far."""
    def __init__(self, lib, queries, reserve):
        self._lib, self._reserve, self.asked = lib, reserve, set()
        self.answers = {(name, tuple(args), res): ans for name, args, res, ans in queries}

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def _answer(self, name, args):
        key = (name, tuple(int(a) for a in args), self._reserve)
        assert key in self.answers, 'a slot query that was not recorded: %r' % (key,)
        self.asked.add(key)
        return self.answers[key]

    def mpnn_msconv_bwd_level_slots(self, H, W, Co, k):
        return self._answer('level', list(H[:k]) + list(W[:k]) + list(Co[:k]))

    def mpnn_msconv_bwd_scale_slots(self, *args):
        return self._answer('scale', args)


def settings_of(spec):
    return {k: v for k, v in spec.items() if k in SETTINGS}


def record(plan, full=False):
    """What the golden file holds of a plan, as JSON gives it back: slab pointers as offsets in the slab buffer, 'G' for a
    gradient that goes straight into G, None for the dwv of a scale without a vert conv."""
    sha = lambda a: hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert plan['items'].dtype == plan['item_seg'].dtype == np.int32
    assert plan['items'].shape[1:] == (6,) and plan['item_seg'].shape == (len(plan['items']), _hip.SEG_INTS)
    dst = lambda t, i, f: None if (f == 'dwv' and i == 0) else 'G' if t['slab'] is None else t['slab'][f]
    rec = dict(groups=plan['groups'], launches=plan['launches'],
               triples=[[kb, i, t['split'], t['split_stride'], dst(t, i, 'dwa'), dst(t, i, 'dwv'), dst(t, i, 'db'),
                         t['accumulate'], t['dy_extra']] for (kb, i), t in plan['triples'].items()],
               slab_size=plan['slab_size'], n_cut=plan['n_cut'], mid_after=plan['mid_after'], mid_reduce=plan['mid_reduce'],
               fused_opt=plan['fused_opt'], slab_params=list(plan['slab_params']),
               sha1=dict(items=sha(plan['items']), item_seg=sha(plan['item_seg'])))
    if full:
        rec['tables'] = dict(items=plan['items'].tolist(), item_seg=plan['item_seg'].tolist())
    return json.loads(json.dumps(rec, default=int))


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(PLANS) and 'tables' in golden[FULL]['plan']
    for name, spec in PLANS.items():
        assert golden[name]['settings'] == dict(SETTINGS, **settings_of(spec)), name
        assert (golden[name]['n'], golden[name]['dp'], golden[name]['reserve']) == \
            (spec['n'], spec.get('dp', False), spec.get('reserve', 0)), name


@pytest.mark.parametrize('name', list(PLANS))
def test_plan_equals_the_recorded_one(name, golden, monkeypatch):
    spec, want = PLANS[name], golden[name]
    host = Host(make(spec['case'], monkeypatch), lambda lib: Replay(lib, want['queries'], spec.get('reserve', 0)),
                **settings_of(spec))
    for flag in ('generic_convs', 'anymap_convs', 'anychan_convs', 'dp_cut_block'):
        assert getattr(host, flag) == want['structure'][flag], flag
    monkeypatch.setattr(_eng_planner, 'torch', None)
    got = record(host._bwd_plan(spec['n'], spec.get('dp', False)), full=name == FULL)
    assert sorted(got) == sorted(want['plan'])
    for field in want['plan']:
        if field in ('sha1', 'tables'):
            for tab in ('items', 'item_seg'):
                assert got[field][tab] == want['plan'][field][tab], (field, tab)
        else:
            assert got[field] == want['plan'][field], field
    assert host.lib.asked == set(host.lib.answers)


def test_the_cases_reach_what_they_are_there_for(golden):
    """Level launches, siblings that add to one parent map, gradients written straight into G, a 'mid' marker with and
    without a slab reduction's prefix, the per-triple and the per-kind schedules."""
    plan = lambda name: golden[name]['plan']
    assert any(len(g) > 1 for g in plan('ac_n128')['groups']) and all(len(g) == 1 for g in plan('ac_no_levels')['groups'])
    assert all(bud is None for g in plan('ac_no_levels')['groups'] for _, _, bud in g)
    assert all(bud is not None for g in plan('ac_co_share_8')['groups'] for _, _, bud in g)
    for tree in ('ac_tree', 'cr_tree'):
        assert {t[7] for t in plan(tree)['triples']} == {None, 0, 1}
    assert {t[7] for t in plan('ac_n128')['triples']} == {None, 0}
    assert plan('ac_dp_buckets_3')['mid_after'] is not None and plan('ac_dp_buckets_3')['mid_reduce'] and \
        plan('ac_dp_buckets_3')['n_cut'] > 0
    assert plan('ac_dp_buckets_1')['mid_after'] is None and plan('ac_dp_buckets_1')['n_cut'] == 0
    assert not any(plan(name)['fused_opt'] for name in ('ac_dp_buckets_1', 'ac_no_fused_opt', 'ac_multi_stream'))
    assert plan('ac_n128')['fused_opt']
    assert plan('ac_multi_stream')['groups'] is None and plan('ac_n128')['launches'] is None
    assert {k for k, _, _ in plan('ac_multi_stream')['launches']} == {'vert', 'horz', 'wgrad'}
    assert golden['ac_dp_buckets_3_reserve_16']['queries'] and all(q[2] == 16 for q in golden['ac_dp_buckets_3_reserve_16']['queries'])


# ------------------------------------------------------------------ refusals
class Slots:
    """The kernel library with both *_slots entry points answered by slots(members of the queried launch)."""
    def __init__(self, lib, slots):
        self._lib, self._slots = lib, slots

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def mpnn_msconv_bwd_level_slots(self, H, W, Co, k):
        return self._slots(k)

    def mpnn_msconv_bwd_scale_slots(self, *args):
        return self._slots(1)


def test_co_trained_launch_of_one_triple_that_does_not_fit_is_refused(monkeypatch):
    host = Host(make('ac_32x32x3', monkeypatch), lambda lib: Slots(lib, lambda k: 1), co_share=8)
    with pytest.raises(NotImplementedError, match='co-training 8 nets: a backward launch does not fit the resident slots'):
        host._bwd_plan(128, False)


def test_co_trained_level_whose_members_do_not_fit_one_by_one_is_refused(monkeypatch):
    """Plenty of slots until the first launch of two triples is asked for, one slot from then on: the level falls back to a
    launch per member, and those do not fit either."""
    seen = []

    def slots(k):
        seen.append(k)
        return 1 if 2 in seen else 1 << 16
    host = Host(make('ac_32x32x3', monkeypatch), lambda lib: Slots(lib, slots), co_share=8)
    with pytest.raises(NotImplementedError, match='co-training 8 nets: a backward launch does not fit the resident slots'):
        host._bwd_plan(128, False)
    assert seen.index(2) > 0 and seen[seen.index(2):] == [2, 1, 1]
