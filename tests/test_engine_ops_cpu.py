"""CPU: what the committed cases of the stale-state fuzz draw (tests/engine_ops.py; the GPU side is
tests/test_engine_state_fuzz.py).  Every operation kind, argument form and transition the fuzz exists for occurs in the
committed (kind, seed) list; the kinds' leaf layouts are those of the nets; the first fuzz still draws what it drew."""
import json
import os

import numpy as np
import pytest

import engine_ops as E

HERE = os.path.dirname(os.path.abspath(__file__))


def seen(cases):
    """The set of everything the cases' sequences contain: ('op', what), ('decode', form), ('conf', form),
    ('source', s), ('routed', r) and the names of the transitions."""
    out = set()
    for kind, seed in cases:
        ops = E.ops_of(kind, seed)
        cap, last_table_use, last_predict, shapes, gated_shapes, rows = E.INITIAL_CAPACITY, None, None, {}, {}, None
        for t, op in enumerate(ops):
            what, n, arg = op
            out.add(('op', what))
            prev = ops[t - 1] if t else None
            if not E.is_predict(op) and n > cap:
                shapes, gated_shapes = {}, {}
            if E.is_predict(op) and n > 0:
                # the launches of the call: (images, probs, routed) -> the gated sets of the calls so far; a reallocation
                # drops the graphs, the third call of a shape replays what the second captured
                chunks = [n] if what == 'predict' else [arg['batch']] * (n // arg['batch']) + [n % arg['batch']] * bool(n % arg['batch'])
                reached = cap
                for m in chunks:
                    if m > reached:
                        shapes, gated_shapes, reached = {}, {}, m
                    calls_key = (m, arg['probs'], False if arg['routed'] == 'auto' and m < 512 else arg['routed'])
                    calls = shapes.setdefault(calls_key, [])
                    if len(calls) >= 2 and calls[1] != E.gated_set(op, kind):
                        out.add('a captured predict shape under another gated set')
                    calls.append(E.gated_set(op, kind))
                    # the graphs as the engine keys them, the gated set included: the thresholds of each launch of a key (a
                    # quantile becomes another number on another call's images: the call stands for its values)
                    if E.gated_set(op, kind):
                        values = arg['conf'][1] if arg['conf'][0] in ('zero', 'above-one') else ('call', t)
                        taus = gated_shapes.setdefault(calls_key + (E.gated_set(op, kind),), [])
                        if len(taus) >= 2 and taus[1] != values:
                            out.add('a captured gated shape replayed under other thresholds')
                        taus.append(values)
            if E.is_predict(op):
                out.update({('decode', arg['decode']), ('conf', arg['conf'][0]), ('routed', arg['routed'])})
                gate = E.gated_set(op, kind)
                if what == 'predict_all':
                    out.add(('source', arg['source']))
                    out.add('predict_all without an image' if n == 0 else
                            ('chunks', 'one' if n <= arg['batch'] else 'many', 'ragged' if n % arg['batch'] else 'even'))
                    if min(arg['batch'], n) > cap:
                        out.add('predict_all beyond the capacity')
                if what == 'predict' and n >= 512 and arg['routed'] == 'auto':
                    out.add('predict auto at 512 or more')
                if what == 'predict' and not gate and prev is not None and prev[0] == 'predict' and E.gated_set(prev, kind):
                    out.add('gated predict -> ungated predict')
                if arg['conf'][0] == 'same-set':
                    # (the previous GATED call may lie further back; the replay with new values needs it right before)
                    if n > 0 and prev is not None and E.is_predict(prev) and prev[1] > 0 and E.gated_set(prev, kind) == gate \
                            and _values(prev) != _values(op):
                        out.add('same gated set twice in a row')
                    if n > 0 and last_predict is not None and E.gated_set(last_predict, kind) == gate:
                        out.add('same gated set as the previous predict call')
                if arg['decode'] == 'table-rewritten':
                    assert last_table_use is not None
                    out.add('table rewritten after its first use')
                    if last_table_use == 'direct':
                        out.add('table rewritten with no other table in between')
                if arg['decode'] is not None:
                    last_table_use = 'direct' if arg['decode'] in ('table', 'table-rewritten') else \
                        (None if last_table_use is None else 'other')
                if n > 0:                                  # (no image: no call of the engine)
                    last_predict = op
            if what == 'eval' and prev is not None and prev[0] == 'predict' and E.gated_set(prev, kind):
                out.add('gated predict -> eval')
            if what == 'train' and prev is not None and E.is_predict(prev):
                out.add('predict -> train')
                if t >= 2 and ops[t - 2][0] == 'train' and ops[t - 2][1] == n:
                    out.add('train -> predict -> train at one batch size')
            # the per-leaf softmax rows: allocated by the first call with probs, dropped by a reallocation, zero where an exit
            # with a label space of its own (the superclass head) writes nothing
            if rows == 'made' and E.capacity_after(op, cap) > cap:
                rows = 'dropped'
            if E.is_predict(op) and n > 0 and arg['probs']:
                if rows == 'dropped' and kind == 'heads':
                    out.add('softmax rows made again after a reallocation, under a narrower head')
                rows = 'made'
            cap = E.capacity_after(op, cap)
    return out


def _values(op):
    return op[2]['conf'][1]


WANTED = [('op', w) for w in ('train', 'steps', 'eval', 'fwd_tr', 'predict', 'predict_all')] + \
         [('decode', d) for d in E.DECODES] + [('conf', f) for f in E.CONF_FORMS] + [('source', s) for s in E.SOURCES] + \
         [('routed', r) for r in E.ROUTED] + \
         [('chunks', 'one', 'ragged'), ('chunks', 'many', 'ragged'), 'predict_all without an image'] + \
         ['gated predict -> eval', 'gated predict -> ungated predict', 'same gated set twice in a row',
          'same gated set as the previous predict call', 'predict -> train', 'train -> predict -> train at one batch size',
          'predict_all beyond the capacity', 'predict auto at 512 or more', 'table rewritten after its first use',
          'table rewritten with no other table in between', 'a captured predict shape under another gated set',
          'a captured gated shape replayed under other thresholds',
          'softmax rows made again after a reallocation, under a narrower head']


def test_committed_cases_cover_the_vocabulary():
    got = seen(E.CASES)
    missing = [w for w in WANTED if w not in got]
    assert not missing, missing


def test_committed_case_list():
    kinds = [k for k, _ in E.CASES]
    assert len(set(E.CASES)) == len(E.CASES)
    for kind in E.NEW:
        assert kinds.count(kind) == 2, kind
    for kind in E.SHIPPED:
        assert kinds.count(kind) == 1, kind
    assert E.cases_from_env('24 36') == [(E.KINDS[s % 12], s) for s in range(24, 36)] and len(E.KINDS) == 12


@pytest.mark.parametrize('kind', E.KINDS)
def test_draws_obey_the_rules_of_the_kind(kind):
    n_leaves, gateable = E.layout_of(kind)
    tree = E.SPEC[kind][3] == 'tree'
    for seed in range(40):
        ops = E.ops_of(kind, seed)
        assert len(ops) == {'tree4': 6, 'tree': 4}.get(kind, 8) and ops == E.ops_of(kind, seed)
        for what, n, arg in ops:
            if kind == 'tree':
                assert n <= 64
            if what == 'train':
                assert n in ((3, 16, 37, 128) if tree else (3, 16, 37, 128, 200))
            elif what == 'steps':
                assert not tree
            elif what == 'eval':
                assert n in ((5, 64, 200, 600, 1500) if kind in E.SHIPPED and not tree else (5, 64, 200, 600))
                assert arg is False or kind != 'sr'
            elif what == 'predict':
                assert n in E.PREDICT_N
            elif what == 'predict_all':
                assert n in E.ALL_N and arg['batch'] in E.ALL_BATCH and (arg['decode'] is not None) == (arg['source'] == 'u8')
            if what in ('predict', 'predict_all'):
                form, value = arg['conf']
                if kind == 'sr':
                    assert form == 'none' and arg['routed'] is False
                if form in ('per-leaf', 'same-set'):
                    assert len(value) == n_leaves and all(v is None for k, v in enumerate(value) if k not in gateable)
                    assert any(value[k] is not None for k in gateable)
                if form == 'per-leaf':
                    assert any(value[k] is None for k in gateable)


@pytest.mark.parametrize('kind', E.KINDS)
def test_leaf_layouts_are_those_of_the_nets(kind, monkeypatch):
    """Building a net needs no device (the engine comes with the first run)."""
    import arch_and_hypers as A
    for name, value in E.knobs_of(kind, A).items():
        monkeypatch.setattr(A, name, value)
    shape, n_cls, blocks, family = E.SPEC[kind]
    if kind in E.NEW:
        ctor = E.ctor_of(kind, A)
    else:
        ctor = {'ac': A.ac_chain(k_cpt=1.6e-8), 'cr': A.cr_chain(k_cpt=4e-9, optimistic=True), 'sr': A.sr_chain(5),
                'tree': A.ac_tree(k_cpt=1e-9), 'dyn': A.cr_chain(dyn_k_cpt=True)}[kind]
    net = ctor(shape, (n_cls,))
    n_leaves, gateable = E.layout_of(kind)
    assert len(list(net.leaves)) == n_leaves and tuple(net.gateable_leaves) == gateable
    assert bool(getattr(net.hypers, 'dyn_k_cpt', False)) == (kind in E.DYN)
    if kind == 'tree4':
        assert sum(1 for ℓ in net.layers if ℓ.router is not None and len(ℓ.sinks) == 3) == 7


def test_the_first_fuzz_draws_what_it_drew():
    """The ten sequences of test_long_lived_engine_equals_fresh_engines, against the copy recorded before the vocabulary
    grew (tests/golden/engine_state_fuzz_draws.json)."""
    import test_engine_state_fuzz as F
    with open(os.path.join(HERE, 'golden', 'engine_state_fuzz_draws.json')) as f:
        recorded = json.load(f)
    if not os.environ.get('MPNN_STATE_FUZZ_SEEDS'):
        assert [(c['kind'], c['seed']) for c in recorded] == F._CASES
    assert len(recorded) == 10
    for c in recorded:
        ops = F._draw_ops(np.random.default_rng(c['seed']), c['kind'], 9 if c['kind'] != 'tree' else 6)
        assert [list(op) for op in ops] == c['ops'], (c['kind'], c['seed'])
