"""The operation vocabulary of the stale-state fuzz (tests/test_engine_state_fuzz.py::test_long_lived_engine_lives_through_
predict_too) and its draw.  No device is touched and nothing here imports torch: tests/test_engine_ops_cpu.py checks on
the host what the committed (kind, seed) list covers.

An operation is a tuple (what, n, arg):

    ('train', n, reps)  ('steps', n, K)  ('eval', n, routed)  ('fwd_tr', n, None)      as the first fuzz draws them
    ('predict', n, dict(routed, probs, conf, decode))
    ('predict_all', N, dict(batch, source, decode, probs, conf, routed))

decode: None (float32 images), 'gamma', 'unit', 'table' (the case's own 256-entry float32 array) or 'table-rewritten' (the
SAME array object, rewritten in place since its last use).  source: 'u8' (host uint8 with a decode), 'f32' (host float32),
'dev' (a float32 tensor on the device).  conf = (form, value) is the exit_conf of the call, still without numbers: an
untrained head's confidences sit near 1 / n_cls, so the test takes every threshold as a QUANTILE of the confidences that an
ungated predict of a fresh net yields on the call's own images (both sides of every gate are then taken):

    ('none', None)  ('zero', 0.0)  ('above-one', 1.5)  ('scalar', q)
    ('per-leaf', [q or None per leaf])      None at some gateable leaves, a quantile at others
    ('same-set', [q or None per leaf])      the gated set of the previous gated call, every value another one: the captured
                                            program of that set replays with new thresholds
"""
import numpy as np

SHIPPED = ('ac', 'cr', 'sr', 'tree', 'dyn')                    # the 32x32x3 nets of the first fuzz (its _make builds them)
NEW = ('rect5', 'odd', 'lln', 'heads', 'wide24', 'tree4', 'dyn-odd')
KINDS = SHIPPED + NEW

#       kind:    (image shape, classes, blocks of the chain / depth of the table, family)
SPEC = {'ac': ((32, 32, 3), 10, 8, 'chain'), 'cr': ((32, 32, 3), 10, 8, 'chain'), 'sr': ((32, 32, 3), 10, 8, 'sr'),
        'tree': ((32, 32, 3), 10, 8, 'tree'), 'dyn': ((32, 32, 3), 10, 8, 'chain'),
        'rect5': ((24, 40, 3), 10, 4, 'chain'),            # general conv kernels, any-map entry points, 5x5 filters
        'odd': ((12, 20, 3), 10, 6, 'chain'),              # channel counts that are no multiples of 16, any-width exits
        'lln': ((24, 40, 3), 10, 3, 'chain'),              # MultiscaleLLN in front of block 0
        'heads': ((32, 32, 3), 10, 4, 'chain'),            # squared, superclass (2), squared-linear and plain exits
        'wide24': ((32, 32, 3), 24, 3, 'chain'),           # 24 classes: any-width exit kernels; squared and squared-linear
        'tree4': ((32, 32, 3), 10, 4, 'tree'),             # 15 blocks, seven three-sink switches
        'dyn-odd': ((16, 16, 2), 10, 6, 'chain')}          # per-sample k_cpt on the any-channel kernels
DYN = ('dyn', 'dyn-odd')
WALKED = ('ac', 'cr', 'rect5', 'odd', 'lln', 'wide24', 'heads')      # chains whose gate the host walk witnesses as well

PREDICT_N = (3, 37, 130, 200, 600)           # both sides of the initial capacity (128) and of routed_min_batch (512)
ALL_N = (0, 7, 300, 700)
ALL_BATCH = (7, 128, 256)
ROUTED = (False, True, 1, 2, 'auto')
DECODES = (None, 'gamma', 'unit', 'table', 'table-rewritten')
SOURCES = ('u8', 'f32', 'dev')
CONF_FORMS = ('none', 'scalar', 'per-leaf', 'zero', 'above-one', 'same-set')
QUANTILES = (0.2, 0.4, 0.6, 0.8)
INITIAL_CAPACITY = 128                       # Engine.__init__


def count_of(kind):
    """Operations per case: 8; 6 for the 15-block tree; 4 for the 47-block tree, whose every operation builds a fresh net
    of 47 blocks (with 6 operations at the sizes of the other kinds the case took 1.9 times as long as the first fuzz's ac-0
    case, against a limit of 1.5; at the small sizes of draw_ops 4 operations take 1.25 times as long, 5 take 1.47)."""
    return {'tree4': 6, 'tree': 4}.get(kind, 8)


def knobs_of(kind, A):
    """The module knobs of arch_and_hypers (read when a constructor is CALLED) under which the kind's nets are built:
    {name: value}, from the module's unpatched values."""
    if kind in SHIPPED:
        return {}
    blocks = SPEC[kind][2]
    if kind in ('odd', 'dyn-odd'):
        import os
        import sys
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
        if golden not in sys.path:                            # (once: tests/test_chan_nets.py imports it the same way)
            sys.path.insert(0, golden)
        from chan_ref_graph import ODD
        return {'arch': ODD}
    out = {'arch': A.arch[:blocks]}
    if kind == 'rect5':
        out['conv_supp'] = 5
    elif kind == 'lln':
        out['lln'] = {}
    elif kind == 'heads':
        from superclass_ref import hard_map
        out.update(exit_loss={0: 'squared', 2: 'squared-linear'}, coarse_exits={1: hard_map(10, 2)})
    elif kind == 'wide24':
        out['exit_loss'] = {0: 'squared', 1: 'squared-linear'}
    return out


def ctor_of(kind, A):
    """The net constructor of a NEW kind (called under knobs_of(kind))."""
    if kind == 'tree4':
        return A.ac_tree(k_cpt=1e-9)
    if kind == 'dyn-odd':
        return A.cr_chain(dyn_k_cpt=True)
    return A.ac_chain(k_cpt=1.6e-8)


def layout_of(kind):
    """(number of leaves, the gateable ones) in net.leaves order (depth first, a block's exit in front of its child blocks):
    a chain's exits but the last; a tree's exits under the forking blocks and under every block of a tail but the last."""
    _, _, blocks, family = SPEC[kind]
    if family == 'sr':
        return 1, ()
    if family == 'chain':
        return blocks, tuple(range(blocks - 1))
    leaves, gateable = [0], []

    def tail(i):
        if i < blocks - 1:
            gateable.append(leaves[0])
        leaves[0] += 1
        if i < blocks - 1:
            tail(i + 1)

    def fork(i):
        gateable.append(leaves[0])
        leaves[0] += 1
        for _ in range(2):
            tail(3) if i == 2 else fork(i + 1)
    fork(0)
    return leaves[0], tuple(gateable)


def images(shape, n, t, u8):
    """The images of operation t: bytes for a decoding call, floats in [0, 1) otherwise."""
    rng = np.random.default_rng(1000 + 17 * t)
    if u8:
        return rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
    return rng.random((n,) + tuple(shape)).astype(np.float32)


def labelled_batch(shape, n_cls, n, t):
    """As tests/test_net_parity.py::batch(n, seed=1000 + 17 * t), for any image shape and label width."""
    rng = np.random.default_rng(1000 + 17 * t)
    x0 = rng.random((n,) + tuple(shape)).astype(np.float32)
    y = np.eye(n_cls, dtype=np.float32)[rng.integers(0, n_cls, n)]
    return x0, y


def first_table():
    """The case's own decode table: one writable float32 array, handed to every 'table' call as the same object."""
    return np.ascontiguousarray((np.arange(256) / 255.0) ** 1.5, dtype=np.float32)


def rewrite_table(table, t):
    """In place, to values no earlier call of the case has seen."""
    table[:] = ((np.arange(256) / 255.0) ** (0.6 + 0.1 * t)).astype(np.float32)


def is_predict(op):
    return op[0] in ('predict', 'predict_all')


def gated_set(op, kind):
    """The leaves whose switches a predict / predict_all operation gates."""
    if not is_predict(op):
        return frozenset()
    form, value = op[2]['conf']
    gateable = layout_of(kind)[1]
    if form == 'none':
        return frozenset()
    if form in ('zero', 'above-one', 'scalar'):
        return frozenset(gateable)
    return frozenset(k for k in gateable if value[k] is not None)


def capacity_after(op, cap):
    """The engine's capacity after an operation (it only grows: Engine._ensure_capacity)."""
    n = min(op[2]['batch'], op[1]) if op[0] == 'predict_all' else op[1]
    return max(cap, n)


def _draw_conf(rng, kind, prev, just_gated):
    """prev: the conf of the previous GATED call of the sequence; just_gated: the operation right before was one."""
    n_leaves, gateable = layout_of(kind)
    if not gateable:
        return ('none', None)
    form = CONF_FORMS[int(rng.integers(0, len(CONF_FORMS)))]
    if just_gated and rng.random() < 0.4:
        form = 'same-set'
    if form == 'same-set' and prev is None:
        form = 'scalar'
    if form == 'none':
        return ('none', None)
    if form == 'zero':
        return ('zero', 0.0)
    if form == 'above-one':
        return ('above-one', 1.5)
    if form == 'scalar':
        return ('scalar', float(rng.choice(QUANTILES)))
    if form == 'per-leaf':
        gated = [k for k in gateable if rng.random() < 0.6]
        if len(gated) == len(gateable):                       # None at some gateable leaf ...
            gated.remove(gated[int(rng.integers(0, len(gated)))])
        if not gated:                                         # ... and a threshold at another
            gated = [gateable[int(rng.integers(0, len(gateable)))]]
        return ('per-leaf', [float(rng.choice(QUANTILES)) if k in gated else None for k in range(n_leaves)])
    old = prev[1] if prev[0] in ('per-leaf', 'same-set') else [prev[1] if k in gateable else None for k in range(n_leaves)]
    return ('same-set', [None if old[k] is None else float(rng.choice([q for q in QUANTILES if q != old[k]])) for k in range(n_leaves)])


def draw_ops(rng, kind, count):
    """`count` operations for a net of `kind`.  Two patterns come more often than chance would have it: a train -> predict
    pair is followed by a training step at the first one's batch size (the step that relies on the accumulators its
    predecessor left clean), and a predict_all of several chunks by another with the same batch, routed and probs under
    thresholds of its own (the hipGraph the first one captured for that shape must not serve another gated set; where the
    second call draws 'same-set', that graph is REPLAYED under thresholds other than those it was captured with)."""
    family = SPEC[kind][3]
    tree, shipped = family == 'tree', kind in SHIPPED
    big = kind == 'tree'                                       # 47 blocks: small batches only (the time of a case)
    train_n = [3, 16] if big else [3, 16, 37, 128] if tree else [3, 16, 37, 128, 128, 200]
    eval_n = [5, 64] if big else [5, 64, 200, 600, 1500] if shipped and not tree else [5, 64, 200, 600]
    predict_n, all_n = (PREDICT_N[:2], ALL_N[:2]) if big else (PREDICT_N, ALL_N)
    eval_routed = [False, True, 1, 2, 4, 'auto'] if shipped else list(ROUTED)
    routed_of = lambda: False if family == 'sr' else ROUTED[int(rng.integers(0, len(ROUTED)))]
    ops, prev_gated, table_used = [], None, False

    def decode_of(forms):
        nonlocal table_used
        d = forms[int(rng.integers(0, len(forms)))]
        if d == 'table-rewritten' and not table_used:
            d = 'table'                                        # (its first use)
        table_used = table_used or d == 'table'
        return d

    def conf_of():
        nonlocal prev_gated
        just = bool(ops) and bool(gated_set(ops[-1], kind))
        conf = _draw_conf(rng, kind, prev_gated, just)
        if conf[0] != 'none':
            prev_gated = conf
        return conf

    while len(ops) < count:
        if len(ops) >= 2 and is_predict(ops[-1]) and ops[-2][0] == 'train' and rng.random() < 0.6:
            ops.append(('train', ops[-2][1], int(rng.choice([1, 1, 3]))))
            continue
        if ops[-1:] and ops[-1][0] == 'predict_all' and ops[-1][1] >= 2 * ops[-1][2]['batch'] and rng.random() < 0.5:
            last = ops[-1][2]
            source = SOURCES[int(rng.integers(0, len(SOURCES)))]
            ops.append(('predict_all', int(rng.choice(all_n[1:])),
                        dict(batch=last['batch'], source=source, decode=decode_of(DECODES[1:]) if source == 'u8' else None,
                             probs=last['probs'], conf=conf_of(), routed=last['routed'])))
            continue
        u = rng.random()
        if u < 0.20:
            ops.append(('train', int(rng.choice(train_n)), int(rng.choice([1, 1, 3]))))
        elif u < 0.25 and not tree:
            ops.append(('steps', int(rng.choice([16, 128])), int(rng.choice([2, 3]))))
        elif u < 0.40:
            ops.append(('eval', int(rng.choice(eval_n)), False if family == 'sr' else eval_routed[int(rng.integers(0, len(eval_routed)))]))
        elif u < 0.45:
            ops.append(('fwd_tr', int(rng.choice([16, 40])), None))
        elif u < 0.80:
            n = int(rng.choice(predict_n))
            ops.append(('predict', n, dict(routed=routed_of(), probs=bool(rng.integers(0, 2)), conf=conf_of(), decode=decode_of(DECODES))))
        else:
            N, batch = int(rng.choice(all_n)), int(rng.choice(ALL_BATCH))
            source = SOURCES[int(rng.integers(0, len(SOURCES)))]
            ops.append(('predict_all', N, dict(batch=batch, source=source, decode=decode_of(DECODES[1:]) if source == 'u8' else None,
                                               probs=bool(rng.integers(0, 2)), conf=conf_of(), routed=routed_of())))
    return ops


# (kind, seed) of the committed cases: two seeds per new kind, one more for each kind of the first fuzz.  Picked on the host
# so that together they cover what tests/test_engine_ops_cpu.py lists; if a seed has to change, change it here, not the list.
CASES = [('rect5', 26), ('rect5', 62), ('odd', 94), ('odd', 107), ('lln', 38), ('lln', 73), ('heads', 32), ('heads', 21),
         ('wide24', 25), ('wide24', 44), ('tree4', 144), ('tree4', 15), ('dyn-odd', 151), ('dyn-odd', 34),
         ('ac', 64), ('cr', 30), ('sr', 67), ('tree', 135), ('dyn', 58)]


def cases_from_env(text):
    """MPNN_STATE_FUZZ_SEEDS="100 140" -> seeds 100 .. 139, the kinds in turn (as the first fuzz reads it)."""
    lo, hi = (int(v) for v in text.split())
    return [(KINDS[s % len(KINDS)], s) for s in range(lo, hi)]


def ops_of(kind, seed):
    return draw_ops(np.random.default_rng(seed), kind, count_of(kind))
