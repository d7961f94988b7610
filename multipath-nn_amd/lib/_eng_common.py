"""What the pieces of the engine (lib/_plan.py and its _eng_* modules) share: the kernel library binding, the chain shapes
the planner accepts, attribute lookup through Python's identifier normalisation, the small record classes and the launch
type of the programs."""
import copy
import ctypes as C
import os
import unicodedata

import numpy as np
import torch

from lib import _hip
from lib._hip import check
from lib.layer_types import Chain
from lib.net_types import n_leaves, params_list_rec

ROUTER_COMPS = ['Select', 'LinTrans', 'BatchNorm', 'Rect', 'LinTrans', 'BatchNorm', 'Rect', 'LinTrans']
BLOCK_COMPS = ['MultiscaleConvMax', 'MultiscaleBatchNorm', 'MultiscaleRect']
HEAD_COMPS = ['Select', 'LinTrans', 'Softmax', 'CrossEntropyError']
HEAD_COMPS_SUPER = HEAD_COMPS[:3] + ['SuperclassCrossEntropyError']      # (a head with a label space of its own)
# ... and with SquaredError, on the softmax or on the LinTrans output itself (layer_types.py: SquaredError)
HEAD_COMPS_SQ = HEAD_COMPS[:3] + ['SquaredError']
HEAD_COMPS_SQ_LIN = HEAD_COMPS[:2] + ['SquaredError']
# ... and any of the four with ActivityError layers (layer_types.py) behind Select, behind the LinTrans or behind the Softmax
ACTIVITY_WHERE = ('map', 'logits', 'probs')
ACTIVITY_POSITIONS = ("ActivityError runs in a LogReg chain only, behind Select ('map': the block's coarsest activation map), behind the "
                      "LinTrans ('logits') or behind the Softmax ('probs'): Select, [ActivityError], LinTrans, [ActivityError], "
                      "[Softmax, [ActivityError]], error layer")
# ... and any of those with ONE Dropout layer (layer_types.py) directly in front of the LinTrans -- not beside a 'map' ActivityError
DROPOUT_POSITION = ("Dropout runs in a LogReg chain only, once, directly in front of the head's LinTrans and without a 'map' ActivityError "
                    "beside it: Select, [Dropout], LinTrans, [ActivityError], [Softmax, [ActivityError]], error layer")
OPT_CHUNK = 2048
# hipGraph capture mode: thread-local, so that other threads' runtime calls (the process group's
# watchdog polling its events under data parallelism) are not errors while this thread captures
CAPTURE_MODE = 'thread_local'


def _nf(name):
    """Python NFKC-normalises identifiers (the keyword ``ϵ=`` U+03F5 is stored as U+03B5) but not
    string literals: every string-keyed attribute lookup must go through the same normalisation."""
    return unicodedata.normalize('NFKC', name)


def _attr(obj, name, default=None):
    return getattr(obj, _nf(name), default)


def _head_split(comps):
    """(the components without their ActivityError layers, [α 'map', α 'logits', α 'probs']) of a chain whose ActivityError
    layers all stand at one of the three positions of a head -- several at one position add their α, as Chain sums their
    costs -- or None."""
    rest, α, where = [], [0.0, 0.0, 0.0], -1
    for c in comps:
        name = type(c).__name__
        if name == 'Dropout':                      # (its position is _kind's to judge: refuse_dropout)
            continue
        if name == 'ActivityError':
            if where < 0:
                return None
            α[where] += float(c.hypers.α)
            continue
        where = {(0, 'Select'): 0, (1, 'LinTrans'): 1, (2, 'Softmax'): 2}.get((len(rest), name), -1)
        rest.append(c)
    return rest, α


def refuse_activity(comps, what):
    """ActivityError anywhere in `comps` (a router's or a block's chain, a Conv net's stages): the refusal that names the
    positions it does run at."""
    if any(type(c).__name__ == 'ActivityError' for c in comps):
        raise NotImplementedError('%s: %s' % (what, ACTIVITY_POSITIONS))


def refuse_dropout(comps, what, head=False):
    """Dropout anywhere in `comps` but at its one position: the refusal that names it.  head: `comps` are a LogReg chain's,
    where Select, Dropout, LinTrans at its start (and no second Dropout) is that position; a router's or a block's chain
    and a Conv net's stages have none."""
    t = [type(c).__name__ for c in comps]
    if 'Dropout' in t and not (head and t[:3] == ['Select', 'Dropout', 'LinTrans'] and t.count('Dropout') == 1):
        raise NotImplementedError('%s: %s' % (what, DROPOUT_POSITION))


def head_dropout(chain):
    """The Dropout layer of a head chain that the training program has to run -- None without one, and None with λ == 1,
    which keeps every element unscaled: such a layer is planned away."""
    for c in chain.comps:
        if type(c).__name__ == 'Dropout':
            return c if float(c.hypers.λ) < 1.0 else None
    return None


def dropout_thresh(λ):
    """thresh of an mpnn_dropout_args record: a 32-bit Philox word r keeps its element iff r >= thresh, i.e. iff
    u = r / 2^32 >= 1 - λ -- ceil((1 - λ) 2^32) in float64, as a uint32 (a λ so small that the product rounds to 2^32: the
    largest word still keeps)."""
    import math
    return min(int(math.ceil((1.0 - float(λ)) * 4294967296.0)), 0xFFFFFFFF)


DROPOUT_RANK_STRIDE = 0x9E3779B97F4A7C15


def dropout_seed(seed, rank=0):
    """The 64-bit Philox key of a Dropout layer on data-parallel rank `rank`: every rank draws its own masks."""
    return (int(seed) + int(rank) * DROPOUT_RANK_STRIDE) % (1 << 64)


def _kind(ℓ):
    if isinstance(ℓ, Chain):
        t = [type(c).__name__ for c in ℓ.comps]
        if 'Dropout' in t:
            refuse_dropout(ℓ.comps, 'layer %r' % (ℓ.name,), head=True)
            t = [name for name in t if name != 'Dropout']
        if 'ActivityError' in t:
            split = _head_split(ℓ.comps)
            if split is None or [type(c).__name__ for c in split[0]] not in (HEAD_COMPS, HEAD_COMPS_SUPER, HEAD_COMPS_SQ, HEAD_COMPS_SQ_LIN):
                refuse_activity(ℓ.comps, 'layer %r' % (ℓ.name,))
            return 'head'
        if t == ['ToPyramid'] or t == ['ToPyramid', 'MultiscaleLLN']:
            return 'pyramid'
        if t == BLOCK_COMPS:
            return 'block'
        if t in (HEAD_COMPS, HEAD_COMPS_SUPER, HEAD_COMPS_SQ, HEAD_COMPS_SQ_LIN):
            return 'head'
    raise NotImplementedError(
        'layer %r (%s) is outside the MI355X hot path: supported tree nodes are the '
        'ToPyramid (with or without MultiscaleLLN), ReConvMax and LogReg chains of arch_and_hypers.py' % (ℓ.name, type(ℓ).__name__))


def head_parts(chain):
    """Of a head chain (any of the HEAD_COMPS shapes, with or without ActivityError layers): its LinTrans and its error layer,
    found by type, the loss kind of its records (MPNN_LOSS_*) and the ϵ of the cross-entropy forms (0 for SquaredError,
    which has none and whose kernels do not read it)."""
    comps = [c for c in chain.comps if type(c).__name__ not in ('ActivityError', 'Dropout')]
    lt = next(c for c in comps if type(c).__name__ == 'LinTrans')
    err = comps[-1]
    if type(err).__name__ == 'SquaredError':
        return lt, err, (_hip.LOSS_SQ if any(type(c).__name__ == 'Softmax' for c in comps) else _hip.LOSS_SQ_LIN), 0.0
    return lt, err, _hip.LOSS_CE, float(err.hypers.ϵ)


def head_activity(chain):
    """(α 'map', α 'logits', α 'probs') of a head chain: the summed α of its ActivityError layers at each of the three
    positions, zeros for a head without the layer -- act_alpha of its mpnn_lin_bwd record, act_z and act_p of its tail
    record.  Only the training records carry them: evaluation and predict programs ignore the layer."""
    return tuple(_head_split(chain.comps)[1])


class _Node:
    pass


class BoundInput:
    """Feed value for ``net.x0`` / ``net.y`` that means "whatever the step's prologue puts into the engine's own
    input buffer" (lib/data.py: Dataset.bind_engine -- the on-device batch assembly is launch 0 of the step).  It
    names the buffer instead of holding a view of it: the buffers are reallocated when a larger batch comes by (the
    statistics pass at 4 096 images), and a view taken before that would feed the step from an orphaned allocation."""

    def __init__(self, eng, which, n):
        self.eng, self.which, self.n = eng, which, int(n)

    @property
    def shape(self):
        return (self.n,) + tuple(getattr(self.eng, self.which).shape[1:])

    def tensor(self):
        return getattr(self.eng, self.which)[:self.n]


class _Block:
    pass


def _marker(st):
    return 0                                  # (a marker launches nothing)


class Launch:
    """One entry of a program: calling it with a stream runs fn(*args, stream) of the kernel library.  A marker -- made
    with fn None: 'fork' / 'join' of the side streams, 'bucket' (tag: a gradient bucket that is final) -- does nothing.
    stream, waits, records: its place in the multi-stream schedule (the events it waits for and records); host: its
    per-net records in host memory, which the co-trainer (lib/_co.py) concatenates and K-step replay (lib/_eng_ksteps.py)
    copies -- the count of a table-driven launch is len(host); reserve: compute units its grid leaves free."""
    __slots__ = ('fn', 'args', 'what', 'tag', 'flops', 'stream', 'waits', 'records', 'host', 'reserve')

    def __init__(self, fn, what, *args, flops=0.0, tag='', stream=0, waits=(), records=None, host=None, reserve=0):
        self.fn, self.args, self.what, self.tag, self.flops = _marker if fn is None else fn, args, what, tag, float(flops)
        self.stream, self.waits, self.records, self.host, self.reserve = stream, tuple(waits), records, host, reserve

    def __call__(self, st):
        check(self.fn(*self.args, st), self.what)

    def with_table(self, table, host=None):
        """A copy that reads its records from `table`, every other field kept.  The first argument of a launch is where its
        records are: the device table of a table-driven launch, fn(table, count, ...), or the one record of mpnn_route,
        fn(&record).  host: the records `table` holds, if they are not this launch's own (a list: the count becomes
        len(host))."""
        c = copy.copy(self)
        c.args = (table,) + self.args[1:]
        if host is not None:
            c.host = host
            if isinstance(host, list):
                c.args = (table, len(host)) + self.args[2:]
        return c


def copy_record(rec, **fields):
    """A copy of the ctypes record `rec` with `fields` set."""
    c = type(rec)()
    C.memmove(C.byref(c), C.byref(rec), C.sizeof(rec))
    for k, v in fields.items():
        setattr(c, k, v)
    return c

