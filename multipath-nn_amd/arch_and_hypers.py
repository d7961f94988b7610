"""Architecture, hyper-parameters and net constructors of the shipped experiments.

Same public names as the reference's ``scripts/arch_and_hypers.py`` (``arch``,
``k_cpts``, ``batch_size``, ``n_iter``, ``t_log``, ``λ_lrn``, ``τ_cr``, ``τ_ds``,
``router``, ``pyr``, ``rcm``, ``reg``, ``sr_chain``, ``ac_chain``, ``cr_chain``,
``ac_tree``, ``cr_tree``); the reference's own file also runs unchanged on top of
``lib/`` (tests/test_host_cpu.py::test_reference_spec_file_drops_in_unchanged).  Values: reference
arch_and_hypers.py:12-39; builders :45-70; constructors :76-139.
"""
import unicodedata

import numpy as np

from lib.layer_types import (
    ActivityError, BatchNorm, Chain, CrossEntropyError, Dropout, LinTrans, MultiscaleBatchNorm,
    MultiscaleConvMax, MultiscaleLLN, MultiscaleRect, Rect, Select, Softmax,
    SquaredError, SuperclassCrossEntropyError, ToPyramid)
from lib.net_types import ActorNet, CriticNet, SRNet

# ---- network hyper-parameters ------------------------------------------------
conv_supp = 3
router_n_chan = 16
k_cpts = [0.0] + [1e-9 * 2 ** i for i in range(7)]       # 0, 1e-9 ... 6.4e-8
k_l2 = 1e-4
σ_w = 1
arch = [4 * [16], 4 * [16], 3 * [32], 3 * [32], 2 * [64], 2 * [64], [128], [128]]
# None: the reference's nets.  A dict of MultiscaleLLN hypers ({} for its defaults σ = 3, ϵ = 1e-3): every net normalises
# the pyramid's local luminance in front of block 0 (read when a constructor is called, like `arch`)
lln = None
# None: every exit classifies the net's classes.  A dict {block index: w_cls}: the exit under that block classifies the
# superclasses of the constant [n_cls, n_sup] map w_cls instead (SuperclassCrossEntropyError: its labels are y @ w_cls);
# read when a constructor is called.  sr_chain(n_tf) has one exit, under block n_tf - 1.
coarse_exits = None
# None: every exit ends in a cross-entropy.  'squared' (Softmax -> SquaredError: a Brier score) or 'squared-linear' (SquaredError
# on the LinTrans output itself: regression, y any float vector): every exit; a dict {block index: one of the two}: the
# exits under those blocks.  Read when a constructor is called.
exit_loss = None
EXIT_LOSSES = ('squared', 'squared-linear')
# None: no activity penalty.  A dict {'map': α, 'logits': α, 'probs': α} (any subset): every exit carries ActivityError layers --
# c_mod = α sum(x^2) per sample -- on the block's coarsest activation map, on its logits and on its softmax outputs ('probs' not
# on a 'squared-linear' exit, which has no Softmax); a dict {block index: such a dict}: the exits under those blocks.  Read
# when a constructor is called.
exit_activity = None
ACTIVITY_WHERE = ('map', 'logits', 'probs')
# None: no dropout.  A keep probability λ, 0 < λ <= 1: every exit has a Dropout(λ) directly in front of its LinTrans (training
# only: evaluation is the identity; not together with a 'map' activity penalty); a dict {block index: λ}: the exits under
# those blocks.  dropout_seed: the seed of those layers' random stream (train-nets gives net i of an experiment
# --dropout-seed + i).  Both read when a constructor is called.
exit_dropout = None
dropout_seed = 0

# ---- training hyper-parameters -------------------------------------------------
n_iter = 80000
t_log = 2500
batch_size = 128


def λ_lrn(t):
    return 0.1 / 2 ** (t / 10000)


def τ_cr(t):
    return 0.1 / 2 ** (t / 20000)


def τ_ds(t):
    return 1 / 2 ** (t / 20000)

# ---- components ---------------------------------------------------------------------

def _dense(n_out, **kw):
    return LinTrans(n_chan=n_out, k_l2=k_l2, **{'σ_w': σ_w, **kw})


def router(n_sinks):
    """Coarsest scale -> 16 -> 16 -> n_sinks MLP; the last map starts at zero."""
    if n_sinks < 2:
        return None
    hidden = []
    for _ in range(2):
        hidden += [_dense(router_n_chan), BatchNorm(), Rect()]
    return Chain(name='Router', comps=[Select(i=-1), *hidden, _dense(n_sinks, σ_w=0)])


def pyr(*sinks):
    comps = [ToPyramid(n_scales=len(arch[0]))]
    if isinstance(lln, dict):
        # (Python NFKC-normalises identifiers but not string keys: {'ϵ': ..} must land on the attribute that `hypers.ϵ` reads)
        comps.append(MultiscaleLLN(**{unicodedata.normalize('NFKC', k): v for k, v in lln.items()}))
    return Chain(name='ToPyramid', sinks=sinks, router=router(len(sinks)), comps=comps)


def rcm(i, *sinks):
    body = [MultiscaleConvMax(n_chan=arch[i], supp=conv_supp, k_l2=k_l2, σ_w=σ_w),
            MultiscaleBatchNorm(), MultiscaleRect()]
    return Chain(name='ReConvMax', sinks=sinks, router=router(len(sinks)), comps=body)


def _check_activity(activity, who):
    if not isinstance(activity, dict) or any(k not in ACTIVITY_WHERE for k in activity):
        raise ValueError('%s: activity is None or a dict with keys among %s, not %r' % (who, ', '.join(map(repr, ACTIVITY_WHERE)), activity))
    for k, α in activity.items():
        if isinstance(α, bool) or not isinstance(α, (int, float, np.integer, np.floating)) or not np.isfinite(α):
            raise ValueError('%s: activity[%r] is a finite float, not %r' % (who, k, α))


def _check_dropout(λ, who):
    if isinstance(λ, bool) or not isinstance(λ, (int, float, np.integer, np.floating)) or not 0 < λ <= 1:
        raise ValueError('%s: dropout is None or a keep probability λ, 0 < λ <= 1, not %r' % (who, λ))


def reg(n_chan, w_cls=None, loss=None, activity=None, dropout=None, seed=0):
    """The exit classifier: n_chan classes, or -- with a map w_cls [n_chan, n_sup] -- the n_sup superclasses of the map.
    loss: None (cross-entropy), 'squared' (SquaredError on the softmax) or 'squared-linear' (SquaredError on the
    LinTrans output, no Softmax); not together with w_cls.
    activity: None, or {'map': α, 'logits': α, 'probs': α} (any subset): an ActivityError(α) behind Select, behind the
    LinTrans and behind the Softmax; 'probs' not together with loss='squared-linear'.
    dropout: None, or the keep probability λ of a Dropout(λ, seed) directly in front of the LinTrans; not together with
    activity['map'] (the penalty would have to choose between the map and its dropped copy)."""
    if loss is not None:
        if w_cls is not None:
            raise ValueError('reg: a squared-error exit has no label space of its own (loss=%r together with w_cls)' % (loss,))
        if loss not in EXIT_LOSSES:
            raise ValueError('reg: loss is None, %s, not %r' % (' or '.join(map(repr, EXIT_LOSSES)), loss))
        comps = [Select(i=-1), _dense(n_chan)] + ([Softmax()] if loss == 'squared' else []) + [SquaredError()]
    elif w_cls is not None:
        comps = [Select(i=-1), _dense(np.shape(w_cls)[1]), Softmax(), SuperclassCrossEntropyError(w_cls=w_cls)]
    else:
        comps = [Select(i=-1), _dense(n_chan), Softmax(), CrossEntropyError()]
    if activity is not None:
        _check_activity(activity, 'reg')
        if 'probs' in activity and loss == 'squared-linear':
            raise ValueError("reg: a 'squared-linear' exit has no Softmax whose outputs activity['probs'] could penalise")
        for where, after in (('probs', Softmax), ('logits', LinTrans), ('map', Select)):
            if where in activity:
                k = next(j for j, c in enumerate(comps) if isinstance(c, after))
                comps.insert(k + 1, ActivityError(α=float(activity[where])))
    if dropout is not None:
        _check_dropout(dropout, 'reg')
        if activity is not None and 'map' in activity:
            raise ValueError("reg: dropout in front of the LinTrans does not go together with activity['map']")
        comps.insert(1, Dropout(λ=float(dropout), seed=int(seed)))
    return Chain(name='LogReg', comps=comps)


def _exit(i, n_cls):
    """The exit under block i: coarse where `coarse_exits` names the block, squared where `exit_loss` does, with the
    activity penalties `exit_activity` gives it and the dropout `exit_dropout` does."""
    loss = exit_loss.get(i) if isinstance(exit_loss, dict) else exit_loss
    act = exit_activity
    if isinstance(act, dict) and not any(k in ACTIVITY_WHERE for k in act):      # ({block index: dict}; {} is no penalty)
        act = act.get(i)
    drop = exit_dropout.get(i) if isinstance(exit_dropout, dict) else exit_dropout
    return reg(n_cls, coarse_exits.get(i) if isinstance(coarse_exits, dict) else None, loss, act, drop, dropout_seed)


def parse_exit_loss(text):
    """The value of `exit_loss` for train-nets --exit-loss LOSS[:K]: LOSS for every exit, or {0: LOSS, ..., K-1: LOSS}."""
    loss, sep, k = text.partition(':')
    if loss not in EXIT_LOSSES or (sep and not k.isdigit()):
        raise ValueError('--exit-loss takes %s, optionally followed by :K, not %r' % (' or '.join(EXIT_LOSSES), text))
    return {i: loss for i in range(int(k))} if sep else loss


def parse_exit_activity(text):
    """The value of `exit_activity` for train-nets --exit-activity WHERE=ALPHA[,WHERE=ALPHA][:K]: the dict for every exit, or
    {0: dict, ..., K-1: dict}."""
    body, sep, k = text.partition(':')
    act = {}
    try:
        for item in body.split(','):
            where, eq, α = item.partition('=')
            if where not in ACTIVITY_WHERE or not eq or where in act:
                raise ValueError(item)
            act[where] = float(α)
            if not np.isfinite(act[where]):
                raise ValueError(item)
        if sep and not k.isdigit():
            raise ValueError(k)
    except ValueError:
        raise ValueError('--exit-activity takes WHERE=ALPHA[,WHERE=ALPHA], WHERE one of %s and ALPHA a finite float, optionally '
                         'followed by :K, not %r' % (', '.join(ACTIVITY_WHERE), text)) from None
    return {i: dict(act) for i in range(int(k))} if sep else act


def parse_exit_dropout(text):
    """The value of `exit_dropout` for train-nets --exit-dropout LAMBDA[:K]: λ for every exit, or {0: λ, ..., K-1: λ}."""
    body, sep, k = text.partition(':')
    try:
        λ = float(body)
        if not 0 < λ <= 1 or (sep and not k.isdigit()):
            raise ValueError(text)
    except ValueError:
        raise ValueError('--exit-dropout takes a keep probability LAMBDA, 0 < LAMBDA <= 1, optionally followed by :K, not %r'
                         % (text,)) from None
    return {i: λ for i in range(int(k))} if sep else λ

# ---- constructors -----------------------------------------------------------------------

def sr_chain(n_tf):
    """pyr -> rcm0 -> ... -> rcm(n_tf-1) -> reg."""
    def make_net(x0_shape, y_shape):
        node = _exit(n_tf - 1, y_shape[0])
        for i in range(n_tf - 1, -1, -1):
            node = rcm(i, node)
        return SRNet(x0_shape=x0_shape, y_shape=y_shape, root=pyr(node))
    return make_net


def dr_chain(type_, **hypers):
    """Every block gets an exit classifier (sink 0) and the next block (sink 1)."""
    def make_net(x0_shape, y_shape):
        node = rcm(len(arch) - 1, _exit(len(arch) - 1, y_shape[0]))
        for i in range(len(arch) - 2, -1, -1):
            node = rcm(i, _exit(i, y_shape[0]), node)
        return type_(x0_shape=x0_shape, y_shape=y_shape, root=pyr(node), **hypers)
    return make_net


def dr_tree(type_, **hypers):
    """Binary tree over blocks 0-2, then chains 3-7 (47 blocks, 47 leaves)."""
    def make_net(x0_shape, y_shape):
        n_cls = y_shape[0]

        def tail(i=3):
            return rcm(i, _exit(i, n_cls)) if i == len(arch) - 1 else rcm(i, _exit(i, n_cls), tail(i + 1))

        def fork(i):
            kids = (tail(), tail()) if i == 2 else (fork(i + 1), fork(i + 1))
            return rcm(i, _exit(i, n_cls), *kids)
        return type_(x0_shape=x0_shape, y_shape=y_shape, root=pyr(fork(0)), **hypers)
    return make_net


def ac_chain(**hypers):
    return dr_chain(ActorNet, **hypers)


def ac_tree(**hypers):
    return dr_tree(ActorNet, **hypers)


def cr_chain(**hypers):
    return dr_chain(CriticNet, **hypers)


def cr_tree(**hypers):
    return dr_tree(CriticNet, **hypers)
