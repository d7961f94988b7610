"""Net types: statically-routed, actor and critic networks, MI355X-native.

Mirrors ``scripts/lib/net_types.py`` of the reference: same class names,
constructor keywords, placeholders (``x0, y, mode, λ_lrn, μ_lrn, ϵ, τ, k_cpt``),
``train`` op and tree iterators, so ``arch_and_hypers.py`` and a ``train-nets``
style driver work unchanged:

    net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: lr, net.τ: τ})

What differs: the reference assembles a TensorFlow graph (routing products,
expected costs, ``minimize_expectation``) and lets TF differentiate it; here
``link`` only infers shapes and registers parameters, and the arithmetic is a
static plan of hand-written HIP kernel launches (``lib/_plan.py``):

* routing probabilities, costs and their gradients -> ``mpnn_route``
  (reference: net_types.py:108-131, 165-177, 193-243, 273-280);
* TALR scaling + L2 + momentum -> ``mpnn_talr_momentum_step``
  (reference: net_types.py:24-37 and tf.train.MomentumOptimizer).
"""
from abc import ABCMeta
from types import SimpleNamespace as Ns

import numpy as np

from lib.layer_types import BatchNorm, Chain, Layer, LinTrans, NoOp, Rect, Sym, _Linker

################################################################################
# Support Functions  (reference: net_types.py:14-22)
################################################################################

def n_leaves(ℓ):
    return 1 if len(ℓ.sinks) == 0 else sum(map(n_leaves, ℓ.sinks))


def params_list_rec(ℓ):
    if ℓ is not None:
        yield from vars(ℓ.params).values()
        for c in getattr(ℓ, 'comps', []):
            yield from params_list_rec(c)

################################################################################
# Placeholders and the train op (session-free stand-ins for the TF idioms)
################################################################################

class Placeholder:
    """A feedable input; hashable so it can key a feed dict like a tf.placeholder."""

    def __init__(self, name, default=None):
        self.name = name
        self.default = default

    def __repr__(self):
        return '<placeholder %s>' % self.name


class _TrainOp:
    def __init__(self, net):
        self._net = net

    def run(self, feed):
        return self._net._run_train(feed)

    def run_steps(self, feeds):
        """len(feeds) consecutive training steps, replayed as ONE hipGraph where the engine can (Engine.run_steps);
        the same results as calling run() on each feed in turn."""
        eng = self._net.engine()
        if hasattr(eng, 'run_steps'):
            return eng.run_steps(list(feeds))
        for f in feeds:                                   # (the single-scale Conv engine: step by step)
            eng.run(f, train=True)

class _Curve(Ns):
    """What ``Net.exit_conf_curve`` returns: the arrays, and ``tau_for_ops``."""

    def tau_for_ops(self, budget):
        """The point with the highest accuracy whose mean operation count stays within ``budget`` (the first such point on
        ties): a namespace ``index, tau, acc, moc``, or None if no point does.  For the 1-D form of ``taus`` (one threshold
        per point); ValueError for a curve of per-leaf rows."""
        if self._points is None:
            raise ValueError('tau_for_ops: the curve was computed from per-leaf threshold rows [T, n_leaves]; there is no one '
                             'threshold per point to return')
        ok = np.flatnonzero(self.moc <= budget)
        if ok.size == 0:
            return None
        k = int(ok[np.argmax(self.acc[ok])])
        return Ns(index=k, tau=float(self._points[k]), acc=float(self.acc[k]), moc=float(self.moc[k]))

################################################################################
# Root Network Class  (reference: net_types.py:43-79)
################################################################################

class Net(metaclass=ABCMeta):
    default_hypers = Ns(x0_shape=(), y_shape=())
    _net_kind = 'sr'

    def __init__(self, **options):
        self.root = options.pop('root', NoOp())
        self.hypers = Ns(**{**vars(type(self).default_hypers), **options})
        self.params = Ns()
        self.x0 = Placeholder('x0')
        self.y = Placeholder('y')
        self.mode = Placeholder('mode', 'ev')
        self.train = _TrainOp(self)
        self._engine = None
        self._device = None
        self._dp = None
        with _Linker() as lk:
            self.link()
        self._all_params = lk.params

    # -- graph construction ----------------------------------------------------
    def _k_cpt_dyn(self):
        return bool(getattr(self.hypers, 'dyn_k_cpt', False))

    def link(self):
        dyn = self._k_cpt_dyn()

        def with_k_cpt(x_):                       # reference: net_types.py:149-154
            s = Sym((x_.n_el + 1,), x_.producer)
            s.base = x_
            return s

        def link_layer(ℓ, x, y, mode):
            ℓ.link(x, y, mode)
            if ℓ.router is not None:
                if not dyn:
                    x_rte = ℓ.x
                elif isinstance(ℓ.x, list):
                    x_rte = list(map(with_k_cpt, ℓ.x))
                else:
                    x_rte = with_k_cpt(ℓ.x)
                ℓ.router.dyn_k_cpt = dyn
                ℓ.router.link(x_rte, y, mode)
            for s in ℓ.sinks:
                link_layer(s, ℓ.x, y, mode)
        link_layer(self.root, Sym(self.hypers.x0_shape), Sym(self.hypers.y_shape), self.mode)

    @property
    def layers(self):
        def all_in_tree(layer):
            yield layer
            for sink in layer.sinks:
                yield from all_in_tree(sink)
        yield from all_in_tree(self.root)

    @property
    def leaves(self):
        return (ℓ for ℓ in self.layers if len(ℓ.sinks) == 0)

    @property
    def leaf_n_cls(self):
        """The width of each leaf's label space, in ``net.leaves`` order: the columns of ``w_cls`` for an exit that ends in
        ``SuperclassCrossEntropyError``, the net's ``y_shape[0]`` for every other."""
        def width(ℓ):
            last = ℓ.comps[-1] if getattr(ℓ, 'comps', None) else None
            if type(last).__name__ == 'SuperclassCrossEntropyError':
                return int(np.shape(last.hypers.w_cls)[1])
            return int(self.hypers.y_shape[0])
        return [width(ℓ) for ℓ in self.leaves]

    @property
    def switches(self):
        return (ℓ for ℓ in self.layers if len(ℓ.sinks) > 1)

    # -- execution ---------------------------------------------------------------
    def to(self, device):
        """Pin the net to a device before first use (default: cuda:LOCAL_RANK)."""
        self._device = device
        return self

    def engine(self):
        if self._engine is None:
            from lib._plan import Engine          # imports the HIP library; raises if missing
            from lib._plan_conv import ConvEngine, is_conv_net
            # (a statically-routed chain of single-scale Conv layers has its own, simpler plan)
            self._engine = (ConvEngine if is_conv_net(self) else Engine)(self, self._device)
        return self._engine

    def _run_train(self, feed):
        return self.engine().run(feed, train=True)

    @property
    def dropout_step(self):
        """The step counter t the net's Dropout layers draw their next training step's masks with (layer_types.py: Dropout):
        0 at first, + 1 per training step, untouched by evaluation.  Settable: a net set back to a step repeats its masks."""
        return self.engine().dropout_step

    @dropout_step.setter
    def dropout_step(self, t):
        self.engine().dropout_step = t

    def eval(self, feed, routed=False):
        """Forward pass + routing in evaluation mode ('ev': BatchNorm moving averages, hard routing);
        per-layer results are then readable as ``ℓ.p_ev``, ``ℓ.δ_cor`` ... device tensors.

        routed='auto' picks the routed evaluation from 512 samples per launch on and the dense one below
        (Engine.routed_min_batch); routed=True runs the ROUTED evaluation: a block only processes the samples its ancestors'
        routers sent to it (sample lists compacted on the device, no host sync) -- from a depth the engine picks by
        batch size (Engine.routed_prefix: the first blocks lose few samples, and below ~6 000 samples running their
        convs on everybody in wavefront-grouped launches is faster than gathering); routed=<int d> sets that depth
        (1: every block below the root gathers).  ``p_ev`` and every
        p_ev-weighted statistic (acc, moc, p_cor, p_inc, *_by_cls: all that the reference's figure
        scripts read) are identical to the dense pass; per-leaf ``c_err`` / ``δ_cor`` and ``router.x``
        are those of the dense pass where the sample reaches the node and 0 elsewhere."""
        return self.engine().run(feed, train=False, routed=routed)

    @property
    def gateable_leaves(self):
        """Indices into ``net.leaves`` of the exits a confidence threshold can gate (``predict(exit_conf=)``): the classifier
        leaves that hang directly under a layer with a router -- in the shipped ``dr_chain`` / ``dr_tree`` nets every exit
        but the last of a chain.  Exits below static nodes (no router: nothing decides there) are not among them."""
        index = {id(ℓ): k for k, ℓ in enumerate(self.leaves)}
        return sorted(index[id(s)] for ℓ in self.layers if ℓ.router is not None for s in ℓ.sinks if len(s.sinks) == 0)

    def _check_exit_conf(self, who, exit_conf):
        """The thresholds of predict(exit_conf=) as one entry per leaf (a float, or None: not gated), or None; refusals come
        before an engine is needed."""
        if exit_conf is None:
            return None
        import numbers
        real = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)
        n = len(list(self.leaves))
        if real(exit_conf):
            vals = [exit_conf] * n
        elif isinstance(exit_conf, (list, tuple, np.ndarray)) and np.ndim(exit_conf) == 1:
            vals = list(exit_conf)
            if len(vals) != n:
                raise ValueError('%s: exit_conf has %d entries for the %d leaves of the net (one per leaf, in net.leaves '
                                 'order; None leaves a switch to its router)' % (who, len(vals), n))
        else:
            raise ValueError('%s: exit_conf is None, one real number or a sequence with one entry per leaf, not %r' % (who, exit_conf))
        for v in vals:
            if v is not None and not real(v):
                raise ValueError('%s: an entry of exit_conf is a real number or None, not %r' % (who, v))
        gateable = set(self.gateable_leaves)
        if not gateable:
            raise ValueError('%s: exit_conf given, but the net has no exit under a block with a router (nothing to gate)' % who)
        return tuple(float(v) if (v is not None and k in gateable) else None for k, v in enumerate(vals))

    def predict(self, x0, routed='auto', probs=False, k_cpt=None, decode=None, exit_conf=None):
        """Classify unlabelled images: the evaluation-mode forward pass without labels.  Returns a namespace of device
        tensors, one entry per image:

            cls   int32   predicted class (arg-max of the softmax at the exit taken, first index on ties): an index into the
                          label space of THAT exit -- one of ``net.leaf_n_cls[leaf]`` classes, the superclasses of its map
                          for an exit that ends in ``SuperclassCrossEntropyError``
            leaf  int32   index into ``net.leaves`` of the exit taken
            conf  float32 softmax probability of ``cls`` at that exit
            ops   int64   operations spent on the image (blocks and routers on its path: the per-sample ``moc``)
            probs float32 [n, max(net.leaf_n_cls)] softmax row at that exit, zero beyond the exit's own
                          ``net.leaf_n_cls[leaf]`` entries (``probs=True``; otherwise None)

        An exit that ends in ``SquaredError`` directly behind its ``LinTrans`` (no ``Softmax``: the regression form) has no
        probabilities: there ``cls`` is the arg-max of the RAW outputs, ``conf`` the raw output of that class (it may be
        negative) and the ``probs`` row the raw outputs.

        They view persistent buffers and stay valid until the next run.  ``routed`` as in ``eval`` (the same programs,
        sample lists and gather depths; default 'auto').  ``k_cpt`` (one value or one per image) is required for a
        ``dyn_k_cpt`` net and refused otherwise.  ``state()`` after ``predict`` raises: there are no labels.

        ``decode`` ('gamma', 'unit' or a table of 256 values: lib/decode.py): ``x0`` holds 8-bit pixels (uint8, a numpy
        array or a torch tensor on the host or the device); they are uploaded as bytes and turned into floats on the
        device, ``table[x0]``, in front of the same program -- the result is that of ``predict(table[x0])``, bit for bit.
        Float images with ``decode`` raise ValueError.

        ``exit_conf``: the CONFIDENCE-THRESHOLD exit policy instead of the learnt routers' -- an image leaves at the first
        exit on its path whose ``conf`` reaches the threshold (``conf >= τ`` in float32; a NaN on either side is "no");
        where it does not, the block's router still picks among the child blocks (a tree's switches).  None (default: the
        learnt routers, the programs of before, launch for launch); one real number for every gateable exit; or a sequence of
        ``len(list(net.leaves))`` entries in ``net.leaves`` order, None leaving that switch to its router.  An exit is
        gateable when it hangs under a block with a router (``net.gateable_leaves``); entries for other leaves -- the last
        exit of a chain, exits below static nodes -- are ignored.  For softmax exits a threshold of 0 or below always
        leaves and one above 1 never does; for ``squared-linear`` exits the comparison is on the raw ``conf`` reported
        above.  The thresholds are values in device memory: a sweep re-uses one program and one captured graph.  ``ops``
        stays the sum over the nodes on the image's path, the router of every gated switch it reaches included (it runs,
        and chooses among the children), exactly as under the learnt policy.  ValueError before an engine is needed: a
        sequence of the wrong length, an entry that is no real number, a net without a gateable exit."""
        exit_conf = self._check_exit_conf('predict', exit_conf)
        if decode is not None:
            from lib.decode import check_decode_input
            decode = check_decode_input('predict', x0, decode)   # (the table; refusals come before an engine is needed)
        eng = self.engine()
        if not hasattr(eng, 'predict'):
            raise NotImplementedError('predict: single-scale Conv nets (ConvEngine) have no label-free evaluation')
        return eng.predict(x0, routed=routed, probs=probs, k_cpt=k_cpt, table=decode, exit_conf=exit_conf)

    def predict_all(self, x, batch=4096, routed='auto', probs=False, k_cpt=None, decode=None, exit_conf=None):
        """Classify a whole array of images, of any length, ``batch`` images per launch: the namespace of ``predict``
        with one entry per image of ``x`` -- the concatenation of ``predict`` over the chunks, bit for bit.  The tensors
        are allocations of their own (not views of the per-launch buffers): they stay valid after later runs.

        ``x``: float32 images, or uint8 pixels with ``decode`` (as in ``predict``).  A host array is streamed: while one
        chunk's program runs, the next chunk is copied into a pinned buffer and uploaded on a copy stream; the host
        never waits for the results.  A device tensor is read where it lies.  ``k_cpt`` of a ``dyn_k_cpt`` net: one
        value, or one per image of ``x``.  No image: empty tensors of the result types, no launch.  ``exit_conf`` as in
        ``predict``: the same thresholds for every chunk."""
        exit_conf = self._check_exit_conf('predict_all', exit_conf)
        from lib.decode import check_decode_input
        table = check_decode_input('predict_all', x, decode)
        if int(batch) != batch or batch < 1:
            raise ValueError('predict_all: batch is a positive number of images per launch, not %r' % (batch,))
        if not hasattr(x, 'shape') or len(x.shape) < 1:
            raise ValueError('predict_all: x is an array of images [n, H, W, C]')
        eng = self.engine()
        if not hasattr(eng, 'predict_all'):
            raise NotImplementedError('predict_all: single-scale Conv nets (ConvEngine) have no label-free evaluation')
        return eng.predict_all(x, batch=int(batch), routed=routed, probs=probs, k_cpt=k_cpt, table=table, exit_conf=exit_conf)

    @property
    def threshold_exits(self):
        """Indices into ``net.leaves`` of the exits a threshold of ``exit_conf_curve`` applies to: ``gateable_leaves`` plus
        the exits under STATIC forks -- a layer without a router whose sinks are one classifier leaf and one other layer
        (a deeply supervised ``SRNet``: an exit under every block of a chain)."""
        index = {id(ℓ): k for k, ℓ in enumerate(self.leaves)}
        return sorted(index[id(s)] for ℓ in self.layers if len(ℓ.sinks) > 1 for s in ℓ.sinks if len(s.sinks) == 0)

    def exit_conf_curve(self, x0, y, taus, batch=4096, k_cpt=None, decode=None):
        """The accuracy-versus-operations curve of confidence-threshold exits on a labelled data set, in ONE dense pass:
        for each of T threshold points, how many images are classified correctly, how many operations they cost and where
        they leave, when every image leaves at the first exit on its path whose ``conf`` reaches that exit's threshold
        (the policy of ``predict(exit_conf=)``; where it does not, a block's router still picks among its child blocks).
        All heads and routers are evaluated once per image; what an image does under a threshold row is then a walk over
        numbers that are already on the device (csrc/exit_curve.hip), summed there in integers.

        ``x0`` [n, H, W, C] (float32, or uint8 with ``decode``: as in ``predict_all``, streamed in chunks of ``batch``),
        ``y`` [n, n_classes] the labels as ``eval`` takes them.  ``taus``: 1-D [T] -- one threshold per point for every exit
        in ``net.threshold_exits`` -- or 2-D [T, n_leaves] in ``net.leaves`` order, NaN meaning "not gated" (that switch
        stays with its router; a static fork is passed by).  Entries for exits no threshold applies to are ignored.  A row
        that is all NaN is the learnt policy of ``eval``.  Unlike ``predict(exit_conf=)`` the curve also covers statically
        forked nets (``SRNet`` chains with an exit under every block).  ``k_cpt`` as in ``predict``.

        Returns a namespace: ``n``; ``taus`` [T, n_leaves] float32 as used (NaN where no threshold applies); ``correct``,
        ``ops`` int64 [T] and ``hist`` int64 [T, n_leaves] (exact sums: images right, operations spent -- blocks and routers
        on the path, as ``predict`` counts them -- and images per exit); ``acc = correct / n`` and ``moc = ops / n``
        (float64); ``tau_for_ops(budget)`` for the 1-D form.

        ValueError before an engine is needed: ``taus`` of the wrong rank or width, without a point, or with entries that
        are no real numbers; ``y`` missing or of the wrong shape; ``decode`` with float images; a net without a threshold
        exit; a static fork that is not "one exit + one child" (nothing chooses among several children)."""
        who = 'exit_conf_curve'
        if self._engine is None:                              # (asked of the net: no engine is built to refuse)
            from lib._plan_conv import is_conv_net
            conv = is_conv_net(self)
        else:
            conv = not hasattr(self._engine, 'exit_conf_curve')
        if conv:
            raise NotImplementedError('%s: single-scale Conv nets (ConvEngine) have no exits to leave at' % who)
        leaves = list(self.leaves)
        for ℓ in self.layers:
            if ℓ.router is None and len(ℓ.sinks) > 1:
                n_exit = sum(1 for s in ℓ.sinks if len(s.sinks) == 0)
                if len(ℓ.sinks) != 2 or n_exit != 1:
                    raise ValueError('%s: a static fork (no router) with %d sinks, %d of them exits: only "one exit + one child" '
                                     'can be walked -- nothing chooses among several child blocks' % (who, len(ℓ.sinks), n_exit))
        exits = self.threshold_exits
        if not exits:
            raise ValueError('%s: the net has no exit a threshold applies to (none under a router or a static fork)' % who)
        try:
            t = np.asarray(taus)
            real = t.dtype.kind in 'fiu'
        except Exception:
            real = False
        if not real:
            raise ValueError('%s: taus is an array of real numbers, [T] or [T, n_leaves], not %r' % (who, taus))
        if t.ndim not in (1, 2) or (t.ndim == 2 and t.shape[1] != len(leaves)):
            raise ValueError('%s: taus of shape %r: one threshold per point, [T], or one per point and leaf, [T, %d] in '
                             'net.leaves order' % (who, t.shape, len(leaves)))
        if t.shape[0] == 0:
            raise ValueError('%s: taus holds no point (T = 0)' % who)
        used = np.full((t.shape[0], len(leaves)), np.nan, np.float32)
        used[:, exits] = t[:, None] if t.ndim == 1 else t[:, exits]
        if not hasattr(x0, 'shape') or len(x0.shape) < 1:
            raise ValueError('%s: x0 is an array of images [n, H, W, C]' % who)
        n = int(x0.shape[0])
        if y is None or not hasattr(y, 'shape') or tuple(y.shape) != (n,) + tuple(self.hypers.y_shape):
            raise ValueError('%s: y holds the labels of the %d images, [%d, %d] as net.eval takes them, not %r'
                             % (who, n, n, self.hypers.y_shape[0], None if y is None else tuple(getattr(y, 'shape', ()))))
        if int(batch) != batch or batch < 1:
            raise ValueError('%s: batch is a positive number of images per launch, not %r' % (who, batch))
        dyn = self._k_cpt_dyn()
        if dyn and k_cpt is None:
            raise ValueError('%s: a dyn_k_cpt net needs k_cpt (one value, or one per image)' % who)
        if not dyn and k_cpt is not None:
            raise ValueError('%s: k_cpt is an input of dyn_k_cpt nets only; this net has a fixed k_cpt' % who)
        from lib.decode import check_decode_input
        table = check_decode_input(who, x0, decode)
        correct, ops, hist = self.engine().exit_conf_curve(x0, y, used, batch=int(batch), k_cpt=k_cpt, table=table)
        one_d = t.astype(np.float32) if t.ndim == 1 else None
        return _Curve(n=n, taus=used, correct=correct, ops=ops, hist=hist, acc=correct / max(n, 1), moc=ops / max(n, 1),
                      _points=one_d)

    def state(self):
        """Per-sample statistics of the last run, keyed like the reference's
        ``state_tensors`` (scripts/train-nets:117-130)."""
        return self.engine().state()

################################################################################
# Statically-Routed Networks  (reference: net_types.py:85-97)
################################################################################

class SRNet(Net):
    default_hypers = Ns(λ_lrn=1e-3, μ_lrn=0.9, seed=None)
    _net_kind = 'sr'

    def link(self):
        super().link()
        ϕ = self.hypers
        self.λ_lrn = Placeholder('λ_lrn', ϕ.λ_lrn)
        self.μ_lrn = Placeholder('μ_lrn', ϕ.μ_lrn)

################################################################################
# Actor Networks  (reference: net_types.py:103-181)
################################################################################

class ActorNet(Net):
    default_hypers = Ns(
        k_cpt=0.0, k_dec=0.01, ϵ=1e-6, τ=1.0, λ_lrn=1e-3, μ_lrn=0.9,
        dyn_k_cpt=False, α_cpt=1e7, talr=True, α_rtr=1.0, seed=None)
    _net_kind = 'actor'

    def link(self):
        ϕ = self.hypers
        self.λ_lrn = Placeholder('λ_lrn', ϕ.λ_lrn)
        self.μ_lrn = Placeholder('μ_lrn', ϕ.μ_lrn)
        self.ϵ = Placeholder('ϵ', ϕ.ϵ)
        self.τ = Placeholder('τ', ϕ.τ)
        self.k_cpt = Placeholder('k_cpt') if ϕ.dyn_k_cpt else ϕ.k_cpt
        super().link()

################################################################################
# Critic Networks  (reference: net_types.py:187-284)
################################################################################

class CriticNet(Net):
    default_hypers = Ns(
        k_cpt=0.0, k_cre=1e-3, ϵ=1e-6, τ=0.01, optimistic=False,
        dyn_k_cpt=False, α_cpt=1e7, use_cls_err=False, λ_lrn=1e-3, μ_lrn=0.9,
        talr=True, α_rtr=1.0, seed=None)
    _net_kind = 'critic'

    def link(self):
        ϕ = self.hypers
        self.λ_lrn = Placeholder('λ_lrn', ϕ.λ_lrn)
        self.μ_lrn = Placeholder('μ_lrn', ϕ.μ_lrn)
        self.ϵ = Placeholder('ϵ', ϕ.ϵ)
        self.τ = Placeholder('τ', ϕ.τ)
        self.k_cpt = Placeholder('k_cpt') if ϕ.dyn_k_cpt else ϕ.k_cpt
        super().link()
