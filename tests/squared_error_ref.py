"""Float64 reference of SquaredError, the reference's lines (scripts/lib/layer_types.py:255-260) written out literally:
c_err = sum((x - y)^2, 1), δ_cor = [argmax x == argmax y] (first index on ties: the stand-in's stated assumption and
what the exit kernels do); x passes through.  TEST INFRASTRUCTURE: nothing here is on the product path.

The exit kernels run the layer in two head forms, on z = the head's LinTrans output:
  'sq'   x = softmax(z)     dL/dz_k = w x_k (g_k - sum_j g_j x_j),  g = 2 (x - y)
  'lin'  x = z              dL/dz_k = 2 w (z_k - y_k)
``head_fwd`` / ``head_bwd`` are those in float64 (``dt=np.float32``: the same lines in numpy float32, the stand-in for
the kernels that shows a test's limit can be met before a GPU is touched); ``RefNetSquared`` is oracle.ref_net.RefNet
with the layer.  Below them: the case tables and inputs of tests/test_squared_head_kernels.py.
"""
import numpy as np
import torch

from oracle.ref_net import RefNet

F64 = np.float64
FORMS = ('sq', 'lin')
LOSS = {'sq': 1, 'lin': 2}                       # MPNN_LOSS_SQ, MPNN_LOSS_SQ_LIN


def layer(x, y):
    """(c_err, δ_cor) of the layer on rows x and targets y (:258-260), float64."""
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    c_err = np.sum(np.square(x - y), 1)
    δ_cor = np.equal(np.argmax(x, 1), np.argmax(y, 1)).astype(F64)
    return c_err, δ_cor


def softmax(z, dt=F64):
    z = np.asarray(z, dt)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _gap(v):
    """Top-two gap of every row (inf for one column)."""
    if v.shape[1] < 2:
        return np.full(len(v), np.inf)
    top = np.sort(np.asarray(v, F64), 1)
    return top[:, -1] - top[:, -2]


def head_fwd(z, y, form, dt=F64):
    """x, c_err, d_cor of a head, with the top-two gaps of x and of y."""
    z, y = np.asarray(z, dt), np.asarray(y, dt)
    x = softmax(z, dt) if form == 'sq' else z
    d = x - y
    c_err = (d * d).sum(1)
    return dict(x=x, c_err=c_err, d_cor=(x.argmax(1) == y.argmax(1)).astype(dt), cls=x.argmax(1), gap_x=_gap(x), gap_y=_gap(y))


def head_bwd(z, y, w, form, dt=F64):
    """(dL/dz, bound): bound = the sum of the absolute values of the element's own terms, every difference expanded --
    'lin': 2 |w| (|z_k| + |y_k|);  'sq': |w| x_k (2 (x_k + |y_k|) + sum_j 2 (x_j + |y_j|) x_j)."""
    z, y, w = np.asarray(z, dt), np.asarray(y, dt), np.asarray(w, dt)[:, None]
    if form == 'lin':
        return dt(2) * w * (z - y), 2 * np.abs(w) * (np.abs(z) + np.abs(y))
    x = softmax(z, dt)
    g = dt(2) * w * (x - y)
    dot = (g * x).sum(1, keepdims=True)
    ag = 2 * np.abs(w) * (x + np.abs(y))
    return x * (g - dot), x * (ag + (ag * x).sum(1, keepdims=True))


def head_fwd_t(z, y, form):
    """head_fwd's c_err on torch tensors (autograd checks head_bwd against it)."""
    x = torch.softmax(z, 1) if form == 'sq' else z
    return ((x - y) ** 2).sum(1)


class RefNetSquared(RefNet):
    """RefNet whose `_link` knows SquaredError: the same lines on torch float64 tensors; everything else is RefNet's
    (its Chain sums c_err over the components and forwards the last δ_cor)."""

    def _link(self, ℓ, x, y, mode, out):
        if type(ℓ).__name__ != 'SquaredError':
            return super()._link(ℓ, x, y, mode, out)
        yt = torch.as_tensor(y, dtype=self.dtype)
        out[id(ℓ)] = dict(c_err=torch.sum(torch.square(x - yt), 1), c_mod=0.0, n_ops=0, x=x,
                          δ_cor=(torch.argmax(x, 1) == torch.argmax(yt, 1)).to(self.dtype))
        return x


# ---- the limits of the GPU kernel tests: the project's constants (tests/test_exit_gen_kernels.py) ------------------------
c_err_lim = lambda ref: 2e-5 * (1 + np.abs(ref))
dz_lim = lambda ref, bound: 2e-5 * bound + 1e-9
OUT_TOL = 2e-4                                   # conf / p_cls: tests/test_predict_kernels.py's TOL * (1 + max |ref|)

# ---- the inputs of tests/test_squared_head_kernels.py (shared with the CPU test that shows its limits can be met) ---------
# (n, n_cls) of the exit-tail tests.  tuned: one sample, one class; two classes; a ragged batch; every limit of the
# LDS-resident kernel.  any-width (16 threads per sample, 64 samples per head workgroup): one class more than the
# threads of a sample; exactly 16 and a full workgroup; fewer classes than threads and one sample into the second
# workgroup; several strides and three workgroups; the class limit; a single class.
TAIL_SHAPES = {'tuned': [(1, 1), (3, 2), (37, 10), (128, 16)],
               'gen': [(1, 17), (64, 16), (65, 15), (130, 100), (5, 1024), (9, 1)]}
TARGETS = ('onehot', 'real')
# evaluation heads: n images (all listed, or a list of about three quarters of them), n_cls per family
EV_N = (1, 64, 65)
EV_CLS = {'tuned': (2, 16), 'gen': (15, 17, 100)}
TIE_CLS = {'tuned': 10, 'gen': 40}               # (40: equal maxima on different threads of a sample, and on the same one)
# per row: (positions of the equal maxima of z, positions of the equal maxima of y)
TIES = {'tuned': [((3, 7), (7, 9)), ((0, 9), (0, 1)), ((2, 4, 8), (4, 8)), ((1, 5), (1, 5, 6)), ((6, 7, 9), (0, 6)), ((0, 1), (1, 2))],
        'gen': [((5, 37), (37, 38)), ((6, 37), (6, 22)), ((5, 21, 37), (21, 37)), ((0, 16), (0, 16, 32)), ((15, 31, 39), (15, 16)), ((7, 8), (8, 23))]}


def _margin(v):
    """Every row's maximum raised by 0.5: a top-two gap of at least 0.5 whatever the draw."""
    v[np.arange(len(v)), v.argmax(1)] += 0.5
    return v


def targets(rng, n, nc, target):
    if target == 'onehot':
        return np.eye(nc, dtype=np.float32)[rng.integers(0, nc, n)]
    return _margin(rng.standard_normal((n, nc))).astype(np.float32)          # regression: any float vector


def tail_input(family, n, nc, target):
    """(z [n, nc], y [n, nc], w_cerr [n]) float32 of an exit-tail case: logits N(0, 2^2) with the margin above, signed
    weights."""
    rng = np.random.default_rng([n, nc, TARGETS.index(target), family == 'gen'])
    z = _margin(rng.standard_normal((n, nc)) * 2).astype(np.float32)
    return z, targets(rng, n, nc, target), rng.standard_normal(n).astype(np.float32)


def sentinel_input(n=70, nc=3):
    """Rows whose outputs all lie in [-9, -2] (one -2 per row, the others below -3): in the linear form every one of them
    is below the probability sentinel -1."""
    rng = np.random.default_rng(77)
    z = (-3 - 6 * rng.random((n, nc))).astype(np.float32)
    z[np.arange(n), rng.integers(0, nc, n)] = -2.0
    return z, targets(rng, n, nc, 'onehot'), rng.standard_normal(n).astype(np.float32)


def tie_input(family):
    """Rows with two or three exactly equal maxima in z (hence in softmax(z)) and in y, at different positions."""
    nc, rows = TIE_CLS[family], TIES[family]
    rng = np.random.default_rng(nc)
    z = np.minimum(rng.standard_normal((len(rows), nc)), 1.5).astype(np.float32)
    y = np.minimum(rng.standard_normal((len(rows), nc)), 1.0).astype(np.float32)
    for r, (pz, py) in enumerate(rows):
        z[r, list(pz)] = 3.0
        y[r, list(py)] = 2.0
    return z, y, rng.standard_normal(len(rows)).astype(np.float32)


# the squared records of the mixed tables (beside them: a cross-entropy record with a router, from tests/exit_ref.py)
MIXED_CLS = {'tuned': 10, 'gen': 100}
MIXED_N = 45                                     # n_max of the tables


def mixed_cases(family):
    """[(id, family, form, inputs)]: the MPNN_LOSS_SQ and the MPNN_LOSS_SQ_LIN record of the family's mixed table."""
    nc = MIXED_CLS[family]
    return [('%s-sq-mixed' % family, family, 'sq', tail_input(family, 29, nc, 'real')),
            ('%s-lin-mixed' % family, family, 'lin', tail_input(family, MIXED_N, nc, 'onehot'))]


def tail_cases():
    """(id, family, form, inputs) of every exit-tail head case: the shapes in both forms with both kinds of target, the
    ties, the sentinel rows, the squared records of the mixed tables."""
    out = []
    for family, shapes in TAIL_SHAPES.items():
        for form in FORMS:
            for n, nc in shapes:
                for target in TARGETS:
                    out.append(('%s-%s-n%d-c%d-%s' % (family, form, n, nc, target), family, form, tail_input(family, n, nc, target)))
            out.append(('%s-%s-ties' % (family, form), family, form, tie_input(family)))
            out.append(('%s-%s-sentinel' % (family, form), family, form, sentinel_input()))
        out += mixed_cases(family)
    return out


def no_tie_rows(case_id, z):
    """Rows of a case that carry no exact tie (all of them, but for the 'ties' cases)."""
    return np.zeros(len(z), bool) if case_id.endswith('ties') else np.ones(len(z), bool)


# ---- evaluation heads: the record's logits come out of its own affine map (tests/test_predict_kernels.py: Exit) --------
EV_GEOM = {'tuned': (16, 16), 'gen': (16, 32)}   # (HW, C) of the coarsest scale: K = 256 and 512


def ev_cases():
    """(family, n_cls) of the evaluation tests; each runs N in EV_N with every image and with a list, both targets."""
    return [(family, nc) for family, ncs in EV_CLS.items() for nc in ncs]


def ev_input(family, nc, N, kind='plain', target='onehot'):
    """The inputs of one evaluation record, numpy only: seed (tests/test_predict_kernels.py's Exit draws x and the
    BatchNorm of the scale from it, in this order), x, g, be, ma, va, the head wh [K, nc] / bh [nc], the targets y.
    kind 'plain': logits of a few units' spread; 'sentinel': every logit in about [-8, -3] (bias -5.5, a spread below 1);
    'ties': the columns TIES[family][0][0] identical and far above the rest, y tied at TIES[family][0][1]."""
    HW, C_ = EV_GEOM[family]
    K = HW * C_
    seed = 1000 * nc + N + {'plain': 0, 'sentinel': 300, 'ties': 600}[kind]
    rng = np.random.default_rng(seed)
    f = np.float32
    d = dict(seed=seed, N=N, HW=HW, C_=C_, K=K, nc=nc, x=rng.standard_normal((N, HW, C_)).astype(f),
             g=(rng.random(C_) + 0.5).astype(f), be=(rng.standard_normal(C_) * 0.2).astype(f),
             ma=(rng.standard_normal(C_) * 0.2).astype(f), va=(rng.random(C_) + 0.5).astype(f))
    r2 = np.random.default_rng(seed + 1)
    if kind == 'sentinel':
        wh, bh = r2.standard_normal((K, nc)) / np.sqrt(K) * 0.5, np.full(nc, -5.5)
    else:
        wh, bh = r2.standard_normal((K, nc)) / np.sqrt(K) * 4, r2.standard_normal(nc)
    y = targets(r2, N, nc, target)
    if kind == 'ties':
        pz, py = TIES[family][0]
        wh[:, pz[1]] = wh[:, pz[0]]
        bh[list(pz)] = 50.0
        y = np.minimum(y, 1.0).astype(f)
        y[:, list(py)] = 2.0
    d.update(wh=wh.astype(f), bh=bh.astype(f), y=y.astype(f))
    return d


def ev_logits(d, dt=F64):
    """z [N, nc] of an evaluation record: relu(bn(x)) @ wh + bh, in float64 or (dt=np.float32) in numpy float32."""
    x = d['x'].astype(dt)
    a = np.maximum(d['g'].astype(dt) * (x - d['ma'].astype(dt)) / np.sqrt(d['va'].astype(dt) + dt(1e-6)) + d['be'].astype(dt), 0)
    return a.reshape(d['N'], d['K']) @ d['wh'].astype(dt) + d['bh'].astype(dt)


def ev_all_inputs():
    """(id, form, inputs, exact ties) of every evaluation head input the GPU tests launch."""
    out = []
    for family, nc in ev_cases():
        for N in EV_N:
            for target in TARGETS:
                d = ev_input(family, nc, N, 'plain', target)
                out += [('%s-c%d-n%d-%s-%s' % (family, nc, N, target, form), form, d, False) for form in FORMS]
    for family in EV_CLS:
        out.append(('%s-sentinel' % family, 'lin', ev_input(family, 3, 65, 'sentinel'), False))
        out += [('%s-ties-%s' % (family, form), form, ev_input(family, TIE_CLS[family], 65, 'ties'), True) for form in FORMS]
    return out
