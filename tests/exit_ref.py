"""Plain numpy reference of the exit path, written out term by term, with the case tables and input draws its CPU and
GPU tests share: the any-width kernels (csrc/exit_gen.hip; tests/test_exit_gen_kernels.py: LIN_CASES, TAIL_CASES) and
the tuned ones (csrc/lin.hip, exit_tail.hip, exit_ev.hip; tests/test_exit_tuned_kernels.py: the TUNED_* tables);
tests/test_exit_ref_cpu.py checks the reference and the tables without a GPU.

Every function takes `dt` (float64: the reference; float32: the same arithmetic at the kernels' precision, used only
to MEASURE how far a correct fp32 evaluation lies from the reference).  Every value that is a sum comes with `bound`,
the sum of the absolute values of its own terms (what tests/test_conv_gen.py::_close calls `bound`): a tolerance is a
multiple of it, element by element.

  lin_fwd / lin_bwd      y[s] = a @ w[s][:K] + b[s] (+ alpha k_cpt w[s][K]),  dW[s], db[s], dx;  a = act(x) flattened
  tail_fwd               softmax, cross-entropy, d_cor, BatchNorm 1, h2, BatchNorm 2, r, bn_save, moving averages
  lin_fused              the tuned backward's fused form: masked dx and the BatchNorm-backward reductions
  tail_bwd               dz, dh2, dh1 and the eight parameter gradients from h1, h2 and the SAVED statistics, by the
                         formulas in the header comment of exit_tail_bwd_gen_k (no autograd)
  REGIMES, _trained      the same records as a TRAINED net fills them (tail_inputs / lin_inputs, `regime=`), with what the
                         GPU file tests/test_exit_trained_regime.py needs to judge them: f32_errors / widened (which limits
                         a float32 evaluation can keep), ambiguous (which ReLU masks it can tell), bn2_given
  pivoted_stats_f32      the tuned kernels' one-pass BatchNorm statistics restated in float32, as they were and as shipped
"""
import numpy as np

F64 = np.float64
ALPHA_CPT = 1e7
K_CPT = (0.0, 1e-9, 6.4e-8)
MARGIN = 1e-4                    # least |pre-activation| of both router BatchNorms in the float64 reference


def log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


# ---------------------------------------------------------------------------------------------------- affine maps
def act(x, mode, gamma=None, beta=None, m_avg=None, v_avg=None, eps=1e-6, dt=F64):
    """relu(bn(x)) over the last axis (statistics over every other axis), or x itself ('identity')."""
    x = np.asarray(x, dt)
    if mode == 'identity':
        return x
    if mode == 'batch':
        f = x.reshape(-1, x.shape[-1])
        m = f.mean(0)
        v = ((f - m) ** 2).mean(0)
    else:
        m, v = np.asarray(m_avg, dt), np.asarray(v_avg, dt)
    return np.maximum(np.asarray(gamma, dt) * (x - m) / np.sqrt(v + dt(eps)) + np.asarray(beta, dt), 0)


def lin_fwd(a, w, b, extra, kc, alpha=ALPHA_CPT, dt=F64):
    """a [n, K], w [K (+1), M], b [M] -> (y, bound)."""
    a, w, b = np.asarray(a, dt), np.asarray(w, dt), np.asarray(b, dt)
    K = a.shape[1]
    y = a @ w[:K] + b
    bound = np.abs(a) @ np.abs(w[:K]) + np.abs(b)
    if extra:
        t = (dt(alpha) * np.asarray(kc, dt))[:, None] * w[K]
        y, bound = y + t, bound + np.abs(t)
    return y, bound


def lin_bwd(a, ws, dys, extras, kc, alpha=ALPHA_CPT, dt=F64):
    """ws / dys / extras: per weight set (None: absent).  Returns dict(dw=[..], db=[..], dx=) of (value, bound); dw[s]
    has the k_cpt row (K + 1 rows) exactly when extras[s]."""
    a = np.asarray(a, dt)
    n, K = a.shape
    out = dict(dw=[None, None], db=[None, None])
    dx, dxb = np.zeros((n, K), dt), np.zeros((n, K), dt)
    for s in range(2):
        if ws[s] is None:
            continue
        w, dy = np.asarray(ws[s], dt), np.asarray(dys[s], dt)
        ext = np.concatenate([a, (dt(alpha) * np.asarray(kc, dt))[:, None]], 1) if extras[s] else a
        out['dw'][s] = (ext.T @ dy, np.abs(ext).T @ np.abs(dy))
        out['db'][s] = (dy.sum(0), np.abs(dy).sum(0))
        dx = dx + dy @ w[:K].T
        dxb = dxb + np.abs(dy) @ np.abs(w[:K]).T
    out['dx'] = (dx, dxb)
    return out


# (n, HW, C, act mode, M0 (head; 0: w[0] NULL), M1 (router; 0: w[1] NULL), extra_col)
LIN_CASES = [
    (5, 1, 3, 'identity', 2, 1, ''),            # K = 3 < 16; the channel wraps inside one 4-feature operand
    (17, 5, 3, 'batch', 17, 33, 'r'),           # K = 15 ragged; a second row tile of one row; ragged column tiles in both sets
    (1, 16, 16, 'batch', 10, 16, 'r'),          # batch of one
    (16, 4, 24, 'moving', 0, 40, ''),           # no head
    (33, 16, 16, 'batch', 10, 0, ''),           # no router
    (37, 16, 32, 'batch', 100, 32, 'r'),        # the 100-class shape
    (129, 4, 16, 'batch', 130, 256, 'hr'),      # four 128-column chunks of dx (the last 2 wide), chunk 2 across the head/router
                                                # boundary; nine row tiles for four waves
    (5, 257, 16, 'batch', 16, 16, ''),          # K = 4112
    (200, 1, 256, 'batch', 1024, 16, 'r'),      # both width limits: 64 column tiles, eight passes of 8 in the dW loop
]
LIN_MULTI = [(5, 4, 24, 'moving', 0, 40, ''), (37, 16, 32, 'batch', 100, 32, 'r'), (129, 1, 16, 'batch', 130, 0, 'h')]


def lin_inputs(case, seed=None, regime=None):
    """fp32 inputs of one affine-map record.  w[s] always has K + 1 rows; the last is NaN without extra_col[s] (a kernel
    that read it would show), as is k_cpt when no set has the column.  regime: None (the draws as they always were) or
    'trained' (REGIMES below), which rewrites the drawn dict from the same rng."""
    n, HW, C_, mode, M0, M1, ex = case
    rng = np.random.default_rng(sum(case[:3]) + M0 + M1 if seed is None else seed)
    f = np.float32
    K = HW * C_
    d = dict(n=n, HW=HW, C=C_, K=K, mode=mode, M=(M0, M1), extra=('h' in ex, 'r' in ex))
    d['x'] = rng.standard_normal((n, HW, C_)).astype(f)
    d['gamma'], d['beta'] = (rng.random(C_) + 0.5).astype(f), (rng.standard_normal(C_) * 0.2).astype(f)
    d['m_avg'], d['v_avg'] = (rng.standard_normal(C_) * 0.2).astype(f), (rng.random(C_) + 0.5).astype(f)
    d['kc'] = rng.choice(K_CPT, n).astype(f) if ex else np.full(n, np.nan, f)
    d['w'], d['b'], d['dy'] = [None, None], [None, None], [None, None]
    for s, M in enumerate((M0, M1)):
        if M:
            w = (rng.standard_normal((K + 1, M)) / np.sqrt(K)).astype(f)
            if not d['extra'][s]:
                w[K] = np.nan
            d['w'][s], d['b'][s] = w, rng.standard_normal(M).astype(f)
            d['dy'][s] = rng.standard_normal((n, M)).astype(f)
    if regime is not None:
        assert regime == 'trained', regime
        _trained(d, rng)
    return d


def _trained(d, rng):
    """The affine maps' inputs a few thousand steps in: per-channel scales of x log-uniform in [1e-2, 1e2], v_avg
    log-uniform in [1e-6, 1e2], gamma of both signs; beta puts 70 % of every channel's pre-activations below zero (minus
    the 0.7 quantile of gamma xhat, from float64), but channel 0 is off everywhere -- a zero column of a, so its dW rows
    are exactly 0 -- and channel 1 on everywhere.  k_cpt stays as drawn."""
    if d['mode'] == 'identity':
        return
    f, C_ = np.float32, d['C']
    d['x'] = (d['x'] * log_uniform(rng, 1e-2, 1e2, C_)).astype(f)
    d['v_avg'] = log_uniform(rng, 1e-6, 1e2, C_).astype(f)
    d['gamma'] = (d['gamma'] * rng.choice([-1.0, 1.0], C_)).astype(f)
    x = np.asarray(d['x'], F64).reshape(-1, C_)
    if d['mode'] == 'batch':
        m, v = x.mean(0), ((x - x.mean(0)) ** 2).mean(0)
    else:
        m, v = np.asarray(d['m_avg'], F64), np.asarray(d['v_avg'], F64)
    t = np.asarray(d['gamma'], F64) * (x - m) / np.sqrt(v + 1e-6)
    beta = -np.quantile(t, 0.7, axis=0)
    top = np.abs(t).max(0)
    beta[0] = -(top[0] + 1)
    if C_ > 1:
        beta[1] = top[1] + 1
    d['beta'] = beta.astype(f)


def lin_ref(d, dt=F64):
    """dict(y=[(v, bound)] * 2, dw=, db=, dx=) of one record's inputs."""
    a = act(d['x'], d['mode'], d['gamma'], d['beta'], d['m_avg'], d['v_avg'], dt=dt).reshape(d['n'], d['K'])
    out = lin_bwd(a, d['w'], d['dy'], d['extra'], d['kc'], dt=dt)
    out['y'] = [None if d['w'][s] is None else lin_fwd(a, d['w'][s], d['b'][s], d['extra'][s], d['kc'], dt=dt) for s in range(2)]
    return out


# The tuned affine maps (csrc/lin.hip; tests/test_exit_tuned_kernels.py).  Same tuple format; every case lies inside
# the engine's tuned domain (C <= 128 in multiples of 16, K = HW C a multiple of 16, both widths <= 16).
TUNED_LIN_CASES = [
    (5, 1, 16, 'identity', 2, 1, ''),           # K = 16: one block; a 64-feature block with 16 live lanes
    (17, 15, 48, 'batch', 16, 5, 'r'),          # K = 720: two K-slices of 22 / 23 blocks; the C = 48 wrap of the fused reduction;
                                                # K % 64 = 16 with the k_cpt row inside the last block; a second row tile of one row
    (33, 3, 80, 'moving', 10, 0, ''),           # no router; C = 80; K = 240
    (1, 16, 16, 'batch', 10, 16, 'r'),          # batch of one; K % 64 == 0: the k_cpt row is a feature block of its own
    (37, 7, 112, 'batch', 0, 16, 'r'),          # no head; K = 784: three slices of 16 / 16 / 17
    (130, 6, 96, 'batch', 16, 16, 'hr'),        # both widths at their limit, the extra column on both; three row groups, the last ragged
    (9, 13, 112, 'batch', 10, 16, 'r'),         # K = 1456: five slices of 18 / 18 / 18 / 18 / 19
    (200, 4, 128, 'batch', 10, 16, ''),         # the C limit; two 128-row supers unsplit; four row groups, the last of one pass
    (520, 1, 32, 'batch', 3, 8, 'r'),           # n > 512: gridDim.z capped at 8 and Z = 7 < 8; five supers unsplit
]
TUNED_LIN_MULTI = [TUNED_LIN_CASES[k] for k in (0, 2, 4, 5)]        # n_max = 130, k_max = 784
NEAR = 1e-5                      # |float64 pre-activation| below which a fused dz may be masked either way


def lin_fused(d, ref, dt=F64):
    """The fused form of the tuned backward (dx == NULL; batch mode): dz = dx where relu(bn(x)) is on, and the
    BatchNorm-backward reductions [sum dz, sum dz xhat] per channel.  Returns dict(pre, xh, on [n, K], dx, dz (value,
    bound))."""
    n, K, C_ = d['n'], d['K'], d['C']
    x = np.asarray(d['x'], dt)
    f = x.reshape(-1, C_)
    m = f.mean(0)
    v = ((f - m) ** 2).mean(0)
    xh = (x - m) / np.sqrt(v + dt(1e-6))
    pre = (np.asarray(d['gamma'], dt) * xh + np.asarray(d['beta'], dt)).reshape(n, K)
    dx, dxb = ref['dx']
    on = pre > 0
    return dict(pre=pre, xh=xh.reshape(n, K), on=on, dx=dx, dxb=dxb, dz=(on * dx, on * dxb))


def fused_red(fz, on, C_):
    """[sum dz, sum dz xhat] over rows and pixels, per channel, for the mask `on`: (value [2C], bound)."""
    t = [on * fz['dx'], on * fz['dx'] * fz['xh']]
    b = [on * fz['dxb'], on * fz['dxb'] * np.abs(fz['xh'])]
    s = lambda a: a.reshape(-1, C_).sum(0)
    return np.concatenate([s(t[0]), s(t[1])]), np.concatenate([s(b[0]), s(b[1])])


def dz_resolve(got, fz):
    """The mask the comparison of a fused dz uses: the reference's, except where |pre| < NEAR -- there whichever of 0 and
    that element's dx lies nearer to `got`.  Returns (mask, share of such elements)."""
    near = np.abs(fz['pre']) < NEAR
    take = np.abs(np.asarray(got, F64) - fz['dx']) < np.abs(np.asarray(got, F64))
    return np.where(near, take, fz['on']), float(near.mean())


# ---------------------------------------------------------------------------------------------------- exit tail
def head_fwd(z, y, eps_ce, dt=F64):
    z, y = np.asarray(z, dt), np.asarray(y, dt)
    nc = z.shape[1]
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    q = dt(eps_ce) / nc + (1 - dt(eps_ce)) * p
    top = np.sort(p, 1)
    gap = top[:, -1] - top[:, -2] if nc > 1 else np.ones(len(z), dt)
    return dict(p=p, q=q, c_err=-(y * np.log(q)).sum(1), d_cor=(p.argmax(1) == y.argmax(1)).astype(dt), gap=gap)


def tail_fwd(d, dt=F64):
    """Forward of one exit-tail record `d` (tail_inputs).  Router values: m1, v1, s1 (= rstd), pre1 (the BatchNorm output
    ahead of the ReLU), h2 (+ h2_bound), m2, v2, s2, pre2, r (+ r_bound), bn_save, and the moving averages after the
    update ('avg': m1, v1, m2, v2; unchanged in 'moving' mode)."""
    A = lambda k: np.asarray(d[k], dt)
    out = {}
    if d['head']:
        out.update(head_fwd(d['z'], d['y'], d['eps_ce'], dt))
    if not d['router']:
        return out
    h1 = A('h1')

    def stats(x, k, dec):
        if d['mode'] == 'batch':
            m = x.mean(0)
            v = ((x - m) ** 2).mean(0)
            avg = [dt(dec) * A('m' + k) + (1 - dt(dec)) * m, dt(dec) * A('v' + k) + (1 - dt(dec)) * v]
        else:
            m, v = A('m' + k), A('v' + k)
            avg = [m, v]
        return m, v, avg
    m1, v1, avg1 = stats(h1, '1', d['bn_decay'])
    s1 = 1 / np.sqrt(v1 + dt(d['bn_eps']))
    pre1 = A('g1') * ((h1 - m1) * s1) + A('b1')
    a1 = np.maximum(pre1, 0)
    h2 = a1 @ A('w2') + A('bias2')
    m2, v2, avg2 = stats(h2, '2', d['bn_decay2'])
    s2 = 1 / np.sqrt(v2 + dt(d['bn_eps2']))
    pre2 = A('g2') * ((h2 - m2) * s2) + A('b2')
    a2 = np.maximum(pre2, 0)
    r = a2 @ A('w3') + A('bias3')
    out.update(m1=m1, v1=v1, s1=s1, pre1=pre1, h2=h2, h2_bound=np.abs(a1) @ np.abs(A('w2')) + np.abs(A('bias2')),
               m2=m2, v2=v2, s2=s2, pre2=pre2, r=r, r_bound=np.abs(a2) @ np.abs(A('w3')) + np.abs(A('bias3')),
               bn_save=np.concatenate([m1, s1, m2, s2]), avg=avg1 + avg2)
    return out


def bn_bwd(dy, dyb, xh, g, s, n):
    """dh = g rstd (dy - mean(dy) - xh mean(dy xh)) with its bound; also (dbeta, bound), (dgamma, bound)."""
    db, dbb = dy.sum(0), dyb.sum(0)
    dg, dgb = (dy * xh).sum(0), (dyb * np.abs(xh)).sum(0)
    dh = g * s * (dy - db / n - xh * (dg / n))
    dhb = np.abs(g * s) * (dyb + dbb / n + np.abs(xh) * (dgb / n))
    return (dh, dhb), (db, dbb), (dg, dgb)


def tail_bwd(d, h2, save, dt=F64, on=None):
    """Backward of the same from h1, h2 and the saved statistics save = (m1, rstd1, m2, rstd2), as the kernel runs it.
    Returns name -> (value, bound) for dz, dh2, dh1, dg1, db1, dw2, dbias2, dg2, db2, dw3, dbias3.  on: the two ReLU
    masks to differentiate through instead of the reference's own (where they are ambiguous: `ambiguous`)."""
    A = lambda k: np.asarray(d[k], dt)
    n = d['n']
    out = {}
    if d['head']:
        f = head_fwd(d['z'], d['y'], d['eps_ce'], dt)
        p, q = f['p'], f['q']
        t = -A('w_cerr')[:, None] * A('y') * (1 - dt(d['eps_ce'])) / q          # dL/dp[k]
        dot = (t * p).sum(1, keepdims=True)
        out['dz'] = (p * (t - dot), p * (np.abs(t) + (np.abs(t) * p).sum(1, keepdims=True)))
    if not d['router']:
        return out
    m1, s1, m2, s2 = (np.asarray(v, dt) for v in save)
    h1, h2, dr = A('h1'), np.asarray(h2, dt), A('dr')
    g1, b1, w2, g2, b2, w3 = A('g1'), A('b1'), A('w2'), A('g2'), A('b2'), A('w3')
    xh2 = (h2 - m2) * s2
    pre2 = g2 * xh2 + b2
    a2, on2 = np.maximum(pre2, 0), pre2 > 0 if on is None else on[1]
    dy2, dy2b = on2 * (dr @ w3.T), on2 * (np.abs(dr) @ np.abs(w3).T)
    out['dw3'] = (a2.T @ dr, np.abs(a2).T @ np.abs(dr))
    out['dbias3'] = (dr.sum(0), np.abs(dr).sum(0))
    out['dh2'], out['db2'], out['dg2'] = bn_bwd(dy2, dy2b, xh2, g2, s2, n)
    dh2, dh2b = out['dh2']
    out['dbias2'] = (dh2.sum(0), dh2b.sum(0))
    xh1 = (h1 - m1) * s1
    pre1 = g1 * xh1 + b1
    a1, on1 = np.maximum(pre1, 0), pre1 > 0 if on is None else on[0]
    out['dw2'] = (a1.T @ dh2, np.abs(a1).T @ dh2b)
    dy1, dy1b = on1 * (dh2 @ w2.T), on1 * (dh2b @ np.abs(w2).T)
    out['dh1'], out['db1'], out['dg1'] = bn_bwd(dy1, dy1b, xh1, g1, s1, n)
    return out


def masks(d, h2, save, dt=F64):
    """The two ReLU masks from h1, h2 and saved statistics (the device's own, on the GPU)."""
    m1, s1, m2, s2 = (np.asarray(v, dt) for v in save)
    A = lambda k: np.asarray(d[k], dt)
    return (A('g1') * ((A('h1') - m1) * s1) + A('b1') > 0, A('g2') * ((np.asarray(h2, dt) - m2) * s2) + A('b2') > 0)


def split_save(save, R, R2):
    return save[:R], save[R:2 * R], save[2 * R:2 * R + R2], save[2 * R + R2:]


def min_margin(d):
    f = tail_fwd(d)
    return min(float(np.abs(f['pre1']).min()), float(np.abs(f['pre2']).min()))


# name: dict(n, nc, R, R2, S, stride, seed, [head, router, mode, eps_ce]).  `seed` is the first for which every
# pre-activation of both router BatchNorms lies at least MARGIN from zero in float64 (tests/test_exit_ref_cpu.py asserts
# it; scan_seed finds one).  n = 2 is left out on purpose: its statistics amplify rounding by 1 / sqrt(eps).
TAIL_CASES = {
    'one':        dict(n=1, nc=5, R=5, R2=3, S=2, stride=4, seed=0),        # zero variance: dh1, dh2 analytically zero
    'unit':       dict(n=5, nc=2, R=1, R2=7, S=2, stride=2, seed=0, eps_ce=0.1),       # one-unit layer; r_stride == n_sinks
    'class17':    dict(n=37, nc=17, R=24, R2=40, S=3, stride=4, seed=0, eps_ce=0.1),   # a 17th class: second pass of a sample's threads
    'limits':     dict(n=40, nc=1000, R=256, R2=256, S=4, stride=4, seed=1),           # row chunks of 16 (last ragged), w2 from global memory
    'w2lds':      dict(n=64, nc=10, R=90, R2=90, S=2, stride=4, seed=4),               # R (R2 + 1) = 8190: w2 through LDS
    'w2glob':     dict(n=64, nc=10, R=91, R2=90, S=2, stride=4, seed=5),               # 8281: just past that switch
    'ship129':    dict(n=129, nc=10, R=16, R2=16, S=2, stride=4, seed=0),              # the shipped exits above 128
    'ship300':    dict(n=300, nc=10, R=16, R2=16, S=2, stride=4, seed=0),
    'rows1100':   dict(n=1100, nc=3, R=8, R2=8, S=2, stride=4, seed=1, eps_ce=0.1),    # more rows than threads; 18 head workgroups
    'odd':        dict(n=200, nc=37, R=33, R2=17, S=3, stride=4, seed=1),
    'headonly':   dict(n=70, nc=12, R=0, R2=0, S=0, stride=4, seed=0, router=False),
    'routeronly': dict(n=70, nc=0, R=20, R2=12, S=3, stride=4, seed=0, head=False),
    'moving':     dict(n=45, nc=10, R=24, R2=20, S=2, stride=4, seed=1, mode='moving'),
    'table0':     dict(n=37, nc=10, R=16, R2=24, S=2, stride=4, seed=0),               # records of the two-record table
    'table1':     dict(n=129, nc=20, R=32, R2=16, S=3, stride=4, seed=0),
}
# The tuned exit tail (csrc/exit_tail.hip: R2 == R <= 16, <= 16 classes, <= 4 sinks); a table of its own, since a case's
# draw depends on its position in its table.  ship129, ship300, rows1100 and headonly above lie inside these limits too.
TUNED_TAIL_CASES = {
    't_one':        dict(n=1, nc=2, R=1, R2=1, S=2, stride=4, seed=0),      # zero variance: dh1 analytically zero
    't_r5':         dict(n=37, nc=16, R=5, R2=5, S=3, stride=4, seed=0),    # eleven inert padding channels; the class limit
    't_full':       dict(n=128, nc=10, R=16, R2=16, S=4, stride=4, seed=2), # every limit of the LDS-resident kernels
    't_stride':     dict(n=64, nc=3, R=12, R2=12, S=2, stride=2, seed=0),   # r_stride == n_sinks
    't_router':     dict(n=70, nc=0, R=12, R2=12, S=2, stride=4, seed=1, head=False),
    't_head':       dict(n=70, nc=16, R=0, R2=0, S=0, stride=4, seed=0, router=False),
    't_moving':     dict(n=45, nc=10, R=16, R2=16, S=2, stride=4, seed=0, mode='moving'),
    't_moving_big': dict(n=200, nc=10, R=8, R2=8, S=2, stride=4, seed=0, mode='moving'),
    't_r3_big':     dict(n=300, nc=16, R=3, R2=3, S=4, stride=4, seed=0),
}
# Cases only the trained-net regimes run (tests/test_exit_trained_regime.py); a table of its own again, so that no
# existing draw moves.  Inside both kernel families' domains.
REGIME_TAIL_CASES = {
    't_r8_1100':    dict(n=1100, nc=3, R=8, R2=8, S=2, stride=4, seed=0, eps_ce=0.1),  # more rows than threads in router_fwd_big
}
EPS = (1e-6, 1e-3)               # the two router BatchNorms never share an epsilon or a decay (alternating by case)
DECAY = (0.9, 0.99)


# The tuned evaluation exit (mpnn_exit_ev): name -> (seed, N, count, HW, C, nc, R (= R2), S, dyn, head, router, sinks
# with a list).  ev_c20: mpnn_exit_ev_check admits C % 4 == 0; the engine sends multiples of 16 only.
TUNED_EV_CASES = {
    'ev_c48':      (21, 70, 41, 15, 48, 16, 5, 3, True, True, True, (1, 2)),     # K / 16 = 45: the odd last block pair
    'ev_hw1':      (22, 37, 29, 1, 16, 2, 16, 2, False, True, True, (0, 1)),     # K = 16: one block, seven idle waves
    'ev_c20':      (23, 70, 41, 4, 20, 10, 12, 4, False, True, True, (0, 1, 3)),
    'ev_nohead':   (24, 70, 41, 3, 80, 10, 8, 3, True, False, True, (1, 2)),
    'ev_norouter': (25, 70, 41, 7, 112, 16, 16, 2, False, True, False, ()),
}


def tail_inputs(name, seed=None, table=None, regime=None):
    """fp32 inputs and hyper-parameters of one exit-tail record of `table` (None: TAIL_CASES).  regime: None (the draws
    as they always were) or names of REGIMES joined by '+', applied in that order to the drawn dict from the same rng;
    its seed is REGIME_SEEDS[name, regime] unless given."""
    table = TAIL_CASES if table is None else table
    c = dict(head=True, router=True, mode='batch', eps_ce=1e-6)
    c.update(table[name])
    if regime is not None:
        c['seed'] = REGIME_SEEDS.get((name, regime), 0)
    if seed is not None:
        c['seed'] = seed
    k = sorted(table).index(name)
    rng = np.random.default_rng([k, c['seed']])
    f = np.float32
    n, nc, R, R2, S = c['n'], c['nc'], c['R'], c['R2'], c['S']
    d = dict(c, name=name)
    d['bn_eps'], d['bn_eps2'] = EPS[k % 2], EPS[1 - k % 2]
    d['bn_decay'], d['bn_decay2'] = DECAY[(k // 2) % 2], DECAY[1 - (k // 2) % 2]
    if c['head']:
        d['z'] = (rng.standard_normal((n, nc)) * 2).astype(f)
        d['y'] = np.eye(nc, dtype=f)[rng.integers(0, nc, n)]
        d['w_cerr'] = rng.random(n).astype(f)
    if c['router']:
        d['h1'] = rng.standard_normal((n, R)).astype(f)
        d['g1'], d['b1'] = (rng.random(R) + 0.5).astype(f), (rng.standard_normal(R) * 0.3).astype(f)
        d['w2'], d['bias2'] = (rng.standard_normal((R, R2)) / np.sqrt(R)).astype(f), (rng.standard_normal(R2) * 0.1).astype(f)
        d['g2'], d['b2'] = (rng.random(R2) + 0.5).astype(f), (rng.standard_normal(R2) * 0.3).astype(f)
        d['w3'], d['bias3'] = (rng.standard_normal((R2, S)) / np.sqrt(R2)).astype(f), (rng.standard_normal(S) * 0.1).astype(f)
        d['m1'], d['v1'] = (rng.standard_normal(R) * 0.1).astype(f), (rng.random(R) + 0.5).astype(f)
        d['m2'], d['v2'] = (rng.standard_normal(R2) * 0.1).astype(f), (rng.random(R2) + 0.5).astype(f)
        d['dr'] = rng.standard_normal((n, S)).astype(f)
    if regime is not None:
        d['regime'] = regime
        for k in regime.split('+'):
            REGIMES[k](d, rng)
    return d


# ---------------------------------------------------------------------------------------------------- trained-net regimes
# The draws above are a net at initialisation.  Each function below rewrites the drawn dict, from the same rng, into what
# one part of a record looks like a few thousand steps in (tests/test_exit_trained_regime.py; properties asserted on the
# CPU: tests/test_exit_ref_cpu.py).  All values stay fp32; the reference is evaluated on the rounded values.
def _confident(d, rng, offset=False):
    """Head.  One logit of every row raised by U(10, 40): the label's, in 5 % of the rows (and in row 4) another class's
    -- confidently wrong.  Row 1 has a logit 120 below its maximum: that p is exactly 0 in fp32 (exp(-104) is below the
    least denormal), q = eps_ce / nc.  Rows 2 and 3 tie their top two logits bitwise, the label the first of the two in
    row 2 and the second in row 3: arg-max is the first index on both sides.  Of the rows from 5 on a quarter carry
    w_cerr = 0 (routed away), three 1e-8, one 1.  offset: a common +-1e4 per row on top, rounded to fp32 with the row.
    eps_ce = 0 stays out: 0 log 0 is NaN in the reference too."""
    if not d['head']:
        return
    n, nc, f = d['n'], d['nc'], np.float32
    assert n >= 16 and nc >= 2 and d['eps_ce'] > 0
    z, y, ar = d['z'].astype(F64), d['y'].copy(), np.arange(n)
    lab = y.argmax(1)
    wrong = rng.random(n) < 0.05
    wrong[4] = True
    tgt = np.where(wrong, (lab + rng.integers(1, nc, n)) % nc, lab)
    z[ar, tgt] += rng.uniform(10, 40, n)
    z[1, (z[1].argmax() + 1) % nc] = z[1].max() - 120
    for row, first in ((2, True), (3, False)):
        a, b = np.sort(rng.choice(nc, 2, replace=False))
        z[row, a] = z[row, b] = z[row].max() + 5
        y[row] = np.eye(nc, dtype=f)[a if first else b]
    w = d['w_cerr'].copy()
    rest = 5 + rng.permutation(n - 5)
    w[rest[:n // 4]], w[rest[n // 4:n // 4 + 3]], w[rest[n // 4 + 3]] = 0.0, 1e-8, 1.0
    if offset:
        z = z.astype(f).astype(F64) + rng.choice([-1e4, 1e4], n)[:, None]
    d['z'], d['y'], d['w_cerr'] = z.astype(f), y, w.astype(f)


def _offset(d, rng):
    _confident(d, rng, offset=True)


def _shifted(d, rng, mu=50.0, sigma=(1e-3, 10.0), pivot=False):
    """Router.  h1 = mu_c + sigma_c N(0, 1) per channel, mu_c in U(-50, 50), sigma_c log-uniform in [1e-3, 10]; w2 and w3
    times 8, so r spans tens of units.  pivot: sigma_c in [1e-2, 1], |mu_c| <= 5, and row 0 -- the row the tuned kernels
    once pivoted their one-pass sums on -- at mu_c +- k_c sigma_c, k_c = 6, 30, 100 cycling over the channels; the h2 row
    of sample 0 is then extreme as well."""
    if not d['router']:
        return
    n, R, f = d['n'], d['R'], np.float32
    m, s = rng.uniform(-mu, mu, R), log_uniform(rng, sigma[0], sigma[1], R)
    h = m + s * rng.standard_normal((n, R))
    if pivot:
        h[0] = m + rng.choice([-1.0, 1.0], R) * np.array([6.0, 30.0, 100.0])[np.arange(R) % 3] * s
    d['h1'], d['w2'], d['w3'] = h.astype(f), d['w2'] * f(8), d['w3'] * f(8)


def _pivot(d, rng):
    _shifted(d, rng, 5.0, (1e-2, 1.0), True)


def _bn64(x, m, v, eps):
    return (x - m) / np.sqrt(v + eps)


def _stats64(d, x, k):
    if d['mode'] == 'batch':
        m = x.mean(0)
        return m, ((x - m) ** 2).mean(0)
    return d['m' + k].astype(F64), d['v' + k].astype(F64)


def _scales(g):
    """BatchNorm scales of a trained net on channels 2, 3, 4 (as far as they exist): 1e-4, 20, negative."""
    g = g.copy()
    for c, v in ((2, 1e-4), (3, 20.0)):
        if c < len(g):
            g[c] = v
    if len(g) > 4:
        g[4] = -g[4]
    return g


def _dead(d, rng):
    """Router, both BatchNorms, channel by channel as far as the width goes: 0 exactly constant (variance 0; h2's by a
    zero column of w2) with beta < 0, a fully masked column; 1 with sigma = 1e-5 around 1, far below sqrt(eps); 2 with
    gamma = 1e-4 and beta > 0, a fully live column; 3 with gamma = 20; 4 with gamma < 0; 5 with beta so negative that
    every pre-activation is off (a dead unit); 6 with beta so positive that every one is on."""
    if not d['router']:
        return
    n, f = d['n'], np.float32
    for k, hk, g, b, eps in (('1', 'h1', 'g1', 'b1', d['bn_eps']), ('2', None, 'g2', 'b2', d['bn_eps2'])):
        W = len(d[g])
        if k == '1':
            d['h1'][:, 0] = d['h1'][0, 0]
            if W > 1:
                d['h1'][:, 1] = (1 + 1e-5 * rng.standard_normal(n)).astype(f)
        else:
            d['w2'][:, 0] = 0
        d[g] = _scales(d[g])
        d[b][0] = -abs(d[b][0]) - f(0.1)
        if W > 2:
            d[b][2] = abs(d[b][2]) + f(0.1)
        x = d['h1'].astype(F64) if k == '1' else tail_fwd(d)['h2']
        top = np.abs(d[g].astype(F64) * _bn64(x, *_stats64(d, x, k), eps)).max(0)
        if W > 5:
            d[b][5] = -(top[5] + 1)
        if W > 6:
            d[b][6] = top[6] + 1


def _moving(d, rng):
    """Router in evaluation mode: v_avg cycles through 0, 1e-8, 1e-3, 1, 1e4 over the channels, m_avg lies up to 30
    sqrt(v_avg) from the batch's mean, the scales as in `dead`."""
    if not d['router']:
        return
    f = np.float32
    for k, g in (('1', 'g1'), ('2', 'g2')):
        W = len(d[g])
        d[g] = _scales(d[g])
        v = np.array([0.0, 1e-8, 1e-3, 1.0, 1e4])[np.arange(W) % 5]
        x = d['h1'].astype(F64) if k == '1' else tail_fwd(d)['h2']
        d['v' + k], d['m' + k] = v.astype(f), (x.mean(0) + rng.uniform(-30, 30, W) * np.sqrt(v)).astype(f)


REGIMES = dict(confident=_confident, offset=_offset, shifted=_shifted, pivot=_pivot, dead=_dead, moving=_moving)
# (case, regime) of tests/test_exit_trained_regime.py: the tuned kernels', the any-width kernels', and the records both
# families run.  Every case is the smallest that reaches its code path: the LDS-resident kernel at its limit (t_full),
# padding channels beside degenerate ones (t_r5), router_fwd_big with fewer and with more rows than threads (t_r3_big,
# t_r8_1100), the moving averages in both tuned kernels, the head alone, n = 1 (every variance 0).
TUNED_REGIME_RUNS = [('t_full', 'confident+shifted'), ('t_full', 'offset+pivot'), ('t_full', 'confident+dead'), ('t_r5', 'pivot'),
                     ('t_r5', 'dead'), ('t_r3_big', 'pivot'), ('t_r8_1100', 'pivot'), ('t_r8_1100', 'shifted'), ('t_moving', 'moving'),
                     ('t_moving_big', 'moving'), ('t_head', 'confident'), ('t_head', 'offset'), ('t_one', 'dead')]
GEN_REGIME_RUNS = [(c, r) for c in ('class17', 'odd', 'ship300') for r in ('confident+pivot', 'offset+dead')] + [('moving', 'moving')]
BOTH_REGIME_RUNS = [('ship300', 'confident+pivot'), ('t_r8_1100', 'pivot')]
REGIME_RUNS = TUNED_REGIME_RUNS + GEN_REGIME_RUNS
# The first seed of each whose float64 pre-activations all lie at least MARGIN from zero and of whose ReLU-mask elements
# at most 0.1 % are ambiguous in fp32 (`ambiguous`); asserted on the CPU, found by scan_seed (python tests/exit_ref.py).
REGIME_SEEDS = {
    ('t_full', 'confident+shifted'): 9, ('t_full', 'offset+pivot'): 0, ('t_full', 'confident+dead'): 0, ('t_r5', 'pivot'): 0,
    ('t_r5', 'dead'): 0, ('t_r3_big', 'pivot'): 0, ('t_r8_1100', 'pivot'): 2, ('t_r8_1100', 'shifted'): 60,
    ('t_moving', 'moving'): 0, ('t_moving_big', 'moving'): 0, ('t_head', 'confident'): 0, ('t_head', 'offset'): 0,
    ('t_one', 'dead'): 0, ('class17', 'confident+pivot'): 0, ('class17', 'offset+dead'): 0, ('odd', 'confident+pivot'): 3,
    ('odd', 'offset+dead'): 2, ('ship300', 'confident+pivot'): 4, ('ship300', 'offset+dead'): 1, ('moving', 'moving'): 0,
}


def near_margin(d, f64=None):
    """Per channel, the distance from zero below which a pre-activation of each router BatchNorm is ambiguous in fp32: 5 x
    the worst error of the float32 evaluation of the reference (as written, and with the batch rows reversed), the
    inverse of the project's rule that a correct fp32 evaluation uses 0.2 of a limit.  Every seed keeps MARGIN, so it
    matters only where it exceeds MARGIN.  Returns (near1 [R], near2 [R2])."""
    f64 = tail_fwd(d) if f64 is None else f64
    out = []
    for k in ('pre1', 'pre2'):
        e = np.maximum(*[np.abs(np.asarray(f[k], F64) - f64[k]).max(0) for f in f32_evaluations(d)])
        out.append(5 * e)
    return out


def reverse_rows(d):
    r = dict(d)
    for k in ('z', 'y', 'w_cerr', 'h1', 'dr'):
        if k in d:
            r[k] = d[k][::-1].copy()
    return r


PER_ROW = ('p', 'q', 'c_err', 'd_cor', 'gap', 'pre1', 'h2', 'h2_bound', 'pre2', 'r', 'r_bound', 'dz', 'dh1', 'dh2')


def f32_evaluations(d, bwd=False, on=None):
    """tail_fwd (bwd: tail_bwd on its own h2 and statistics, values only, through the masks `on`) in float32 as written
    and with the batch rows reversed (another summation order), rows put back."""
    out = []
    for rev in (False, True):
        e = reverse_rows(d) if rev else d
        f = tail_fwd(e, np.float32)
        if bwd:
            g = tail_bwd(e, f.get('h2'), split_save(f['bn_save'], d['R'], d['R2']) if d['router'] else None, np.float32,
                         on if on is None or not rev else [m[::-1] for m in on])
            f = {k: v[0] for k, v in g.items()}
        out.append({k: (v[::-1] if rev and k in PER_ROW else v) for k, v in f.items()})
    return out


def bn2_given(d, h2, dt=F64):
    """The second BatchNorm's statistics of a GIVEN h2 [n, R2]: dict(bn_save2 = [m2, rstd2], m2, v2 = the moving averages
    after the update).  The GPU tests hold a kernel's second-BatchNorm statistics to these of ITS OWN h2 (and its h2 to
    the reference): what h2 inherits from an ill-conditioned first layer is then not charged to the statistics."""
    x, A = np.asarray(h2, dt), lambda k: np.asarray(d[k], dt)
    if d['mode'] == 'batch':
        m = x.mean(0)
        v = ((x - m) ** 2).mean(0)
        dec = dt(d['bn_decay2'])
        avg = [dec * A('m2') + (1 - dec) * m, dec * A('v2') + (1 - dec) * v]
    else:
        m, v = A('m2'), A('v2')
        avg = [m, v]
    return dict(bn_save2=np.concatenate([m, 1 / np.sqrt(v + dt(d['bn_eps2']))]), m2=avg[0], v2=avg[1])


def f32_errors(d, f64, g64=None, on=None):
    """quantity -> |float32 evaluation - reference| element by element, the larger of the two summation orders, for
    every quantity the GPU tests compare: c_err, h2, r, bn_save1 (= m1, rstd1), the moving averages m1, v1; bn_save2, m2,
    v2 as bn2_given computes them in both precisions from the float32 evaluation's h2; and, with g64 (tail_bwd's result
    for the masks `on`; None: the reference's own), every gradient.  The float32 backward goes through the same masks,
    so the figure is arithmetic error and never a flipped ReLU."""
    err = {}
    up = lambda k, a, b: err.__setitem__(k, np.maximum(err.get(k, 0), np.abs(np.asarray(a, F64) - b)))
    ev = f32_evaluations(d)
    for f in ev:
        for k in ('c_err', 'h2', 'r'):
            if k in f64:
                up(k, f[k], f64[k])
        if d['router']:
            up('bn_save1', f['bn_save'][:2 * d['R']], f64['bn_save'][:2 * d['R']])
            for k, a, b in zip(('m1', 'v1'), f['avg'], f64['avg']):
                up(k, a, b)
    if d['router']:
        h2, want = ev[0]['h2'], bn2_given(d, ev[0]['h2'])
        for got in (bn2_given(d, h2, np.float32), bn2_given(d, h2[::-1], np.float32)):
            for k in want:
                up(k, got[k], want[k])
    if g64 is not None:
        if on is None and d['router']:
            on = (f64['pre1'] > 0, f64['pre2'] > 0)
        for g in f32_evaluations(d, True, on):
            for k in g64:
                up(k, g[k], g64[k][0])
    return err


def widened(lim, err):
    """(the limit a quantity is held to in a trained-net regime, the float32 reference's worst error / existing limit, the
    floor the limit was raised to or 0).
    At most 0.2 (the rule tests/test_exit_ref_cpu.py asserts for the draws at initialisation): the existing limit `lim`,
    unchanged.  Above: the input is ill-conditioned for ANY fp32 evaluation, and the limit is max(lim, 5 x the float32
    reference's worst error) -- 5 being the inverse of that 0.2; from the reference alone, never from a kernel."""
    lim, err = np.broadcast_to(lim, np.shape(err)), np.asarray(err, F64)
    ratio = float((err / lim).max()) if err.size else 0.0
    return (lim if ratio <= 0.2 else np.maximum(lim, 5 * err.max())), ratio, (5 * float(err.max()) if ratio > 0.2 else 0.0)


def tail_table(name):
    """The table a tail case's name is from (None: TAIL_CASES)."""
    return next((t for t in (TUNED_TAIL_CASES, REGIME_TAIL_CASES) if name in t), None)


def ambiguous(d, f64=None):
    """(amb1 [n, R], amb2 [n, R2]): where a ReLU mask may fall either way (near_margin), and the share of such elements."""
    f64 = tail_fwd(d) if f64 is None else f64
    near = near_margin(d, f64)
    amb = [np.abs(f64[k]) < nr for k, nr in zip(('pre1', 'pre2'), near)]
    return amb, float(sum(a.sum() for a in amb)) / max(1, sum(a.size for a in amb))


def _tree(v):
    """Sum over axis 0 (a power of two long) as a binary tree of adjacent pairs, in v's own precision: the order of
    wave_sum_f's DPP steps and of block_sums' four wave partials."""
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return v[0]


REDO = 31.0                      # MPNN_BN_REDO of csrc/exit_tail.hip: (mean - pivot)^2 > REDO var, five bits lost, repeats the pass


def pivoted_stats_f32(h, n, eps, form='shipped'):
    """(mean, var, rstd) of h [n, W <= 16] as csrc/exit_tail.hip computes a router BatchNorm's batch statistics, restated
    from the kernel source in numpy float32: ONE pass of sums of d = x - pivot and d^2 (the square fused into its add, as
    the compiler contracts it) around the pivot row 0, dm = t1 inv, mean = pivot + dm, var = fma(-dm, dm, t2 inv), as the
    kernel writes the finish out with contraction off.
      n <= 128   bn_stats: thread (sub, c) adds rows sub, sub + 16, ... in order; 16 partials per channel added in order
      n >  128   router_fwd_big: thread t adds rows t, t + 256, ... in order; block_sums adds the 256 partials as a tree
    form 'row0': the form up to this file's arrival -- that pass alone.
    form 'shipped': where the pass finds (mean - pivot)^2 > REDO var in ANY channel -- the subtraction has then lost more
    than log2(1 + REDO) = 5 bits there -- the pass runs once more, for every channel, around the mean it found.
    The summation order is the kernel's; the contraction of the sweep's d * d is the compiler's choice."""
    f = np.float32
    h = np.asarray(h, f)[:n]
    T = 16 if n <= 128 else 256
    rows = -(-n // T) * T

    def one_pass(pv):
        dp = np.zeros((rows,) + h.shape[1:], f)
        dp[:n] = h - pv
        dp = dp.reshape(rows // T, T, -1)                   # [k, thread, channel]: row k T + thread
        s1, s2 = np.zeros(dp.shape[1:], f), np.zeros(dp.shape[1:], f)
        for k in range(dp.shape[0]):
            s1 = s1 + dp[k]
            s2 = (s2.astype(F64) + dp[k].astype(F64) ** 2).astype(f)
        if T == 16:
            t1, t2 = np.zeros_like(s1[0]), np.zeros_like(s2[0])
            for k in range(16):
                t1, t2 = t1 + s1[k], t2 + s2[k]
        else:
            t1, t2 = _tree(s1), _tree(s2)
        inv = f(1) / f(n)
        dm = t1 * inv
        var = np.maximum(((t2 * inv).astype(F64) - dm.astype(F64) ** 2).astype(f), f(0))    # (one rounding: the fma)
        return pv + dm, var, bool((dm * dm > f(REDO) * var).any())

    mu, var, bad = one_pass(h[0])
    if bad and form != 'row0':
        mu, var, bad = one_pass(mu)
    return mu, var, (f(1) / np.sqrt(var + f(eps))).astype(f)


def scan_seed(name, limit=200, table=None, regime=None):
    for seed in range(limit):
        d = tail_inputs(name, seed, table, regime)
        if not d['router'] or (min_margin(d) >= MARGIN and (regime is None or ambiguous(d)[1] <= 1e-3)):
            return seed
    raise RuntimeError('no seed for ' + name)


if __name__ == '__main__':          # python tests/exit_ref.py: the seeds of TAIL_CASES
    for table in (TAIL_CASES, TUNED_TAIL_CASES):
        for name in table:
            print(name, scan_seed(name, table=table))
    for name, regime in REGIME_RUNS:
        print('    (%r, %r): %d,' % (name, regime, scan_seed(name, table=tail_table(name), regime=regime)))
