"""Float64 reference of ActivityError, the reference's lines (scripts/lib/layer_types.py:287-293) written out literally:

    x passes through;  c_mod[s] = α * sum(square(x[s])) over every axis but the batch;  c_err = 0, n_ops = 0, no parameters

TEST INFRASTRUCTURE: nothing here is on the product path.

The nets weigh the cost per sample: SRNet takes mean(c_err + c_mod), ActorNet / CriticNet mean(stop_gradient(p_tr) c_mod), so
with w[s] = dL/dc_err[s] of the leaf (1/n, or p_tr[s]/n: mpnn_route's w_cerr) the gradient into x[s] is 2 α w[s] x[s].  The
exit kernels add it where the layer may stand in a LogReg chain:
  'map'     behind Select    x = relu(bn(map)) [n, K]    dX[s][k] += 2 α w[s] x[s][k]                       map_bwd_extra
  'logits'  behind LinTrans  x = z [n, nc]               dz[s][k] += 2 α w[s] z[s][k]                       head_bwd_extra
  'probs'   behind Softmax   x = p = softmax(z)          dz[s][k] += 2 α w[s] p_k (p_k - sum_j p_j^2)       head_bwd_extra
(the last is d/dz_k of α sum_j p_j^2 through the softmax: sum_j 2 p_j p_j (δ_jk - p_k)).  Each function returns the term
with its bound, the sum of the absolute values of its own terms; they ADD to exit_ref.tail_bwd / lin_bwd / squared_error_ref.
head_bwd.  ``dt=np.float32``: the same lines in numpy float32, the stand-in for the kernels.

Below them: ``RefNetActivity`` (oracle.ref_net.RefNet with the layer) and the cases of tests/test_activity_kernels.py.
"""
import numpy as np
import torch

import exit_ref as X
import squared_error_ref as SQ
import superclass_ref as SU

F64 = np.float64


def layer(x, α):
    """(x, c_mod) of the layer on a batch x of any rank (:292-293), float64."""
    x = np.asarray(x, F64)
    dims = tuple(range(1, x.ndim))
    return x, α * np.sum(np.square(x), dims)


def softmax(z, dt=F64):
    return SQ.softmax(z, dt)


def head_bwd_extra(z, p, w, α_z, α_p, dt=F64):
    """(term, bound) the layer adds to dL/dz [n, nc]: 2 w α_z z + 2 w α_p p (p - sum_j p_j^2); p None: a head without
    Softmax (α_p must be 0 there)."""
    z, w = np.asarray(z, dt), np.asarray(w, dt)[:, None]
    term = dt(2) * w * dt(α_z) * z
    bound = 2 * np.abs(w) * abs(α_z) * np.abs(z)
    if p is None:
        assert α_p == 0
        return term, bound
    p = np.asarray(p, dt)
    pp = (p * p).sum(1, keepdims=True)
    term = term + dt(2) * w * dt(α_p) * p * (p - pp)
    return term, bound + 2 * np.abs(w) * abs(α_p) * p * (p + pp)


def map_bwd_extra(xa, w, α, dt=F64):
    """(term, bound) the layer adds to dL/dx of the activated map xa [n, K]: 2 α w[s] xa[s][k] (one term: its own bound)."""
    term = dt(2) * dt(α) * np.asarray(w, dt)[:, None] * np.asarray(xa, dt)
    return term, np.abs(term)


def cost_t(x, w, α):
    """mean-weighted cost on torch tensors: sum_s w[s] α sum(x[s]^2) (autograd checks the two functions against it)."""
    return (w * α * (x ** 2).reshape(len(x), -1).sum(1)).sum()


class RefNetActivity(SQ.RefNetSquared, SU.RefNetSuper):
    """RefNet whose `_link` knows ActivityError (and, through its bases, SquaredError and SuperclassCrossEntropyError): the
    layer's lines on torch float64 tensors.  RefNet's Chain sums c_mod over the components and its nets weigh it with
    p_tr.detach(): a per-sample c_mod tensor broadcasts there."""

    def _link(self, ℓ, x, y, mode, out):
        if type(ℓ).__name__ != 'ActivityError':
            return super()._link(ℓ, x, y, mode, out)
        dims = tuple(range(1, x.dim()))
        out[id(ℓ)] = dict(c_err=0.0, c_mod=ℓ.hypers.α * torch.sum(torch.square(x), dims), n_ops=0, x=x)
        return x


# ---- the limits of the GPU kernel tests: the project's constants (tests/test_exit_gen_kernels.py), bound extended by the term's
grad_lim = lambda bound: 4e-6 * bound + 1e-6          # dx, the fused dz and the fused reductions
dz_lim = lambda bound: 2e-5 * bound + 1e-9            # dz of the head

# ---- the cases of tests/test_activity_kernels.py (inputs: the tables of tests/exit_ref.py) -----------------------------------
# affine maps: index into the table -> α.  Signs alternate (α is any finite float); magnitudes are of order one so that the
# term stands far above the limit wherever the map is active (tests/test_activity_error_ref_cpu.py asserts it).
TUNED_LIN = {0: 0.5, 1: -0.75, 3: 0.5, 5: 1.0, 7: -0.5}          # into exit_ref.TUNED_LIN_CASES
TUNED_LIN_MULTI_α = (0.5, 0.0, -0.75, 0.0)                        # per record of exit_ref.TUNED_LIN_MULTI: records 0 and 2 only
GEN_LIN = {0: 0.5, 1: -0.75, 5: 1.0, 6: -0.5}                     # into exit_ref.LIN_CASES
# exit tails: (α_z, α_p) combinations per loss kind; the linear form has no softmax, so α_p does not exist there
FORMS = ('ce', 'sq', 'lin')
LOSS = {'ce': 0, 'sq': 1, 'lin': 2}                               # MPNN_LOSS_*
ALPHAS = {'ce': [(0.05, 0.0), (0.0, -0.5), (-0.05, 0.5)], 'sq': [(0.05, 0.0), (0.0, -0.5), (-0.05, 0.5)], 'lin': [(0.05, 0.0), (-0.05, 0.0)]}
TUNED_TAIL = ('t_one', 't_r5', 't_full', 't_head', 't_r3_big')   # of exit_ref.TUNED_TAIL_CASES
# any-width: more than 16 classes (20 with n = 129; 100), and n = 37, no multiple of the 64 samples of a head workgroup
# (the 100-class head stands in a table of its own: a case's draw depends on its place in its table, and the cases of
# exit_ref.TAIL_CASES must stay the records tests/test_exit_gen_kernels.py launches under the same names)
C100 = {'act_c100': dict(n=130, nc=100, R=0, R2=0, S=0, stride=4, seed=0, router=False)}
GEN_TAIL = ('table1', 'act_c100', 'class17')


def tail_table(name):
    """The table a tail case is drawn from: exit_ref.TUNED_TAIL_CASES, exit_ref.TAIL_CASES (None) or C100."""
    return X.TUNED_TAIL_CASES if name in X.TUNED_TAIL_CASES else C100 if name in C100 else None


def act_w(n, seed):
    """The leaf's w_cerr of an affine-map case: weights in [0.25, 1), as exit_ref.tail_inputs draws them in [0, 1) (not
    divided by n: dy of these cases is N(0, 1), not a gradient of a mean either)."""
    return (0.25 + 0.75 * np.random.default_rng(1000 + seed).random(n)).astype(np.float32)


def lin_activated(d, dt=F64):
    """act(x) [n, K] of an affine-map record (exit_ref.lin_inputs)."""
    return X.act(d['x'], d['mode'], d['gamma'], d['beta'], d['m_avg'], d['v_avg'], dt=dt).reshape(d['n'], d['K'])


def lin_ref_with(d, ref, w, α, dt=F64):
    """exit_ref.lin_ref's result with the layer's term in dx (dW, db, y are not touched by it)."""
    t, b = map_bwd_extra(lin_activated(d, dt), w, α, dt)
    return dict(ref, dx=(ref['dx'][0] + t, ref['dx'][1] + b))


def tail_dz(d, form, α_z, α_p, dt=F64):
    """(dz, bound) of a tail record's head (exit_ref.tail_inputs) with loss `form` and the layer's terms."""
    z, y, w = d['z'], d['y'], d['w_cerr']
    if form == 'ce':
        f = X.head_fwd(z, y, d['eps_ce'], dt)
        p, q = f['p'], f['q']
        t = -np.asarray(w, dt)[:, None] * np.asarray(y, dt) * (1 - dt(d['eps_ce'])) / q
        dz, bound = p * (t - (t * p).sum(1, keepdims=True)), p * (np.abs(t) + (np.abs(t) * p).sum(1, keepdims=True))
    else:
        dz, bound = SQ.head_bwd(z, y, w, form, dt)
        p = None if form == 'lin' else softmax(z, dt)
    te, be = head_bwd_extra(z, p, w, α_z, α_p, dt)
    return dz + te, bound + be
