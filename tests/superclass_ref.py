"""Float64 reference of SuperclassCrossEntropyError, the reference's lines (scripts/lib/layer_types.py:274-285) written out
literally: y_sup = y @ w_cls, p = ϵ / n_sup + (1 - ϵ) x, c_err = -sum(y_sup log p), δ_cor = [argmax x == argmax y_sup]
(first index on ties: the stand-in's stated assumption and what the exit kernels do).  TEST INFRASTRUCTURE: nothing here is
on the product path.

``RefNetSuper`` is oracle.ref_net.RefNet with that layer: `_link` handles 'SuperclassCrossEntropyError' and defers
everything else.  Below it: the maps the net tests use, the fp32 model of csrc/label_map.hip's fold, its tolerance and
the case tables of tests/test_label_map_kernel.py.
"""
import numpy as np
import torch

from oracle.ref_net import RefNet


def label_map(y, w):
    """y_sup = y @ w_cls in float64 (:280)."""
    return np.asarray(y, np.float64) @ np.asarray(w, np.float64)


def layer(x, y, w_cls, ϵ=1e-6):
    """(c_err, δ_cor, y_sup) of the layer on softmax rows x [n, n_sup] and labels y [n, n_cls] (:280-285), float64."""
    x = np.asarray(x, np.float64)
    y_sup = label_map(y, w_cls)
    n_cls = y_sup.shape[1]
    p_cls = ϵ / n_cls + (1 - ϵ) * x
    c_err = -np.sum(y_sup * np.log(p_cls), 1)
    δ_cor = (np.argmax(x, 1) == np.argmax(y_sup, 1)).astype(np.float64)
    return c_err, δ_cor, y_sup


class RefNetSuper(RefNet):
    """RefNet whose `_link` knows SuperclassCrossEntropyError: the same lines on torch float64 tensors (the map is a
    constant: no gradient to it or to y)."""

    def _link(self, ℓ, x, y, mode, out):
        if type(ℓ).__name__ != 'SuperclassCrossEntropyError':
            return super()._link(ℓ, x, y, mode, out)
        ϕ = ℓ.hypers
        y_sup = torch.as_tensor(y, dtype=self.dtype) @ torch.tensor(np.asarray(ϕ.w_cls, np.float64), dtype=self.dtype)
        n_cls = y_sup.shape[1]
        p_cls = ϕ.ϵ / n_cls + (1 - ϕ.ϵ) * x
        out[id(ℓ)] = dict(c_err=-(y_sup * torch.log(p_cls)).sum(1), c_mod=0.0, n_ops=0, x=x,
                          δ_cor=(torch.argmax(x, 1) == torch.argmax(y_sup, 1)).to(self.dtype))
        return x


# ---- the maps of the net tests ---------------------------------------------------------------------------------------

def hard_map(n_cls, n_sup):
    """0/1 map: class c belongs to superclass c * n_sup // n_cls (consecutive groups of equal size where it divides)."""
    w = np.zeros((n_cls, n_sup), np.float32)
    w[np.arange(n_cls), np.arange(n_cls) * n_sup // n_cls] = 1
    return w


def soft_map(n_cls, n_sup):
    """Dyadic soft map: 0.75 on the class's own superclass, 0.25 on the next one (a 0.75 / 0.25 margin: the maximum of
    y_sup is unique for one-hot labels)."""
    w = 0.75 * hard_map(n_cls, n_sup)
    w[np.arange(n_cls), (np.arange(n_cls) * n_sup // n_cls + 1) % n_sup] += 0.25
    return w.astype(np.float32)


# ---- the fp32 model of the kernel, and the tolerance of the GPU test ----------------------------------------------------

U = 2.0 ** -24


def model_fp32(y, w):
    """What csrc/label_map.hip computes, in numpy float32: acc = 0; for c in class order: acc = y[:, c] * w[c, :] + acc.
    (numpy has no fused multiply-add: every product is rounded too, which the device does not do -- the model's error is an
    upper estimate of the kernel's.  Its worst case, two roundings per term, is beyond the bound below; on the test's
    inputs it stays well inside: tests/test_superclass_ref_cpu.py.)"""
    y, w = np.asarray(y, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((y.shape[0], w.shape[1]), np.float32)
    for c in range(w.shape[0]):
        acc = y[:, c:c + 1] * w[c:c + 1, :] + acc
    return acc


def bound(y, w):
    """(reference, per-element bound): |got - ref| <= (n_cls + 1) 2^-24 sum_c |y_c w_cs| -- the rounding of an n_cls-long
    fmaf chain (each partial sum rounded once, relative error 2^-24 at most, first order, one term of headroom)."""
    y, w = np.asarray(y, np.float64), np.asarray(w, np.float64)
    return y @ w, (w.shape[0] + 1) * U * (np.abs(y) @ np.abs(w))


# ---- the inputs of tests/test_label_map_kernel.py (shared with the CPU test that shows its tolerance can be met) -----------

TILE_R, TILE_S, CHUNK = 16, 16, 64              # LM_R, LM_S, LM_C of csrc/label_map.hip
SIZES = [(1, 1), (2, 1), (10, 2), (10, 3), (17, 16), (100, 20), (1024, 17), (16, 1024),
         # columns one below, at and one above the column tile, and over two tiles; classes around the LDS chunk
         (10, 15), (10, 16), (10, 33), (63, 5), (64, 5), (65, 5), (129, 31)]
NS = [1, 5, 15, 16, 17, 63, 64, 65, 129]       # (15, 16, 17: one below, at and one above the row tile)
N_MAX = max(NS)


def _rng(kind, n_cls, n_sup):
    return np.random.default_rng(7919 * n_cls + 31 * n_sup + {'onehot': 0, 'dyadic': 1, 'soft': 2}[kind])


def kernel_input(kind, n_cls, n_sup, n=N_MAX):
    """(y [n, n_cls], w [n_cls, n_sup]) float32.
    'onehot': one-hot labels, finite non-zero weights N(0, 1) -- the result is exactly the label's row of w;
    'dyadic': labels k / 8 on up to 3 classes, weights j / 16 with |j| <= 32 -- every product and partial sum is a multiple
              of 2^-7 below 2^12: exact in fp32 whatever the order;
    'soft'  : labels a softmax row, weights N(0, 1) (signed: cancellation is in the bound through sum |y w|)."""
    rng = _rng(kind, n_cls, n_sup)
    if kind == 'onehot':
        y = np.eye(n_cls, dtype=np.float32)[rng.integers(0, n_cls, n)]
        w = rng.standard_normal((n_cls, n_sup)).astype(np.float32)
        w[w == 0] = 1.0
    elif kind == 'dyadic':
        y = np.zeros((n, n_cls), np.float32)
        for _ in range(3):
            y[np.arange(n), rng.integers(0, n_cls, n)] += rng.integers(1, 4, n) / 8.0
        w = (rng.integers(-32, 33, (n_cls, n_sup)) / 16.0).astype(np.float32)
    else:
        z = rng.standard_normal((n, n_cls))
        y = (np.exp(z) / np.exp(z).sum(1, keepdims=True)).astype(np.float32)
        w = rng.standard_normal((n_cls, n_sup)).astype(np.float32)
    return y, w


def kernel_cases():
    """(n_cls, n_sup): the test runs each at n = 129 = N_MAX and at every smaller n of NS on a prefix of the same rows."""
    return list(SIZES)
