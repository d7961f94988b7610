"""Float64 reference of MultiscaleLLN, the reference's lines (scripts/lib/layer_types.py:127-147) written out literally:
the 2-D filter k[u, v, c] = g(u, v) lum[c], the explicit zero pad of s = ceil(2σ), the SAME cross-correlation, the crop,
the density from an image of ones, x / (lum / dens + ϵ).  Deliberately NOT the separable form the kernel runs
(csrc/lln.hip).  TEST INFRASTRUCTURE: nothing here is on the product path.

``RefNetLLN`` is oracle.ref_net.RefNet with that layer: `_link` handles 'MultiscaleLLN' and defers everything else.
"""
import numpy as np
import torch
import torch.nn.functional as TF

from oracle import ref_net
from oracle.ref_net import RefNet

LUM = [[0.2126], [0.7152], [0.0722]]


def radius(σ):
    return int(np.ceil(2 * σ))                                       # :133


def lln_filter(σ):
    """k [2s+1, 2s+1, 3, 1] (:134-137)."""
    s = radius(σ)
    u = np.linspace(-s, s, 2 * s + 1)[:, None, None, None]
    v = np.linspace(-s, s, 2 * s + 1)[:, None, None]
    return np.exp(-(u ** 2 + v ** 2) / (2 * σ ** 2)) / (2 * np.pi * σ ** 2) * LUM


def pad(x, s):
    """tf.pad(x, [[0, 0], [s, s], [s, s], [0, 0]])."""
    return np.pad(x, [(0, 0), (s, s), (s, s), (0, 0)])


def conv_same(x, k):
    """tf.nn.conv2d(x, k, (1, 1, 1, 1), 'SAME') for an odd support: cross-correlation, (K - 1) // 2 zeros each way."""
    K = k.shape[0]
    n, H, W, _ = x.shape
    xp = pad(x, (K - 1) // 2)
    out = np.zeros((n, H, W, k.shape[3]))
    for a in range(K):
        for b in range(K):
            out += xp[:, a:a + H, b:b + W, :] @ k[a, b]
    return out


def local_mean(x_i, σ):
    """lum / dens [n, h, w, 1] of one scale (:140-146): the Gaussian-weighted mean luminance over the part of the window
    that lies inside the map."""
    x_i = np.asarray(x_i, np.float64)
    s, k = radius(σ), lln_filter(σ)
    h, w = x_i.shape[1:3]
    lum = conv_same(pad(x_i, s), k)[:, s:s + h, s:s + w, :]
    dens = conv_same(pad(np.ones_like(x_i), s), k)[:, s:s + h, s:s + w, :]
    return lum / dens


def pyramid(x, n_scales):
    """ToPyramid (:118-125): at an integer ratio the legacy bilinear resize is the strided pick (oracle/np_ops.py)."""
    return [x[:, ::2 ** i, ::2 ** i, :] for i in range(n_scales)]


def lln(x, n_scales, σ=3, ϵ=1e-3):
    """The layer behind ToPyramid: [x_i / (lum_i / dens_i + ϵ)] (:147), float64."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return [x_i / (local_mean(x_i, σ) + ϵ) for x_i in pyramid(x, n_scales)]


class RefNetLLN(RefNet):
    """RefNet whose `_link` knows MultiscaleLLN: the same lines on torch float64 tensors (the image carries no gradient)."""

    def _link(self, ℓ, x, y, mode, out):
        if type(ℓ).__name__ != 'MultiscaleLLN':
            return super()._link(ℓ, x, y, mode, out)
        ϕ = ℓ.hypers
        s = radius(ϕ.σ)
        k = torch.tensor(lln_filter(ϕ.σ), dtype=self.dtype)
        res = []
        for x_i in x:
            h, w = x_i.shape[1:3]
            p = lambda t: TF.pad(t, (0, 0, s, s, s, s))
            lum = ref_net._nhwc(TF.conv2d(ref_net._nchw(p(x_i)), k.permute(3, 2, 0, 1), padding=s))[:, s:s + h, s:s + w, :]
            dens = ref_net._nhwc(TF.conv2d(ref_net._nchw(p(torch.ones_like(x_i))), k.permute(3, 2, 0, 1), padding=s))[:, s:s + h, s:s + w, :]
            res.append(x_i / (lum / dens + ϕ.ϵ))
        out[id(ℓ)] = dict(c_err=0.0, c_mod=0.0, n_ops=0, x=res)
        return res


# ---- the separable fp32 model of the kernel, and the tolerance of the GPU tests -----------------------------------

def taps(σ):
    s = radius(σ)
    u = np.arange(-s, s + 1, dtype=np.float64)
    return np.exp(-u ** 2 / (2 * σ ** 2))


def model_fp32(x, n_scales, σ, ϵ):
    """What csrc/lln.hip computes, in numpy float32: luminance, two 1-D passes in tap order, the row / column density
    factors as differences of the taps' prefix sums, IEEE division.  (numpy has no fused multiply-add: every product
    is rounded, which the device does not do -- the model's error is an upper estimate of the kernel's.)"""
    f = np.float32
    x = np.asarray(x, f)
    s = radius(σ)
    g = taps(σ).astype(f)
    cum = np.concatenate([[0.0], np.cumsum(g.astype(np.float64))]).astype(f)
    res = []
    for x_i in pyramid(x, n_scales):
        n, h, w, _ = x_i.shape
        Y = f(0.2126) * x_i[..., 0]
        Y = f(0.7152) * x_i[..., 1] + Y
        Y = f(0.0722) * x_i[..., 2] + Y
        Yp = np.pad(Y, [(0, 0), (s, s), (s, s)])
        Hs = np.zeros((n, h + 2 * s, w), f)
        for v in range(2 * s + 1):
            Hs = g[v] * Yp[:, :, v:v + w] + Hs
        lum = np.zeros((n, h, w), f)
        for u in range(2 * s + 1):
            lum = g[u] * Hs[:, u:u + h, :] + lum
        r, c = np.arange(h), np.arange(w)
        dr = cum[np.minimum(2 * s, h - 1 - r + s) + 1] - cum[np.maximum(0, s - r)]
        dc = cum[np.minimum(2 * s, w - 1 - c + s) + 1] - cum[np.maximum(0, s - c)]
        with np.errstate(divide='ignore', invalid='ignore'):
            d = lum / (dr[:, None] * dc[None, :]) + f(ϵ)
            res.append(x_i / d[..., None])
    return res


U = 2.0 ** -24


def chain(σ):
    """Roundings on the longest path, with a factor of two of headroom for reciprocal-based division."""
    return 4 * radius(σ) + 16


def bound(x, n_scales, σ, ϵ, signed):
    """The per-element error bound of every scale (float64 arrays shaped like the outputs) and the reference itself.
    Positive images: chain u |ref| (no cancellation).  Signed images: chain u (|ref| + |x| m_abs / (m + ϵ)²), m_abs the
    same weighted mean of |x| -- the first-order propagation of the sum's error through the division."""
    x = np.asarray(x, np.float64)
    ref, bnd = [], []
    for x_i in pyramid(x, n_scales):
        m = local_mean(x_i, σ)
        r = x_i / (m + ϵ)
        b = np.abs(r)
        if signed:
            b = b + np.abs(x_i) * local_mean(np.abs(x_i), σ) / (m + ϵ) ** 2
        ref.append(r)
        bnd.append(chain(σ) * U * b)
    return ref, bnd


# ---- the inputs of tests/test_lln_kernel.py (shared with the CPU test that shows its tolerance can be met) ----------

TILE = 32                                       # LLN_T of csrc/lln.hip
# (H, W), scales: smaller than every filter | coarsest map 1x2 | the tuned nets' image | the general nets' image |
# larger than the tile on both axes (rows 32 + 8, columns 32 + 32 + 4: seams and halos between tiles on both)
SHAPES = [((4, 4), 1), ((8, 16), 4), ((32, 32), 4), ((24, 40), 4), ((40, 68), 2)]
SIGMAS = (0.5, 1.5, 3, 8)                       # s = 1, 3, 6, 16
N = 5


def kernel_input(shape, signed, seed=0):
    """[N, H, W, 3] float32: U(0.1, 1) (no cancellation in the local mean) or N(0, 0.25²), which the tests pair with
    ϵ = 1 (then min |m + ϵ| >= 0.25: tests/test_lln_ref_cpu.py)."""
    rng = np.random.default_rng(1000 * seed + 10 * shape[0] + shape[1] + (500 if signed else 0))
    x = rng.normal(0, 0.25, (N,) + tuple(shape) + (3,)) if signed else rng.uniform(0.1, 1, (N,) + tuple(shape) + (3,))
    return x.astype(np.float32)


def kernel_cases():
    """(shape, n_scales, σ, ϵ, signed): every shape x σ with positive images at both ϵ and signed images at ϵ = 1."""
    return [(shape, S, σ, ϵ, signed) for shape, S in SHAPES for σ in SIGMAS
            for ϵ, signed in ((1e-3, False), (1, False), (1, True))]
