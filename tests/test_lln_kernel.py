"""GPU: mpnn_lln_fwd (csrc/lln.hip) through the C ABI against the float64 reference tests/lln_ref.py -- the reference's
lines written out literally, not the separable form the kernel runs.

Shapes (tests/lln_ref.py: SHAPES), the smallest that reach each edge: 4x4 with one scale (smaller than every filter), 8x16
with four (coarsest map 1x2), 32x32 and 24x40 with four, 40x68 with two (larger than the 32x32 tile on both axes: seams and
halos between tiles) -- each with σ = 0.5, 1.5, 3, 8 (s = 1, 3, 6, 16), n = 1 and 5, ϵ = 1e-3 and 1, and a table of three
records with different n.

Tolerance, u = 2^-24, chain = 4 s + 16 (every rounding on the longest path -- 3 luminance terms, 2 (2 s + 1) taps, the
density, the divisions -- with a factor of two of headroom):
  positive images U(0.1, 1):   |got - ref| <= chain u |ref|
  signed images N(0, 0.25²), ϵ = 1:  |got - ref| <= chain u (|ref| + |x| m_abs / (m + ϵ)²)
Worst observed |got - ref| / bound on an MI355X over the 60 cases (each at n = 5 and n = 1): 0.255 on positive images
(8x16, σ = 0.5, ϵ = 1e-3), 0.095 on signed ones; the fp32 numpy model of tests/test_lln_ref_cpu.py comes to 0.234.

Also: 64 guard words on each side of every output buffer stay as they were; the image at sample 0 gives the same bits with
n = 1 as with n = 5, and as record 0 or record 2 of a table; the refusals return their codes with the outputs unwritten.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lln_ref as R
from lib import _hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
SENTINEL = np.float32(-1.2345678e25)


def geom_of(shape, S, σ, n_max, radius=None):
    g = _hip.LlnGeom()
    g.n_max, g.H, g.W, g.n_scales = n_max, shape[0], shape[1], S
    g.radius = R.radius(σ) if radius is None else radius
    for k, t in enumerate(R.taps(σ)[:2 * _hip.LLN_MAX_RADIUS + 1]):
        g.tap[k] = t
    return g


class Record:
    """One net's record: the images on the device and a guarded buffer per scale."""

    def __init__(self, x, shape, S, eps, cap=None):
        n = x.shape[0]
        cap = n if cap is None else cap                   # (samples the buffers hold: rows beyond n must stay untouched)
        self.n, self.S, self.shape = n, S, shape
        self.x = torch.from_numpy(np.array(x)).to(DEV)                # (a copy: the shared inputs are read-only)
        self.sizes = [cap * (shape[0] >> i) * (shape[1] >> i) * 3 for i in range(S)]
        self.bufs = [torch.full((sz + 2 * GUARD,), float(SENTINEL), device=DEV) for sz in self.sizes]
        self.rec = _hip.LlnArgs()
        self.rec.x, self.rec.n, self.rec.eps = self.x.data_ptr(), n, eps
        for i, b in enumerate(self.bufs):
            self.rec.out[i] = b.data_ptr() + 4 * GUARD

    def results(self):
        """[n, h, w, 3] per scale (as int32 bit patterns too), after checking the guards and the rows beyond n."""
        sent = SENTINEL.view(np.int32)
        outs = []
        for i, (b, sz) in enumerate(zip(self.bufs, self.sizes)):
            bits = b.cpu().numpy().view(np.int32)
            h, w = self.shape[0] >> i, self.shape[1] >> i
            used = self.n * h * w * 3
            assert (bits[:GUARD] == sent).all() and (bits[GUARD + used:] == sent).all(), ('written outside out[%d]' % i)
            outs.append(bits[GUARD:GUARD + used].reshape(self.n, h, w, 3).copy())
        return outs


def launch(records, geom):
    lib = _hip.load()
    tab = _hip.to_device_table([r.rec for r in records], DEV)
    rc = lib.mpnn_lln_fwd(tab.data_ptr(), len(records), C.byref(geom), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def reference(shape, S, σ, eps, signed):
    """(input, reference, bound) of one case: computed once, shared, never written."""
    x = R.kernel_input(shape, signed)
    ref, bnd = R.bound(x, S, σ, eps, signed)
    for a in [x] + ref + bnd:
        a.setflags(write=False)
    return x, ref, bnd


def worst_ratio(outs, ref, bnd):
    worst = 0.0
    for o, r, b in zip(outs, ref, bnd):
        got = o.view(np.float32).astype(np.float64)
        n = got.shape[0]
        assert np.isfinite(got).all()
        worst = max(worst, float((np.abs(got - r[:n]) / b[:n]).max()))
    return worst


@pytest.mark.parametrize('shape,S,σ,eps,signed', R.kernel_cases())
def test_against_the_float64_reference(shape, S, σ, eps, signed):
    x, ref, bnd = reference(shape, S, σ, eps, signed)
    five, one = Record(x, shape, S, eps), Record(x[:1], shape, S, eps)
    assert launch([five], geom_of(shape, S, σ, R.N)) == 0
    assert launch([one], geom_of(shape, S, σ, 1)) == 0
    o5, o1 = five.results(), one.results()
    w5, w1 = worst_ratio(o5, ref, bnd), worst_ratio(o1, ref, bnd)
    print('lln %dx%d S=%d σ=%g ϵ=%g %s: worst |got - ref| / bound = %.3f (n = 5), %.3f (n = 1)'
          % (*shape, S, σ, eps, 'signed' if signed else 'positive', w5, w1))
    assert w5 <= 1.0 and w1 <= 1.0, (w5, w1)
    for a, b in zip(o5, o1):                              # the image at sample 0: the same bits whatever n
        assert np.array_equal(a[:1], b)


@pytest.mark.parametrize('shape,S,σ', [((32, 32), 4, 3), ((40, 68), 2, 8), ((8, 16), 4, 1.5)])
def test_table_of_three_records_with_different_n(shape, S, σ):
    eps = 1e-3
    x, ref, bnd = reference(shape, S, σ, eps, False)
    other = R.kernel_input(shape, False, seed=7)
    r_other, b_other = R.bound(other, S, σ, eps, False)
    # record 0: n = 3, record 1: other images, n = 5 = n_max, record 2: n = 2 in buffers of 5 (rows 2.. stay untouched)
    recs = [Record(x[:3], shape, S, eps), Record(other, shape, S, eps), Record(x[:2], shape, S, eps, cap=5)]
    assert launch(recs, geom_of(shape, S, σ, 5)) == 0
    outs = [r.results() for r in recs]
    assert worst_ratio(outs[0], ref, bnd) <= 1.0 and worst_ratio(outs[2], ref, bnd) <= 1.0
    assert worst_ratio(outs[1], r_other, b_other) <= 1.0
    alone = Record(x[:1], shape, S, eps)
    assert launch([alone], geom_of(shape, S, σ, 1)) == 0
    for a, b, c in zip(alone.results(), outs[0], outs[2]):        # sample 0 as record 0, as record 2 and alone
        assert np.array_equal(a, b[:1]) and np.array_equal(a, c[:1])
    for b, c in zip(outs[0], outs[2]):
        assert np.array_equal(b[:2], c)


def test_zero_denominator_is_not_clamped():
    """lum / dens + ϵ == 0 divides as IEEE does (TensorFlow would): a zero image with ϵ = 0 gives nan, nothing is clamped."""
    x = np.zeros((1, 8, 8, 3), np.float32)
    x[0, :, 4:] = 1.0
    r = Record(x, (8, 8), 1, 0.0)
    assert launch([r], geom_of((8, 8), 1, 0.5, 1)) == 0
    got = r.results()[0].view(np.float32)
    assert np.isnan(got[0, :, :3]).all()                  # 0 / 0 where the window sees only zeros
    assert np.isfinite(got[0, :, 4:]).all() and (got[0, :, 5:] > 0).all()


def test_refusals_leave_the_outputs_unwritten():
    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    shape, S, σ = (16, 16), 2, 1.5
    x = R.kernel_input((16, 16), False)[:2]
    r = Record(x, shape, S, 1e-3)
    tab = _hip.to_device_table([r.rec], DEV)
    good = geom_of(shape, S, σ, 2)

    def edited(**kw):
        g = geom_of(shape, S, σ, 2)
        for k, v in kw.items():
            setattr(g, k, v)
        return g
    shape_cases = [dict(radius=0), dict(radius=17), dict(n_scales=0), dict(n_scales=9), dict(H=0), dict(W=0), dict(H=257), dict(W=264),
                   dict(H=15), dict(W=18, n_scales=3), dict(H=12, n_scales=4)]
    for kw in shape_cases:
        assert lib.mpnn_lln_fwd(tab.data_ptr(), 1, C.byref(edited(**kw)), st) == _hip.E_SHAPE, kw
    assert lib.mpnn_lln_fwd(None, 1, C.byref(good), st) == _hip.E_ARG
    assert lib.mpnn_lln_fwd(tab.data_ptr(), 1, None, st) == _hip.E_ARG
    assert lib.mpnn_lln_fwd(tab.data_ptr(), 0, C.byref(good), st) == _hip.E_ARG
    assert lib.mpnn_lln_fwd(tab.data_ptr(), -1, C.byref(good), st) == _hip.E_ARG
    assert lib.mpnn_lln_fwd(tab.data_ptr(), 1, C.byref(edited(n_max=0)), st) == _hip.E_ARG
    torch.cuda.synchronize()
    sent = SENTINEL.view(np.int32)
    for b in r.bufs:
        assert (b.cpu().numpy().view(np.int32) == sent).all()
    assert launch([r], good) == 0                          # ... and the same record runs once the geometry is right
    ref, bnd = R.bound(x, S, σ, 1e-3, False)
    assert worst_ratio(r.results(), ref, bnd) <= 1.0
