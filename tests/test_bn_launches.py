"""The three elementwise BatchNorm launches of csrc/misc.hip -- mpnn_bn_relu_fwd, mpnn_bn_bwd_reduce, mpnn_bn_bwd_apply --
alone, through the C ABI, on the GPU, against the float64 restatement of tests/small_launch_ref.py.

Eight kernels stand behind the three entry points and the channel count selects among them (the table KERNELS of
small_launch_ref, which the CPU test holds to the two predicates of misc.hip): the cases run every kernel at one pixel,
at one pixel less than a reduction workgroup takes side by side, and on four reduction workgroups with a remainder, in
batch mode with 8 slots; and every kernel in the other modes -- moving averages (`sum` NULL), plain ReLU (every BatchNorm
pointer NULL, cnt = n_pix, as lib/_plan_conv.py passes it), identity (mpnn_bn_relu_fwd only: a copy, bit for bit) -- and
with 1, 3, 8 and 16 slots of statistics and 0 (= 1), 1, 3, 8 and 16 slots of reductions.  Statistics buffers always hold
MPNN_BN_SLOTS slots: those beyond the count in use are NaN where the kernel reads, and must keep their bits where it adds.

Every output sits between sentinel guards (hiputil.Guarded), plain-store outputs pre-filled with NaN; red_out starts
from known non-zero values.  No element is excluded from a comparison: the maps keep a margin of 1e-3 around every ReLU
edge (in float64), and the plain-ReLU maps carry exact +0 and -0, whose mask is 0.  dz is a copy or a zero, so it is
compared exactly; y and g within 2e-6 of the sum of the absolute values of their terms (+ 1e-6), the fp64 reductions
within 1e-5 (+ 1e-9), as tests/test_conv_ch.py::test_bn_launches_any_c_vs_float64 writes the bounds.  Every launch runs
twice: equal bits, red_out included where one workgroup does all the adding.
"""
import ctypes as C

import numpy as np
import pytest

from lib import _hip
import small_launch_ref as R

S = _hip.BN_SLOTS
NAN = float('nan')
MODE = dict(id=_hip.ACT_IDENTITY, relu=_hip.ACT_RELU, batch=_hip.ACT_BN_BATCH, moving=_hip.ACT_BN_MOVING)
pytestmark = pytest.mark.gpu


def _close(got, ref, bound, rel=R.REL, what=''):
    err = np.abs(np.asarray(got, np.float64) - ref)
    lim = rel * bound + 1e-6
    print('worst error / limit, %s: %.3g' % (what, float((err / lim).max())))
    assert np.all(np.isfinite(got)), what + ': not every element written'
    assert (err <= lim).all(), '%s: worst %.3g (limit %.3g)' % (what, float((err - lim).max()), float(lim.max()))


def _sum_close(got, ref, bound, what):
    err = np.abs(got - ref)
    print('worst error / limit, %s: %.3g' % (what, float((err / (1e-5 * bound + 1e-9)).max())))
    assert (err <= 1e-5 * bound + 1e-9).all(), '%s: worst %.3g' % (what, float(err.max()))


class Dev:
    """The device side of one small_launch_ref.ActMap."""

    def __init__(self, a):
        import torch
        import hiputil as U
        self.a, self.U = a, U
        self.sd = U.dev(a.s.reshape(-1))
        self.bn = None
        if a.mode in ('batch', 'moving'):
            self.bn = dict(sum=U.dev(a.sums, torch.float64), gamma=U.dev(a.gamma), beta=U.dev(a.beta),
                           m_avg=U.dev(a.m_avg), v_avg=U.dev(a.v_avg), eps=float(R.EPS), nslot=a.nslot)

    def act(self, x=True):
        a = self.a
        return _hip.act(self.sd if x else None, a.C, MODE[a.mode], 0, self.bn, a.cnt, nslot=a.nslot)

    def ctx(self, red=None, red_nslot=1):
        """mpnn_bn_ctx; red: [S][2C] float64 (slots beyond red_nslot NaN) or None."""
        import torch
        c = _hip.BnCtx()
        c.s, c.bn = self.sd.data_ptr(), self.act(False)
        self.red_d = self.U.dev(red, torch.float64)
        c.red, c.red_nslot = _hip.ptr(self.red_d), red_nslot
        return c

    # -- launches; each returns host copies and has checked its guards
    def relu_fwd(self):
        import torch
        y = self.U.Guarded(self.a.s.size); y.fill(NAN)
        a = self.act()
        _hip.check(_hip.load().mpnn_bn_relu_fwd(C.byref(a), y.ptr(), self.a.n_pix, self.U.stream()), 'bn_relu_fwd')
        torch.cuda.synchronize()
        assert y.guards_ok()
        return y.get().reshape(self.a.s.shape)

    def reduce(self, dy, red_nslot, prior, in_place=False, times=1):
        import torch
        U, a = self.U, self.a
        dz = U.Guarded(a.s.size); dz.fill(dy if in_place else NAN)
        dyd = None if in_place else U.dev(dy.reshape(-1))
        red = U.Guarded(S * 2 * a.C, torch.float64); red.fill(prior)
        ctx = self.ctx(None, red_nslot)
        for _ in range(times):
            _hip.check(_hip.load().mpnn_bn_bwd_reduce(dz.ptr() if in_place else dyd.data_ptr(), C.byref(ctx), dz.ptr(), red.ptr(),
                                                     a.n_pix, U.stream()), 'bn_bwd_reduce')
        torch.cuda.synchronize()
        assert dz.guards_ok() and red.guards_ok()
        return dz.get().reshape(a.s.shape), red.get().reshape(S, 2 * a.C)

    def apply(self, dz, red, red_nslot):
        import torch
        U, a = self.U, self.a
        buf = U.Guarded(a.s.size); buf.fill(dz)
        ctx = self.ctx(red, red_nslot)
        _hip.check(_hip.load().mpnn_bn_bwd_apply(buf.ptr(), C.byref(ctx), a.n_pix, U.stream()), 'bn_bwd_apply')
        torch.cuda.synchronize()
        assert buf.guards_ok()
        return buf.get().reshape(a.s.shape)


def _same_bits(x, y):
    return x.tobytes() == y.tobytes()


@pytest.mark.parametrize('case', R.BN_CASES, ids=list(map(R.case_id, R.BN_CASES)))
def test_bn_launches_vs_float64(case):
    C_, n_pix, mode, nslot, red_nslot = case
    assert R.selected(C_) == R.KERNELS[C_]
    d = R.bn_inputs(case)
    a, rn = d['a'], d['rn']
    dv = Dev(a)
    # mpnn_bn_relu_fwd
    y = dv.relu_fwd()
    assert _same_bits(y, dv.relu_fwd())
    if mode == 'id':
        assert _same_bits(y, a.s)
        return
    want, bound = a.fwd()
    _close(y, want, bound, what='y')
    assert np.array_equal(y > 0, a.on)
    # mpnn_bn_bwd_reduce: dz = dy * [y > 0]; red_out += [sum dz, sum dz * xhat] over the slots in use
    prior = d['prior']
    dz, red = dv.reduce(d['dy'], red_nslot, prior)
    want_dz, want_red, terms = a.reduce(d['dy64'])
    assert np.all(np.isfinite(dz)), 'dz: not every element written'
    assert np.array_equal(dz.astype(np.float64), want_dz), 'dz'
    assert _same_bits(red[rn:], prior[rn:]), 'red_out beyond red_nslot'
    pb = np.abs(prior[:rn]).sum(0)
    _sum_close(red[:rn].sum(0), prior[:rn].sum(0) + want_red, terms + pb + 1e-3, 'red')
    dz2, red2 = dv.reduce(d['dy'], red_nslot, prior)
    assert _same_bits(dz, dz2)
    if R.reduce_blocks(C_, n_pix) == 1:
        assert _same_bits(red, red2)
    # twice into the same red_out: twice the sums
    _, red3 = dv.reduce(d['dy'], red_nslot, prior, times=2)
    assert _same_bits(red3[rn:], prior[rn:])
    _sum_close(red3[:rn].sum(0), prior[:rn].sum(0) + 2 * want_red, 2 * terms + pb + 1e-3, 'red twice')
    # in place, dz == dy (lib/_plan_conv.py masks the head's dX so)
    dz4, red4 = dv.reduce(d['dy'], red_nslot, prior, in_place=True)
    assert _same_bits(dz4, dz), 'in place'
    _sum_close(red4[:rn].sum(0), prior[:rn].sum(0) + want_red, terms + pb + 1e-3, 'red in place')
    # mpnn_bn_bwd_apply, with reductions and with ctx->red == NULL
    for red_in, red64 in ((d['red'], d['red64']), (None, None)):
        g = dv.apply(d['dz'], red_in, red_nslot)
        want, bound = a.apply(d['dz64'], red64)
        _close(g, want, bound, what='g')
        assert _same_bits(g, dv.apply(d['dz'], red_in, red_nslot))


@pytest.mark.parametrize('case', R.CONTRACT_CASES, ids=list(map(R.case_id, R.CONTRACT_CASES)))
def test_relu_fwd_decides_what_the_reduction_decides(case):
    """include/mpnn_hip.h: mpnn_bn_relu_fwd computes exactly what the consumers compute.  On a map drawn WITHOUT the
    margin -- elements within rounding of the ReLU edge -- [y > 0] of mpnn_bn_relu_fwd equals [dz != 0] of
    mpnn_bn_bwd_reduce (dy has no zero), bit for bit; at C = 12 and 48 a quad kernel meets an any-C kernel."""
    a, dy = R.contract_inputs(case)
    dv = Dev(a)
    y = dv.relu_fwd()
    dz, _ = dv.reduce(dy, 8, np.zeros((S, 2 * a.C)))
    assert np.array_equal(y > 0, dz != 0)
    assert np.array_equal(dz[dz != 0], dy[dz != 0])


def test_refusals_launch_nothing():
    """Host-side checks: MPNN_E_SHAPE / MPNN_E_ARG, and n_pix <= 0 returns 0 with the outputs untouched."""
    import torch
    import hiputil as U
    lib = _hip.load()
    a = R.ActMap(np.random.default_rng(1), 2, 513, 'relu')                 # (buffers that would hold any C tried here)
    dv = Dev(a)
    out = U.Guarded(a.s.size); out.fill(NAN)
    red = U.Guarded(S * 2 * 513, torch.float64); red.fill(NAN)
    dyd = U.dev(a.s.reshape(-1))
    st = U.stream()

    def act(C_, shift=0, x=True):
        r = dv.act(x)
        r.C, r.shift = C_, shift
        return r

    def ctx(C_, s=True):
        c = dv.ctx(None, 1)
        c.bn.C = C_
        if not s:
            c.s = None
        return c

    for C_ in (0, 513):
        assert lib.mpnn_bn_relu_fwd(C.byref(act(C_)), out.ptr(), 1, st) == _hip.E_SHAPE
        assert lib.mpnn_bn_bwd_reduce(dyd.data_ptr(), C.byref(ctx(C_)), out.ptr(), red.ptr(), 1, st) == _hip.E_SHAPE
        assert lib.mpnn_bn_bwd_apply(out.ptr(), C.byref(ctx(C_)), 1, st) == _hip.E_SHAPE
    assert lib.mpnn_bn_relu_fwd(C.byref(act(16, shift=1)), out.ptr(), 1, st) == _hip.E_SHAPE
    ok = ctx(16)
    assert lib.mpnn_bn_relu_fwd(None, out.ptr(), 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_relu_fwd(C.byref(act(16, x=False)), out.ptr(), 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_relu_fwd(C.byref(act(16)), None, 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_reduce(None, C.byref(ok), out.ptr(), red.ptr(), 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_reduce(dyd.data_ptr(), None, out.ptr(), red.ptr(), 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_reduce(dyd.data_ptr(), C.byref(ctx(16, s=False)), out.ptr(), red.ptr(), 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_reduce(dyd.data_ptr(), C.byref(ok), None, red.ptr(), 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_reduce(dyd.data_ptr(), C.byref(ok), out.ptr(), None, 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_apply(None, C.byref(ok), 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_apply(out.ptr(), None, 1, st) == _hip.E_ARG
    assert lib.mpnn_bn_bwd_apply(out.ptr(), C.byref(ctx(16, s=False)), 1, st) == _hip.E_ARG
    for n_pix in (0, -3):
        assert lib.mpnn_bn_relu_fwd(C.byref(act(16)), out.ptr(), n_pix, st) == 0
        assert lib.mpnn_bn_bwd_reduce(dyd.data_ptr(), C.byref(ok), out.ptr(), red.ptr(), n_pix, st) == 0
        assert lib.mpnn_bn_bwd_apply(out.ptr(), C.byref(ok), n_pix, st) == 0
    torch.cuda.synchronize()
    assert np.isnan(out.get()).all() and np.isnan(red.get()).all() and out.guards_ok() and red.guards_ok()
