"""The 1x1 kernels of csrc/conv_nhwc.hip -- mpnn_conv_nhwc_fwd / _dgrad / _wgrad with supp = 1: two MFMA GEMM kernels and one
weight-gradient kernel -- alone, through the C ABI, on the GPU, against float64 contractions over the activation as the
kernel sees it (tests/small_launch_ref.py).

Channel pairs with 1, 15, 17, 18, 255 and 256 channels on either operand (the scalar path where K % 4 != 0, the 16-byte
path with a part-filled last block of 16, one either side of a tile, both maxima); pixel counts around 16, 64 and 1024
(the weight gradient's step from one pixel split to two) as ragged n x H x W, and one count beyond each grid cap; the
activation on load in all its modes -- identity, plain ReLU, batch statistics over 1, 3 and 8 slots with the unused
slots NaN, moving averages; the input gradient with and without relu_src, which carries exact +0 and -0.

out and dx are NaN-filled between guards; dw and db sit between guards, once from zero and once from a known prior, and
db is added once, not once per input-channel tile.  Limits per element, of the sum of the absolute values of its terms:
2e-6 (+ 1e-6) for out and dx, 4e-6 for dw and db (tests/test_conv_hw.py).  Forward and input gradient give equal bits
twice; the weight gradient where M <= 1024 (one workgroup per tile).
"""
import ctypes as C

import numpy as np
import pytest

from lib import _hip
import small_launch_ref as R
from test_bn_launches import Dev, _close, _same_bits, NAN

pytestmark = pytest.mark.gpu


def _fwd(dv, d, case, wd=None, bd=None):
    import torch
    U = dv.U
    n, H, W, ci, co = case[:5]
    wd = U.dev(d['w']) if wd is None else wd
    bd = U.dev(d['b']) if bd is None else bd
    out = U.Guarded(n * H * W * co); out.fill(NAN)
    r = _hip.ConvNhwcFwdArgs()
    r.a, r.w, r.bias, r.out = dv.act(), wd.data_ptr(), bd.data_ptr(), out.ptr()
    r.n, r.H, r.W, r.Cout, r.supp = n, H, W, co, 1
    _hip.check(_hip.load().mpnn_conv_nhwc_fwd(C.byref(r), U.stream()), 'conv_nhwc_fwd')
    torch.cuda.synchronize()
    assert out.guards_ok()
    return out.get().reshape(-1, co)


def _wgrad(dv, d, case, prior):
    import torch
    U = dv.U
    n, H, W, ci, co = case[:5]
    gd = U.dev(d['g'])
    dw, db = U.Guarded(ci * co), U.Guarded(co)
    dw.fill(d['dw0'] if prior else 0.0); db.fill(d['db0'] if prior else 0.0)
    r = _hip.ConvNhwcWgradArgs()
    r.a, r.g, r.dw, r.db = dv.act(), gd.data_ptr(), dw.ptr(), db.ptr()
    r.n_split, r.n, r.H, r.W, r.Cout, r.supp = 1, n, H, W, co, 1
    _hip.check(_hip.load().mpnn_conv_nhwc_wgrad(C.byref(r), U.stream()), 'conv_nhwc_wgrad')
    torch.cuda.synchronize()
    assert dw.guards_ok() and db.guards_ok()
    return dw.get().reshape(ci, co), db.get()


def _dgrad(d, case):
    import torch
    import hiputil as U
    n, H, W, cg, ci, masked = case
    gd, wd = U.dev(d['g']), U.dev(d['w'])
    sd = U.dev(d['src'].s) if masked else None
    dx = U.Guarded(n * H * W * ci); dx.fill(NAN)
    r = _hip.ConvNhwcDgradArgs()
    r.g, r.Cg, r.w, r.relu_src, r.dx = gd.data_ptr(), cg, wd.data_ptr(), _hip.ptr(sd), dx.ptr()      # (scratch stays NULL)
    r.n, r.H, r.W, r.Cin, r.supp = n, H, W, ci, 1
    _hip.check(_hip.load().mpnn_conv_nhwc_dgrad(C.byref(r), U.stream()), 'conv_nhwc_dgrad')
    torch.cuda.synchronize()
    assert dx.guards_ok()
    return dx.get().reshape(-1, ci)


@pytest.mark.parametrize('case', R.CONV_CASES, ids=list(map(R.case_id, R.CONV_CASES)))
def test_conv1x1_fwd_vs_float64(case):
    d = R.conv_inputs(case)
    dv = Dev(d['a'])
    out = _fwd(dv, d, case)
    want, bound = R.conv_fwd_ref(d)
    _close(out, want, bound, what='out')
    assert _same_bits(out, _fwd(dv, d, case))


@pytest.mark.parametrize('case', R.CONV_CASES, ids=list(map(R.case_id, R.CONV_CASES)))
def test_conv1x1_wgrad_vs_float64(case):
    d = R.conv_inputs(case)
    dv = Dev(d['a'])
    want_w, bound_w, want_b, bound_b = R.conv_wgrad_ref(d)
    dw, db = _wgrad(dv, d, case, False)
    _close(dw, want_w, bound_w, rel=R.REL_W, what='dw')
    _close(db, want_b, bound_b, rel=R.REL_W, what='db')
    if d['M'] <= 1024:
        dw2, db2 = _wgrad(dv, d, case, False)
        assert _same_bits(dw, dw2) and _same_bits(db, db2)
    dw, db = _wgrad(dv, d, case, True)
    _close(dw, d['dw064'] + want_w, bound_w + np.abs(d['dw064']), rel=R.REL_W, what='dw')
    _close(db, d['db064'] + want_b, bound_b + np.abs(d['db064']), rel=R.REL_W, what='db')


@pytest.mark.parametrize('case', R.DGRAD_CASES, ids=list(map(R.case_id, R.DGRAD_CASES)))
def test_conv1x1_dgrad_vs_float64(case):
    d = R.dgrad_inputs(case)
    dx = _dgrad(d, case)
    want, bound = R.conv_dgrad_ref(d)
    _close(dx, want, bound, what='dx')
    if d['src'] is not None:
        assert not dx[d['src'].planted].any() and np.array_equal(dx[~d['src'].on], 0 * dx[~d['src'].on])
    assert _same_bits(dx, _dgrad(d, case))


@pytest.mark.parametrize('case', R.IDENT_CASES, ids=list(map(R.case_id, R.IDENT_CASES)))
def test_conv1x1_with_the_identity_matrix_gives_the_bits_of_bn_relu_fwd(case):
    """w = I and a zero bias: the MFMA adds exact zeros to the one live product, so out is the activation itself, with
    the bits mpnn_bn_relu_fwd materialises from the same mpnn_act."""
    n, H, W, C_, act = case
    a = R.act_of(np.random.default_rng(R.seed(case)), n * H * W, C_, act)
    dv = Dev(a)
    out = _fwd(dv, None, (n, H, W, C_, C_), wd=dv.U.dev(np.eye(C_, dtype=np.float32)), bd=dv.U.dev(np.zeros(C_, np.float32)))
    assert _same_bits(out, dv.relu_fwd())


def test_refusals_launch_nothing():
    import torch
    import hiputil as U
    lib = _hip.load()
    st = U.stream()
    buf = torch.full((257 * 257,), 1.0, device=U.DEV)                      # (would hold any operand tried here)
    out = U.Guarded(257 * 257); out.fill(NAN)
    p, o = buf.data_ptr(), out.ptr()

    def fwd(ci=16, co=16, supp=1, shift=0, n=1, **null):
        r = _hip.ConvNhwcFwdArgs()
        r.a = _hip.act(buf, ci, _hip.ACT_IDENTITY, shift)
        r.w, r.bias, r.out = p, p, o
        r.n, r.H, r.W, r.Cout, r.supp = n, 1, 1, co, supp
        for k in null:
            setattr(r.a if k == 'x' else r, k, None)
        return lib.mpnn_conv_nhwc_fwd(C.byref(r), st)

    def wgrad(ci=16, co=16, supp=1, shift=0, n=1, **null):
        r = _hip.ConvNhwcWgradArgs()
        r.a = _hip.act(buf, ci, _hip.ACT_IDENTITY, shift)
        r.g, r.dw, r.db = p, o, o
        r.n_split, r.n, r.H, r.W, r.Cout, r.supp = 1, n, 1, 1, co, supp
        for k in null:
            setattr(r.a if k == 'x' else r, k, None)
        return lib.mpnn_conv_nhwc_wgrad(C.byref(r), st)

    def dgrad(cg=16, ci=16, supp=1, n=1, **null):
        r = _hip.ConvNhwcDgradArgs()
        r.g, r.Cg, r.w, r.relu_src, r.dx = p, cg, p, p, o
        r.n, r.H, r.W, r.Cin, r.supp = n, 1, 1, ci, supp
        for k in null:
            setattr(r, k, None)
        return lib.mpnn_conv_nhwc_dgrad(C.byref(r), st)

    for f in (fwd, wgrad, dgrad):
        for bad in (0, 257):
            assert f(bad, 16) == _hip.E_SHAPE and f(16, bad) == _hip.E_SHAPE
        assert f(supp=2) == _hip.E_SHAPE
        assert f(n=0) == 0
    assert fwd(shift=1) == _hip.E_SHAPE and wgrad(shift=1) == _hip.E_SHAPE
    for k in ('x', 'w', 'bias', 'out'):
        assert fwd(**{k: 1}) == _hip.E_ARG, k
    for k in ('x', 'g', 'dw', 'db'):
        assert wgrad(**{k: 1}) == _hip.E_ARG, k
    for k in ('g', 'w', 'dx'):
        assert dgrad(**{k: 1}) == _hip.E_ARG, k
    assert lib.mpnn_conv_nhwc_fwd(None, st) == lib.mpnn_conv_nhwc_wgrad(None, st) == lib.mpnn_conv_nhwc_dgrad(None, st) == _hip.E_ARG
    torch.cuda.synchronize()
    assert np.isnan(out.get()).all() and out.guards_ok()
