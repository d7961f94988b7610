"""GPU: mpnn_dropout_fwd / mpnn_dropout_bwd (csrc/dropout.hip) alone through the C ABI against tests/dropout_ref.py.

Cases (dropout_ref.KERNEL_CASES, a dozen): rows 1, 5, 128, 130; maps 16x16, 16x128, 4x6 (K = 24), 1x5 (K = 5: a quad tail),
3x2 (K = 6), 6x10 (K = 60); λ 1, 0.9, 0.5, 1e-3; both activation modes (batch statistics built by tests/hiputil.py: bn_dict, as
the exit-kernel tests build theirs); tables of 1 to 3 records with different n, seeds and leaves, launched with n_max / k_max
larger than any record.

  * the zero pattern of xd and of a non-accumulating dx is EXACTLY the reference mask, and those zeros are +0.0f; an
    accumulating dx keeps its bits where the element was dropped (a -0.0f among them);
  * kept values within the forward limit of the exit-kernel tests (2e-6 bound + 1e-6, tests/test_exit_gen_kernels.py) times
    1/λ; gradients within tests/activity_error_ref.py: grad_lim with bound = |dx| + |dxd| / λ;
  * guard words round every output intact; the same record at two table positions, a second launch with the same t: the same
    bits; t + 1: the mask moves, and is the reference's again;
  * λ = 1: xd is mpnn_bn_relu_fwd's output bit for bit; the refusals of mpnn_dropout_check and of the launchers.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import activity_error_ref as AR
import dropout_ref as R
from hiputil import DEV, Guarded, bn_dict, dev, stream
from lib import _hip

pytestmark = pytest.mark.gpu

MODES = {'identity': _hip.ACT_IDENTITY, 'batch': _hip.ACT_BN_BATCH}
fwd_lim = lambda bound: 2e-6 * bound + 1e-6            # (tests/test_exit_gen_kernels.py: forward values)
T0 = 5                                                # the step counter of the first launch


@functools.lru_cache(maxsize=None)
def reference(name, t):
    """(inputs, float64 activation and its bound, keep mask at step t): computed once per (case, t), shared, never written."""
    d = R.kernel_inputs(name)
    a, ab = R.activated(d)
    m = R.mask(d['seed'], t, d['leaf'], d['n'], d['K'], d['λ'])
    for v in (a, ab, m):
        v.setflags(write=False)
    return d, a, ab, m


class Rec:
    """One record on the device: guarded outputs, a step counter of its own."""

    def __init__(self, name, step, accumulate):
        d = self.d = R.kernel_inputs(name)
        n, K = d['n'], d['K']
        self.x = dev(d['x'])
        bn, cnt = (None, 1) if d['mode'] == 'identity' else bn_dict(d['x'], d['gamma'], d['beta'])
        self.bn = bn
        self.act = _hip.act(self.x, d['C'], MODES[d['mode']], 0, bn, cnt)
        self.dxd = dev(d['dxd'])
        self.xd, self.dx = Guarded(n * K), Guarded(n * K)
        self.xd.fill(np.nan)
        self.dx.fill(d['dx'] if accumulate else np.nan)
        self.step = step
        r = self.rec = _hip.DropoutArgs()
        r.a, r.HW, r.n = self.act, d['HW'], n
        r.seed_lo, r.seed_hi, r.leaf = d['seed'] & 0xFFFFFFFF, d['seed'] >> 32, d['leaf']
        r.thresh, r.inv_keep = R.thresh(d['λ']), float(R.inv_keep(d['λ']))
        r.step, r.xd, r.dxd, r.dx, r.accumulate = step.data_ptr(), self.xd.ptr(), self.dxd.data_ptr(), self.dx.ptr(), int(accumulate)
        self.accumulate = accumulate

    def outputs(self):
        assert self.xd.guards_ok() and self.dx.guards_ok(), self.d['name'] + ': written outside an output'
        n, K = self.d['n'], self.d['K']
        return self.xd.get().reshape(n, K).copy(), self.dx.get().reshape(n, K).copy()


def launch(recs, n_max=None, k_max=None, fwd=True, bwd=True):
    lib = _hip.load()
    for r in recs:
        assert lib.mpnn_dropout_check(C.byref(r.rec)) == 0
    tab = _hip.to_device_table([r.rec for r in recs], DEV)
    n_max = max(r.d['n'] for r in recs) if n_max is None else n_max
    k_max = max(r.d['K'] for r in recs) if k_max is None else k_max
    if fwd:
        _hip.check(lib.mpnn_dropout_fwd(tab.data_ptr(), len(recs), n_max, k_max, stream()), 'dropout_fwd')
    if bwd:
        _hip.check(lib.mpnn_dropout_bwd(tab.data_ptr(), len(recs), n_max, k_max, stream()), 'dropout_bwd')
    torch.cuda.synchronize()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def judge(rec, t):
    """xd and dx of a launched record against the reference at step t."""
    d, a, ab, m = reference(rec.d['name'], t)
    λ = d['λ']
    xd, dx = rec.outputs()
    name = d['name']
    # dropped: exact +0.0f; a kept element is zero only where the activation itself is (ReLU)
    assert (bits(xd)[~m] == 0).all(), name + ': a dropped element of xd is not +0.0f'
    a32 = R.activated(d, np.float32)[0]
    live = m & (np.abs(a) > fwd_lim(ab))               # (the float64 activation stands clear of zero: the kernel's does too)
    assert (xd[live] != 0).all(), name + ': a kept, active element of xd is zero'
    err = np.abs(xd.astype(np.float64) - R.layer(a, m, λ))
    lim = fwd_lim(ab) / λ
    print('%-12s xd  worst error / limit %.3g; kept %.4f (λ = %g)' % (name, float((err / lim).max()), m.mean(), λ))
    assert (err <= lim).all(), name
    if d['mode'] == 'identity':                        # the float32 stand-in: one rounded product, the same bits
        assert np.array_equal(bits(xd), bits(R.layer(a32, m, λ, np.float32))), name
    if rec.accumulate:
        ref, bound = R.layer_bwd(d['dxd'], m, λ, d['dx'])
        assert (bits(dx)[~m] == bits(d['dx'])[~m]).all(), name + ': a dropped element of an accumulating dx changed'
    else:
        ref, bound = R.layer_bwd(d['dxd'], m, λ)
        assert (bits(dx)[~m] == 0).all(), name + ': a dropped element of dx is not +0.0f'
        assert (dx[m] != 0).all(), name + ': a kept element of dx is zero'          # (dxd is N(0, 1): never 0)
    err = np.abs(dx.astype(np.float64) - ref)
    lim = AR.grad_lim(bound)
    print('%-12s dx  worst error / limit %.3g' % (name, float((err / lim).max())))
    assert (err <= lim).all(), name
    return xd, dx


@pytest.mark.parametrize('table', R.KERNEL_TABLES, ids=lambda t: '+'.join(t))
@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
def test_tables_against_the_reference(table, accumulate):
    step = torch.tensor([T0], dtype=torch.int32, device=DEV)
    recs = [Rec(name, step, accumulate) for name in table]
    # n_max / k_max beyond every record (they only size the grid)
    launch(recs, n_max=max(r.d['n'] for r in recs) + 3, k_max=max(r.d['K'] for r in recs) + 5)
    for r in recs:
        judge(r, T0)
    assert {R.CASE[name][0] for t in R.KERNEL_TABLES for name in t} == set(R.CASE)


def test_place_in_the_table_grid_and_relaunch_do_not_matter_but_the_step_does():
    step = torch.tensor([T0], dtype=torch.int32, device=DEV)
    alone = Rec('ship', step, False)
    launch([alone])
    want = judge(alone, T0)
    # the same record at two table positions, between others, with another grid
    a, b = Rec('ship', step, False), Rec('ship', step, False)
    launch([a, Rec('k5-tail', step, False), b], n_max=1000, k_max=4096)
    for r in (a, b):
        got = r.outputs()
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(got, want))
    # a second launch with the same t: the same bits
    launch([alone])
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(alone.outputs(), want))
    # a smaller grid than the record (n_max, k_max below it): every element is still walked
    small = Rec('ship', step, False)
    launch([small], n_max=1, k_max=4)
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(small.outputs(), want))
    # t + 1, read from DEVICE memory by the same records: the mask moves, and is the reference's
    step.fill_(T0 + 1)
    launch([alone])
    moved = judge(alone, T0 + 1)
    m0, m1 = reference('ship', T0)[3], reference('ship', T0 + 1)[3]
    frac = float((m0 != m1).mean())
    assert abs(frac - 0.5) < 0.02, frac                      # (2 λ (1 - λ) at λ = 0.5, 32 768 elements)
    assert not np.array_equal(bits(moved[0]), bits(want[0]))
    # another leaf, another seed: other masks
    for field, value in (('leaf', 4), ('seed_lo', 77), ('seed_hi', 1)):
        other = Rec('ship', step, False)
        setattr(other.rec, field, value)
        launch([other])
        assert ((other.outputs()[1] == 0) != (moved[1] == 0)).mean() > 0.4, field


@pytest.mark.parametrize('name', ['keep-all', 'ship', 'wide', 'k5-tail', 'k24'])
def test_lambda_one_is_bn_relu_fwd_bit_for_bit(name):
    """With thresh == 0 and inv_keep == 1 the forward launch materialises the activation: mpnn_bn_relu_fwd's bits."""
    lib = _hip.load()
    step = torch.tensor([T0], dtype=torch.int32, device=DEV)
    r = Rec(name, step, False)
    r.rec.thresh, r.rec.inv_keep = 0, 1.0
    launch([r], bwd=False)
    d = r.d
    y = torch.full((d['n'] * d['K'],), float('nan'), device=DEV)
    _hip.check(lib.mpnn_bn_relu_fwd(C.byref(r.act), y.data_ptr(), d['n'] * d['HW'], stream()), 'bn_relu_fwd')
    torch.cuda.synchronize()
    assert r.xd.guards_ok()
    assert np.array_equal(bits(r.xd.get()), bits(y.cpu().numpy()))


def test_refusals():
    lib = _hip.load()
    step = torch.tensor([T0], dtype=torch.int32, device=DEV)
    good = Rec('k24', step, False)
    assert lib.mpnn_dropout_check(C.byref(good.rec)) == 0
    assert lib.mpnn_dropout_check(None) == _hip.E_ARG

    def refused(code, **fields):
        r = Rec('k24', step, False)
        for k, v in fields.items():
            obj, _, leaf = k.rpartition('__')
            setattr(getattr(r.rec, obj) if obj else r.rec, leaf, v)
        assert lib.mpnn_dropout_check(C.byref(r.rec)) == code, fields
    refused(_hip.E_SHAPE, a__shift=1)
    refused(_hip.E_SHAPE, a__C=0)
    refused(_hip.E_SHAPE, a__C=513)
    refused(_hip.E_SHAPE, n=1 << 20, HW=1 << 10)
    refused(_hip.E_ARG, n=0)
    refused(_hip.E_ARG, HW=0)
    refused(_hip.E_ARG, step=None)
    refused(_hip.E_ARG, inv_keep=float('inf'))
    refused(_hip.E_ARG, inv_keep=float('nan'))
    refused(_hip.E_ARG, inv_keep=0.5)
    refused(_hip.E_ARG, accumulate=2)
    refused(_hip.E_ARG, xd=None)
    refused(_hip.E_ARG, dx=None)
    refused(_hip.E_ARG, a__mode=_hip.ACT_BN_MOVING)
    refused(_hip.E_ARG, a__mode=_hip.ACT_RELU)
    refused(_hip.E_ARG, a__sum=None)
    refused(_hip.E_ARG, a__nslot=0)
    tab = _hip.to_device_table([good.rec], DEV)
    for fn in (lib.mpnn_dropout_fwd, lib.mpnn_dropout_bwd):
        assert fn(None, 1, 5, 24, stream()) == _hip.E_ARG
        assert fn(tab.data_ptr(), 0, 5, 24, stream()) == _hip.E_ARG
        assert fn(tab.data_ptr(), 1, 0, 24, stream()) == _hip.E_ARG
        assert fn(tab.data_ptr(), 1, 5, 0, stream()) == _hip.E_ARG
        assert fn(tab.data_ptr(), 70000, 5, 24, stream()) == _hip.E_SHAPE
        assert fn(tab.data_ptr(), 1, 1 << 20, 1 << 10, stream()) == _hip.E_SHAPE
    torch.cuda.synchronize()
    assert np.isnan(good.xd.get()).all() and np.isnan(good.dx.get()).all() and good.xd.guards_ok() and good.dx.guards_ok()
