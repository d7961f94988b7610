"""GPU: mpnn_label_map (csrc/label_map.hip) through the C ABI against tests/superclass_ref.py.

Sizes (superclass_ref.SIZES): (n_cls, n_sup) = (1,1), (2,1), (10,2), (10,3), (17,16), (100,20), (1024,17), (16,1024); around
the kernel's column tile LM_S = 16: n_sup = 15, 16, 17 and 33 (three tiles, the last of one column); around its LDS chunk of
LM_C = 64 classes: n_cls = 63, 64, 65 and 129 (three chunks, the last of one class).  Rows (superclass_ref.NS): n = 1, 5, 63,
64, 65, 129 and, around the row tile LM_R = 16, n = 15, 16, 17 -- each as a prefix of the same 129 rows, in buffers of n rows,
and once with n < n_max.  A table of three records with different n (one of them 0) and different widths.

  * one-hot labels on finite non-zero maps: exactly the label's row of w_cls; dyadic labels and maps whose products and
    partial sums are exact in fp32: exactly the float64 product;
  * soft labels: |got - ref| <= (n_cls + 1) 2^-24 sum_c |y_c w_cs|, the rounding of an n_cls-long fmaf chain;
  * 64 guard words on each side of every output, and the rows beyond n, stay as they were;
  * sample 0 gives the same bits with n = 1 and n = 129, and as record 0 or record 2 of a table; two launches give the
    same bits; nothing is clamped (0 * inf is nan); the refusals return their codes with the outputs unwritten.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import superclass_ref as R
from lib import _hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
SENTINEL = np.float32(-1.2345678e25)


class Record:
    """One map's record: labels and map on the device and a guarded output of `cap` rows."""

    def __init__(self, y, w, n=None, cap=None):
        self.n = len(y) if n is None else n
        self.cap = max(self.n, 1) if cap is None else cap          # (rows the buffer holds: those beyond n must stay untouched)
        self.n_cls, self.n_sup = w.shape
        self.y = torch.from_numpy(np.array(y)).to(DEV)             # (copies: the shared inputs are read-only)
        self.w = torch.from_numpy(np.array(w)).to(DEV)
        self.buf = torch.full((self.cap * self.n_sup + 2 * GUARD,), float(SENTINEL), device=DEV)
        self.rec = _hip.LabelMapArgs()
        self.rec.y, self.rec.w_cls, self.rec.y_sup = self.y.data_ptr(), self.w.data_ptr(), self.buf.data_ptr() + 4 * GUARD
        self.rec.n, self.rec.n_cls, self.rec.n_sup = self.n, self.n_cls, self.n_sup

    def result(self):
        """[n, n_sup] as int32 bit patterns, after checking the guards and the rows beyond n."""
        bits = self.buf.cpu().numpy().view(np.int32)
        sent = SENTINEL.view(np.int32)
        used = self.n * self.n_sup
        assert (bits[:GUARD] == sent).all() and (bits[GUARD + used:] == sent).all(), 'written outside y_sup[0 .. n * n_sup)'
        return bits[GUARD:GUARD + used].reshape(self.n, self.n_sup).copy()

    def unwritten(self):
        return bool((self.buf.cpu().numpy().view(np.int32) == SENTINEL.view(np.int32)).all())


def launch(records, n_max=None, n_sup_max=None):
    lib = _hip.load()
    for r in records:
        assert lib.mpnn_label_map_check(C.byref(r.rec)) == 0
    tab = _hip.to_device_table([r.rec for r in records], DEV)
    rc = lib.mpnn_label_map(tab.data_ptr(), len(records), max(r.n for r in records) if n_max is None else n_max,
                            max(r.n_sup for r in records) if n_sup_max is None else n_sup_max, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def f32(bits):
    return bits.view(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(kind, n_cls, n_sup):
    """(y, w, float64 reference, bound) of one case at N_MAX rows: computed once, shared, never written."""
    y, w = R.kernel_input(kind, n_cls, n_sup)
    ref, bnd = R.bound(y, w)
    for a in (y, w, ref, bnd):
        a.setflags(write=False)
    return y, w, ref, bnd


@pytest.mark.parametrize('n_cls,n_sup', R.kernel_cases())
def test_against_the_reference_at_every_n(n_cls, n_sup):
    full = {}
    for kind in ('onehot', 'dyadic', 'soft'):
        y, w, ref, bnd = inputs(kind, n_cls, n_sup)
        by_n = {}
        for n in R.NS:
            r = Record(y[:n], w)
            assert launch([r]) == 0
            got = by_n[n] = r.result()
            if kind == 'onehot':                              # exactly the selected row of the map
                assert np.array_equal(got, w[np.argmax(y[:n], 1)].view(np.int32)), (kind, n)
            elif kind == 'dyadic':                            # every partial sum exact: the float64 product, to the bit
                assert np.array_equal(f32(got).astype(np.float64), ref[:n]), (kind, n)
            else:
                err = np.abs(f32(got).astype(np.float64) - ref[:n])
                print('label_map %d>%d soft n=%d: worst |got - ref| / bound = %.3f' % (n_cls, n_sup, n, (err / bnd[:n]).max()))
                assert (err <= bnd[:n]).all(), (kind, n, float((err / bnd[:n]).max()))
        full[kind] = by_n[R.N_MAX]
        for n in R.NS:                                        # a row's bits do not depend on n (sample 0: n = 1 and n = 129)
            assert np.array_equal(by_n[n], full[kind][:n]), (kind, n)
    # n < n_max and n_sup < n_sup_max: the grid is larger than the record, rows and columns beyond it are not computed
    y, w, _, _ = inputs('soft', n_cls, n_sup)
    r = Record(y[:5], w, cap=R.N_MAX)
    assert launch([r], n_max=R.N_MAX, n_sup_max=min(1024, n_sup + 17)) == 0
    assert np.array_equal(r.result(), full['soft'][:5])


def test_table_of_three_records_with_different_n_and_widths():
    ya, wa, _, _ = inputs('soft', 10, 3)
    yb, wb, _, _ = inputs('soft', 100, 20)
    yc, wc, _, _ = inputs('soft', 17, 16)
    alone = [Record(ya[:1], wa), Record(yc[:1], wc)]
    for r in alone:
        assert launch([r]) == 0
    # record 0: 10>3, n = 129; record 1: 100>20 with n = 0 in a buffer of 5 rows; record 2: 17>16, n = 37 in a buffer of 129
    recs = [Record(ya, wa), Record(yb[:5], wb, n=0, cap=5), Record(yc[:37], wc, cap=R.N_MAX)]
    assert launch(recs) == 0
    a, b, c = (r.result() for r in recs)
    assert recs[1].unwritten() and b.size == 0
    for got, y, w in ((a, ya, wa), (c, yc[:37], wc)):
        ref, bnd = R.bound(y, w)
        assert (np.abs(f32(got).astype(np.float64) - ref) <= bnd).all()
    assert np.array_equal(a[:1], alone[0].result())           # sample 0 with n = 129 in a table and alone with n = 1
    # the same rows as record 2 and as record 0, alone: the record's place in the table does not matter
    swapped = [Record(yc[:37], wc), Record(yb[:5], wb), Record(ya, wa)]
    assert launch(swapped) == 0
    assert np.array_equal(swapped[0].result(), c) and np.array_equal(swapped[2].result(), a)
    assert np.array_equal(swapped[0].result()[:1], alone[1].result())
    ref_b, bnd_b = R.bound(yb[:5], wb)
    assert (np.abs(f32(swapped[1].result()).astype(np.float64) - ref_b) <= bnd_b).all()


def test_two_launches_give_the_same_bits():
    y, w, _, _ = inputs('soft', 1024, 17)
    a, b = Record(y, w), Record(y, w)
    assert launch([a]) == 0 and launch([b]) == 0
    assert np.array_equal(a.result(), b.result())
    assert launch([a]) == 0                                    # ... and over its own earlier result
    assert np.array_equal(a.result(), b.result())


def test_nothing_is_skipped_or_clamped():
    """A zero label times an infinite weight is nan, as in a matmul; an infinite weight under a non-zero label is inf."""
    y = np.eye(4, dtype=np.float32)[[0, 1, 2]]
    w = np.ones((4, 3), np.float32)
    w[1, 0], w[3, 2] = np.inf, -np.inf
    r = Record(y, w)
    assert launch([r]) == 0
    got = f32(r.result())
    assert np.isnan(got[0, 0]) and got[1, 0] == np.inf and np.isnan(got[2, 0])       # column 0: inf under label 1
    assert (got[:, 1] == 1).all() and np.isnan(got[:, 2]).all()                        # column 2: -inf under a label nobody has


def test_refusals_leave_the_outputs_unwritten():
    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    y, w, ref, bnd = inputs('soft', 10, 3)
    r = Record(y[:5], w)
    tab = _hip.to_device_table([r.rec], DEV)
    assert lib.mpnn_label_map(None, 1, 5, 3, st) == _hip.E_ARG
    assert lib.mpnn_label_map(tab.data_ptr(), 0, 5, 3, st) == _hip.E_ARG
    assert lib.mpnn_label_map(tab.data_ptr(), -1, 5, 3, st) == _hip.E_ARG
    assert lib.mpnn_label_map(tab.data_ptr(), 1, 0, 3, st) == _hip.E_ARG
    assert lib.mpnn_label_map(tab.data_ptr(), 1, 5, 0, st) == _hip.E_SHAPE
    assert lib.mpnn_label_map(tab.data_ptr(), 1, 5, _hip.LABEL_MAP_MAX_SUP + 1, st) == _hip.E_SHAPE
    torch.cuda.synchronize()
    assert r.unwritten()

    def edited(**kw):
        rec = _hip.LabelMapArgs.from_buffer_copy(r.rec)
        for k, v in kw.items():
            setattr(rec, k, v)
        return lib.mpnn_label_map_check(C.byref(rec))
    assert lib.mpnn_label_map_check(None) == _hip.E_ARG
    for kw in (dict(y=None), dict(w_cls=None), dict(y_sup=None), dict(n=-1)):
        assert edited(**kw) == _hip.E_ARG, kw
    for kw in (dict(n_cls=0), dict(n_cls=_hip.LABEL_MAP_MAX_CLS + 1), dict(n_sup=0), dict(n_sup=_hip.LABEL_MAP_MAX_SUP + 1)):
        assert edited(**kw) == _hip.E_SHAPE, kw
    assert edited(n=0) == 0 and edited(n_cls=_hip.LABEL_MAP_MAX_CLS, n_sup=_hip.LABEL_MAP_MAX_SUP) == 0
    assert launch([r]) == 0                                    # ... and the same record runs once the arguments are right
    assert (np.abs(f32(r.result()).astype(np.float64) - ref[:5]) <= bnd[:5]).all()
