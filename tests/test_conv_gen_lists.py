"""Sample lists on the general forward conv kernel (csrc/conv_gen.hip: mpnn_msconv_fwd_gen / mpnn_msconv_fwd_hw with
mpnn_conv_fwd_args.idx / cnt), through the C ABI, on the GPU.

One forward conv per case, launched without a list and then with lists of 0, 1, 5, n - 1 and n samples (n = 7: no count
but 0 is a multiple of the two or four images of a tile).  `out` and `pool_out` lie between sentinel guards and are filled
with NaN before every launch:

  * the rows of the listed images are BIT-equal to the launch without a list (the slot an image takes in a tile changes
    nothing of its arithmetic), in whatever order the list names them;
  * the rows of every other image are still NaN, a count of 0 writes nothing, no guard is touched;
  * the count is read on the device: the same record launched again after only the count tensor changed writes the other
    set of rows;
  * one of idx / cnt alone, a list with out_sum, a list with batch statistics: MPNN_E_ARG.

The maps give all four tile shapes (16x16 and 8x8: 8x8 pixels of one image; 8x4 and 4x8: two images; 4x4 and 2x2: four)
and tiles that hang over the bottom / right edge (12x20, 6x10, 2x2); the filters 1, 2, 3, 5, 7 per side, clipped ones
(4x4 on the 4x4 map, 4x7 on the 4x8 map) and even ones (asymmetric SAME padding); one and two 64-channel output groups."""
import ctypes as C

import numpy as np
import pytest

from lib import _hip
from test_conv_hw import _act, _fn, _id, _seed

pytestmark = pytest.mark.gpu

N = 7
COUNTS = (0, 1, 5, N - 1, N)

# (entry points, H, W, Cin, act mode, shift, Cv, Cout, horz kh x kw, vert kvh x kvw, pool)
CASES = [
    ('gen', 16, 16, 3, 'img', 1, 0, 16, (3, 3), None, True),
    ('hw', 16, 16, 16, 'moving', 0, 16, 64, (5, 5), (5, 5), True),
    ('gen', 16, 16, 16, 'moving', 0, 16, 16, (7, 7), (3, 3), False),
    ('hw', 16, 16, 3, 'img', 1, 0, 16, (1, 1), None, False),
    ('gen', 8, 8, 16, 'id', 0, 16, 64, (2, 2), (1, 1), True),
    ('gen', 4, 4, 48, 'moving', 0, 16, 128, (4, 4), (5, 5), False),     # (supp 5 clipped to the 4x4 map; two channel groups)
    ('hw', 4, 4, 16, 'moving', 0, 0, 16, (1, 1), None, True),
    ('hw', 4, 4, 48, 'moving', 0, 16, 128, (4, 4), (5, 5), True),
    ('gen', 16, 16, 16, 'moving', 0, 16, 64, (5, 5), (5, 5), True),
    ('hw', 8, 4, 16, 'moving', 0, 16, 16, (3, 3), (3, 3), True),
    ('hw', 4, 8, 32, 'moving', 0, 0, 64, (4, 7), None, False),
    ('hw', 12, 20, 3, 'img', 2, 0, 16, (7, 7), None, True),
    ('hw', 6, 10, 16, 'moving', 0, 16, 128, (5, 5), (5, 5), True),
    ('hw', 2, 2, 16, 'moving', 0, 16, 16, (2, 2), (3, 3), True),        # (pooled to 1x1)
]


class Conv:
    """One forward conv record on N images with NaN-poisoned, guarded outputs."""

    def __init__(self, case, n=N):
        import hiputil as U
        self.fam, H, W, Cin, mode, shift, Cv, Cout, self.kh, self.kv, pool = case
        rng = np.random.default_rng(_seed(case))
        self.n, self.row, self.prow = n, H * W * Cout, (H // 2) * (W // 2) * Cout
        rec = self.rec = _hip.ConvFwdArgs()
        rec.a, _, self.keep = _act(rng, n, H, W, Cin, mode, shift)
        wh = U.dev(U.f32(rng.standard_normal(self.kh + (Cin, Cout)) * 0.2)[0])
        b = U.dev(U.f32(rng.standard_normal(Cout) * 0.1)[0])
        rec.wa_pack, rec.bias = wh.data_ptr(), b.data_ptr()
        self.keep += [wh, b]
        if Cv:
            v = U.dev(U.f32(rng.standard_normal((n, H, W, Cv)))[0])
            wv = U.dev(U.f32(rng.standard_normal(self.kv + (Cv, Cout)) * 0.2)[0])
            rec.v, rec.Cv, rec.wv_pack = v.data_ptr(), Cv, wv.data_ptr()
            self.keep += [v, wv]
        self.out = U.Guarded(n * self.row)
        self.pool = U.Guarded(n * self.prow) if pool else None
        rec.out = self.out.ptr()
        rec.pool_out = self.pool.ptr() if pool else None
        rec.n, rec.H, rec.W, rec.Cout = n, H, W, Cout

    def launch(self, expect=0):
        """Poison the outputs, launch, return (out rows, pool rows or None)."""
        import torch
        import hiputil as U
        self.out.fill(float('nan'))
        if self.pool is not None:
            self.pool.fill(float('nan'))
        rc = _fn(_hip.load(), 'fwd', self.fam)(C.byref(self.rec), *self.kh, *(self.kv or (0, 0)), U.stream())
        torch.cuda.synchronize()
        assert rc == expect, rc
        assert self.out.guards_ok() and (self.pool is None or self.pool.guards_ok())
        return (self.out.get().reshape(self.n, self.row),
                self.pool.get().reshape(self.n, self.prow) if self.pool is not None else None)

    def set_list(self, idx, cnt):
        """idx, cnt: device int32 tensors (or None, None)."""
        self.rec.idx = idx.data_ptr() if idx is not None else None
        self.rec.cnt = cnt.data_ptr() if cnt is not None else None


def _check(got, dense, listed, n, what):
    """Rows of the listed images equal the dense launch's bits; every other row is still NaN."""
    for g, d, name in zip(got, dense, ('out', 'pool_out')):
        if d is None:
            continue
        rest = np.setdiff1d(np.arange(n), listed)
        assert np.isfinite(d).all(), name
        assert np.array_equal(g[listed], d[listed]), '%s: %s rows of the listed images differ from the dense launch' % (what, name)
        assert np.isnan(g[rest]).all(), '%s: %s rows of images that are not listed were written' % (what, name)


@pytest.mark.parametrize('case', CASES, ids=list(map(_id, CASES)))
def test_listed_rows_equal_the_dense_launch_and_the_rest_is_untouched(case):
    import torch
    import hiputil as U
    cv = Conv(case)
    dense = cv.launch()
    assert np.isfinite(dense[0]).all() and (dense[1] is None or np.isfinite(dense[1]).all())
    rng = np.random.default_rng(_seed(case) + 1)
    cnt = torch.zeros(1, dtype=torch.int32, device=U.DEV)
    for c in COUNTS:
        perm = rng.permutation(N)
        idx = U.dev(perm.astype(np.int32), torch.int32)
        cnt.fill_(c)
        cv.set_list(idx, cnt)
        got = cv.launch()
        _check(got, dense, perm[:c], N, 'count %d' % c)
        if c == 0:
            assert np.isnan(got[0]).all() and (got[1] is None or np.isnan(got[1]).all())
        if c == N:                                            # a permutation of every image: the dense launch everywhere
            assert np.array_equal(got[0], dense[0]) and (got[1] is None or np.array_equal(got[1], dense[1]))


@pytest.mark.parametrize('case', CASES, ids=list(map(_id, CASES)))
def test_the_count_is_read_on_the_device(case):
    """The same record, launched twice; only the device count tensor changes in between."""
    import torch
    import hiputil as U
    cv = Conv(case)
    dense = cv.launch()
    perm = np.random.default_rng(_seed(case) + 2).permutation(N)
    idx = U.dev(perm.astype(np.int32), torch.int32)
    cnt = torch.full((1,), 5, dtype=torch.int32, device=U.DEV)
    cv.set_list(idx, cnt)
    _check(cv.launch(), dense, perm[:5], N, 'count 5')
    cnt.fill_(2)
    _check(cv.launch(), dense, perm[:2], N, 'count 2 (the record unchanged)')
    cnt.fill_(N - 1)
    _check(cv.launch(), dense, perm[:N - 1], N, 'count n - 1 (the record unchanged)')


@pytest.mark.parametrize('fam', ['gen', 'hw'])
def test_refusals(fam):
    import torch
    import hiputil as U
    E_ARG = _hip.E_ARG
    idx = U.dev(np.arange(N, dtype=np.int32), torch.int32)
    cnt = torch.full((1,), 3, dtype=torch.int32, device=U.DEV)
    mk = lambda mode: Conv((fam, 8, 8, 16, mode, 0, 16, 16, (3, 3), (3, 3), True))
    cv = mk('moving')
    dense = cv.launch()
    for only in ((idx, None), (None, cnt)):                   # one of the two alone
        cv.set_list(*only)
        got = cv.launch(expect=E_ARG)
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all()
    cv.set_list(idx, cnt)                                     # with the BatchNorm sums of a training step
    osum = torch.zeros(_hip.BN_SLOTS * 2 * 16, dtype=torch.float64, device=U.DEV)
    cv.rec.out_sum, cv.rec.out_nslot = osum.data_ptr(), 4
    got = cv.launch(expect=E_ARG)
    assert np.isnan(got[0]).all() and not osum.any()
    cv.rec.out_sum = None
    _check(cv.launch(), dense, np.arange(3), N, 'the record without out_sum')
    cb = mk('batch')                                          # with batch statistics
    cb.launch()
    cb.set_list(idx, cnt)
    got = cb.launch(expect=E_ARG)
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all()
