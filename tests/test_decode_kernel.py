"""GPU: mpnn_decode_u8 through the C ABI -- dst[i] = lut[src[i]], compared as bit patterns.

  * the table is 256 random float32 bit patterns with -0.0, inf, a denormal and a NaN among them (a lookup copies bits);
  * counts around every boundary of the kernel (the 16-element groups, the 256-thread workgroup, the 4 x 256 groups of one
    workgroup pass), one CIFAR chunk of 200 images and 3 * 2^20 + 5 elements (several passes of many workgroups);
  * every source offset 0 .. 15 bytes crossed with every destination offset 0 .. 3 floats for the counts below 300: the
    vector kernel with every head length, and the scalar kernel where no head aligns both pointers;
  * 64 sentinel floats on each side of the destination stay as they were; a second launch gives the same bits."""
import numpy as np
import pytest
import torch

from lib import _hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
SENTINEL = np.float32(-1.2345678e25)
COUNTS = [1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 4097, 614400, 3 * 2 ** 20 + 5]
SMALL = [c for c in COUNTS if c < 300]


@pytest.fixture(scope='module')
def table():
    """(host int32 view, device float tensor) of the table; built once, never written."""
    rng = np.random.default_rng(11)
    bits = rng.integers(-2 ** 31, 2 ** 31, 256, dtype=np.int64).astype(np.int32)
    t = bits.view(np.float32).copy()
    t[7], t[100], t[200], t[255] = -0.0, np.inf, 1e-41, np.nan
    t[0] = -np.inf
    bits = t.view(np.int32).copy()
    assert len(np.unique(bits)) > 250                             # (a wrong index shows)
    dev = torch.from_numpy(bits.copy()).to(DEV).view(torch.float32)
    return bits, dev


def pixels(count, seed):
    """count bytes; every value occurs once there are 256 or more."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, count, dtype=np.uint8)
    if count >= 256:
        src[rng.permutation(count)[:256]] = np.arange(256, dtype=np.uint8)
        assert len(np.unique(src)) == 256
    return src


def run_case(table, count, s_off, d_off, seed=0):
    bits, lut = table
    lib = _hip.load()
    src = pixels(count, seed + count)
    sbuf = torch.zeros(count + 32, dtype=torch.uint8, device=DEV)
    assert sbuf.data_ptr() % 16 == 0
    sbuf[s_off:s_off + count].copy_(torch.from_numpy(src))
    dbuf = torch.full((count + 2 * GUARD + 4,), float(SENTINEL), device=DEV)
    assert dbuf.data_ptr() % 16 == 0
    lo = GUARD + d_off
    outs = []
    for _ in range(2):
        dbuf[lo:lo + count].fill_(float(SENTINEL))
        _hip.check(lib.mpnn_decode_u8(sbuf.data_ptr() + s_off, dbuf.data_ptr() + 4 * lo, lut.data_ptr(), count,
                                      torch.cuda.current_stream().cuda_stream), 'decode_u8')
        torch.cuda.synchronize()
        outs.append(dbuf.cpu().numpy().view(np.int32).copy())
    want = bits[src]
    sent = SENTINEL.view(np.int32)
    for got in outs:
        assert np.array_equal(got[lo:lo + count], want), (count, s_off, d_off)
        assert (got[:lo] == sent).all() and (got[lo + count:] == sent).all(), (count, s_off, d_off)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize('count', COUNTS)
def test_aligned(table, count):
    run_case(table, count, 0, 0)


@pytest.mark.parametrize('count', SMALL)
def test_every_offset(table, count):
    for s_off in range(16):
        for d_off in range(4):
            run_case(table, count, s_off, d_off, seed=16 * d_off + s_off)


@pytest.mark.parametrize('count,s_off,d_off', [(4097, 5, 1), (4097, 5, 2), (614400, 13, 1), (614400, 2, 3), (3 * 2 ** 20 + 5, 9, 1),
                                               (3 * 2 ** 20 + 5, 9, 0)])
def test_large_counts_off_alignment(table, count, s_off, d_off):
    """The long counts with a head (vector kernel) and with pointers that disagree modulo 4 (scalar kernel)."""
    run_case(table, count, s_off, d_off)
