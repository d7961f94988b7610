"""CPU: the decode tables of 8-bit images, the host-side refusals of mpnn_decode_u8 (no device is touched: the entry point
returns before it launches) and the argument errors of Net.predict / Net.predict_all that are raised before an engine is
needed."""
import os

import numpy as np
import pytest

from lib import _hip
from lib.decode import decode_table

FAKE = 0x1000                       # a non-NULL, 16-byte aligned pointer value; the checks never dereference it


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip.load()


def test_named_tables_are_the_prep_data_expressions():
    gamma, unit = decode_table('gamma'), decode_table('unit')
    for t in (gamma, unit):
        assert t.dtype == np.float32 and t.shape == (256,)
    want_gamma = np.float32(np.arange(256, dtype=np.uint8) ** 2.2 / 255 ** 2.2)
    want_unit = np.float32(np.arange(256) / 255)
    assert np.array_equal(gamma.view(np.int32), want_gamma.view(np.int32))
    assert np.array_equal(unit.view(np.int32), want_unit.view(np.int32))
    # the same as decoding an image the way prep-data does: the table is indexed by the pixel value
    img = np.random.default_rng(0).integers(0, 256, (5, 4, 4, 3), dtype=np.uint8)
    assert np.array_equal(gamma[img], np.float32(img ** 2.2 / 255 ** 2.2))
    assert np.array_equal(unit[img], np.float32(img / 255))


def test_gamma_table_is_monotone_from_0_to_1():
    gamma = decode_table('gamma')
    assert gamma[0] == 0 and gamma[255] == 1
    assert (np.diff(gamma.astype(np.float64)) > 0).all()


def test_an_array_is_used_as_it_is():
    rng = np.random.default_rng(1)
    t = rng.standard_normal(256).astype(np.float32)
    t[3], t[4], t[5] = np.inf, -0.0, np.nan
    got = decode_table(t)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), t.view(np.int32))
    assert np.array_equal(decode_table(list(range(256))), np.arange(256, dtype=np.float32))
    assert np.array_equal(decode_table(np.arange(256, dtype=np.float64) / 4), np.arange(256, dtype=np.float32) / 4)


@pytest.mark.parametrize('spec', ['srgb', '', None, 2.2, 3, True, np.zeros(255), np.zeros(257), np.zeros((2, 128)), np.zeros((256, 1)),
                                  ['a'] * 256, object()])
def test_bad_specs_raise(spec):
    with pytest.raises(ValueError):
        decode_table(spec)


def test_decode_u8_refuses_bad_arguments_on_the_host():
    lib = _lib()
    assert lib.mpnn_decode_u8(None, FAKE, FAKE, 16, None) == _hip.E_ARG
    assert lib.mpnn_decode_u8(FAKE, None, FAKE, 16, None) == _hip.E_ARG
    assert lib.mpnn_decode_u8(FAKE, FAKE, None, 16, None) == _hip.E_ARG
    assert lib.mpnn_decode_u8(None, None, None, 0, None) == _hip.E_ARG
    assert lib.mpnn_decode_u8(FAKE, FAKE, FAKE, -1, None) == _hip.E_ARG
    assert lib.mpnn_decode_u8(FAKE, FAKE, FAKE, -2 ** 40, None) == _hip.E_ARG
    assert lib.mpnn_decode_u8(FAKE, FAKE + 2, FAKE, 16, None) == _hip.E_ARG         # dst is no float pointer
    assert lib.mpnn_decode_u8(FAKE, FAKE, FAKE, 0, None) == 0                        # nothing to do: no launch
    assert lib.mpnn_decode_u8(FAKE + 5, FAKE + 12, FAKE, 0, None) == 0


def _net():
    import arch_and_hypers as A
    return A.ac_chain(k_cpt=1e-9)((32, 32, 3), (10,))


def test_predict_argument_errors_need_no_engine():
    net = _net()
    xf = np.zeros((4, 32, 32, 3), np.float32)
    xu = np.zeros((4, 32, 32, 3), np.uint8)
    for x in (xf, xf.astype(np.float64), xu.astype(np.int32)):
        with pytest.raises(ValueError, match='uint8'):
            net.predict(x, decode='gamma')
        with pytest.raises(ValueError, match='uint8'):
            net.predict_all(x, decode='unit')
    import torch
    with pytest.raises(ValueError, match='uint8'):
        net.predict(torch.zeros((4, 32, 32, 3)), decode='gamma')
    with pytest.raises(ValueError, match='decode'):
        net.predict(xu, decode='srgb')
    with pytest.raises(ValueError, match='decode'):
        net.predict_all(xu, decode=np.zeros(100))
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='batch'):
            net.predict_all(xf, batch=bad)
    with pytest.raises(ValueError, match='array of images'):
        net.predict_all(3.0)
    assert net._engine is None                                    # none of these built an engine
