"""CPU: the any-channel entry points of the general conv kernels (csrc/conv_gen_ch.hip: mpnn_msconv_*_ch) and the ground the
GPU tests of odd-channel nets stand on.

* mpnn_msconv_ch_check: any channel count from 1 to 512 on the maps and filters of mpnn_msconv_hw_check, which it extends
  (the _gen / _hw forms keep their limits); the MPNN_E_ARG / MPNN_E_SHAPE returns of the four entry points on bad records
  (no GPU is touched).
* The device code of conv_gen_ch.hip: every kernel runs on v_mfma_f32_16x16x4_f32 and its metadata reports a zero private
  segment (no scratch).
* oracle/ref_net.py against the reference's own graph code on tables of odd widths over 2-, 4- and 5-channel images:
  tests/golden/chan_ref_graph_golden.npz, written by tests/golden/chan_ref_graph.py -- the checks of
  tests/test_conv_hw_cpu.py::test_oracle_matches_the_reference_graph_code_on_rectangular_images themselves, at 1e-9.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from lib import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import chan_ref_graph as CH
import test_conv_hw_cpu as HW

GOLDEN = os.path.join(HERE, 'golden', 'chan_ref_graph_golden.npz')

# the rows of BAD_CHANNELS_FILTERS whose only offence is a channel count from 1 to 512: Cin 2, 4, 24; Cv 8; Cout 24
ONLY_CHANNELS = [(32, 32, 2, 0, 16, 3, 3, 0, 0), (32, 32, 4, 0, 16, 3, 3, 0, 0), (32, 32, 24, 0, 16, 3, 3, 0, 0),
                 (32, 32, 16, 8, 16, 3, 3, 3, 3), (32, 32, 16, 0, 24, 3, 3, 0, 0)]


def test_ch_check_limits():
    lib = _hip.load()
    ck, hw, gen = lib.mpnn_msconv_ch_check, lib.mpnn_msconv_hw_check, lib.mpnn_msconv_gen_check
    assert all(row in HW.BAD_CHANNELS_FILTERS for row in ONLY_CHANNELS)
    for args in ONLY_CHANNELS:
        assert ck(*args) == 0 and hw(*args) == _hip.E_SHAPE and gen(*args) == _hip.E_SHAPE, args
    for c in (1, 5, 17, 511, 512):
        assert ck(8, 8, c, 0, 16, 3, 3, 0, 0) == 0 and ck(8, 8, 16, 0, c, 3, 3, 0, 0) == 0, c
        assert ck(3, 5, c, c, c, 3, 5, 5, 5) == 0, c
    for args in [(8, 8, 0, 0, 16, 3, 3, 0, 0), (8, 8, 16, 0, 0, 3, 3, 0, 0), (8, 8, 513, 0, 16, 3, 3, 0, 0),
                 (8, 8, 16, 0, 513, 3, 3, 0, 0), (8, 8, 16, 513, 16, 3, 3, 3, 3), (8, 8, 16, -1, 16, 3, 3, 3, 3),
                 (8, 8, -3, 0, 16, 3, 3, 0, 0)]:
        assert ck(*args) == _hip.E_SHAPE, args
    for args in HW.BAD_CHANNELS_FILTERS:                    # the bad filters, 0 and 528 channels
        if args not in ONLY_CHANNELS:
            assert ck(*args) == _hip.E_SHAPE, args
    for H, W in [(0, 8), (8, 0), (257, 8), (8, 257), (-4, 4), (0, 0)]:
        assert ck(H, W, 16, 0, 16, 3, 3, 0, 0) == _hip.E_SHAPE and ck(H, W, 5, 0, 7, 3, 3, 0, 0) == _hip.E_SHAPE, (H, W)
    # every shape of the _hw forms is a shape of the _ch forms
    for H, W in [(3, 3), (6, 6), (7, 7), (12, 12), (24, 40), (16, 64), (64, 16), (1, 2), (2, 1), (1, 1), (256, 1), (255, 256),
                 (4, 4), (8, 8), (32, 32), (256, 256)]:
        for rest in [(16, 16, 32, 3, 3, 5, 5), (3, 0, 16, 7, 1, 0, 0), (128, 64, 128, 4, 4, 5, 5), (1, 16, 16, 1, 1, 7, 7),
                     (16, 0, 512, 2, 2, 0, 0)]:
            assert hw(H, W, *rest) == 0 and ck(H, W, *rest) == 0, (H, W, rest)
    # the _gen / _hw forms still refuse what they refused
    for args in HW.BAD_CHANNELS_FILTERS:
        assert hw(*args) == _hip.E_SHAPE and gen(*args) == _hip.E_SHAPE, args


def test_ch_bad_records_return_codes():
    """Host-side validation only: every record here is refused before anything reaches a device."""
    lib = _hip.load()
    fake = 1 << 20                                  # (never dereferenced: the records are refused first)
    assert lib.mpnn_msconv_fwd_ch(None, 3, 3, 0, 0, None) == _hip.E_ARG
    a = _hip.ConvFwdArgs()
    a.n, a.H, a.W, a.Cout = 2, 6, 10, 7
    a.a = _hip.act(None, 5)
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_ARG           # no input map
    a.a.x, a.wa_pack, a.bias, a.out = fake, fake, fake, fake
    assert lib.mpnn_msconv_fwd_ch(a, 8, 3, 0, 0, None) == _hip.E_SHAPE         # filter beyond 7
    a.H = 0
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_SHAPE         # map size
    a.H, a.Cout = 6, 513
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_SHAPE         # channels beyond 512
    a.Cout = 0
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_SHAPE
    a.Cout = 7
    a.a.C = 513
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_SHAPE
    a.a.C = 5
    a.H, a.W = 7, 10
    a.pool_out = fake
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_SHAPE         # odd H with pool_out
    a.pool_out = None
    a.H, a.W = 6, 10
    a.idx = fake
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_ARG           # idx without cnt
    a.idx = None
    a.v, a.Cv = fake, 12
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 3, 3, None) == _hip.E_ARG           # v without w_vert
    a.a.mode = _hip.ACT_BN_BATCH
    a.v = None
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_ARG           # batch statistics without sums
    a.n = -1
    assert lib.mpnn_msconv_fwd_ch(a, 3, 3, 0, 0, None) == _hip.E_ARG

    h = _hip.DgradHorzArgs()
    h.n, h.H, h.W, h.Cout, h.Cg = 2, 3, 5, 10, 7
    assert lib.mpnn_msconv_dgrad_horz_ch(h, 3, 5, None) == _hip.E_ARG
    h.g, h.w_pack, h.out = fake, fake, fake
    ctx = _hip.BnCtx()
    h.g_ctx = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_horz_ch(h, 3, 5, None) == _hip.E_ARG         # g_ctx is not offered
    h.g_ctx = None
    h.prev = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_horz_ch(h, 3, 5, None) == _hip.E_ARG         # prev without s / red_out
    h.prev = None
    assert lib.mpnn_msconv_dgrad_horz_ch(h, 3, 9, None) == _hip.E_SHAPE
    h.W = 300
    assert lib.mpnn_msconv_dgrad_horz_ch(h, 3, 5, None) == _hip.E_SHAPE
    h.W, h.Cout = 5, 513
    assert lib.mpnn_msconv_dgrad_horz_ch(h, 3, 5, None) == _hip.E_SHAPE
    h.Cout = 3
    assert lib.mpnn_msconv_dgrad_horz_hw(h, 3, 5, None) == _hip.E_SHAPE       # (the _hw form: outputs in multiples of 16)

    v = _hip.DgradVertArgs()
    v.n, v.H, v.W, v.Cout, v.Cg = 2, 3, 5, 12, 20
    assert lib.mpnn_msconv_dgrad_vert_ch(v, 5, 5, None) == _hip.E_ARG
    v.g, v.w_pack, v.dz_g_fine = fake, fake, fake
    v.fine = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_vert_ch(v, 5, 5, None) == _hip.E_ARG         # fine context without s
    assert lib.mpnn_msconv_dgrad_vert_ch(v, 5, 0, None) == _hip.E_SHAPE
    v.Cg = 0
    assert lib.mpnn_msconv_dgrad_vert_ch(v, 5, 5, None) == _hip.E_SHAPE

    w = _hip.WgradArgs()
    w.n, w.H, w.W, w.Cout, w.n_split = 2, 12, 20, 10, 1
    w.a = _hip.act(None, 17)
    assert lib.mpnn_msconv_wgrad_ch(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.a.x, w.g, w.dwa, w.db = fake, fake, fake, fake
    w.n_split = 0
    assert lib.mpnn_msconv_wgrad_ch(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.n_split = 2
    w.split_stride = 16
    assert lib.mpnn_msconv_wgrad_ch(w, 3, 3, 0, 0, None) == _hip.E_ARG         # splits would overlap
    w.split_stride = 0
    assert lib.mpnn_msconv_wgrad_ch(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.n_split = 1
    assert lib.mpnn_msconv_wgrad_ch(w, 0, 3, 0, 0, None) == _hip.E_SHAPE
    w.Cout = 600
    assert lib.mpnn_msconv_wgrad_ch(w, 3, 3, 0, 0, None) == _hip.E_SHAPE
    # the _hw form still refuses the channels only the _ch form takes
    w.Cout = 10
    assert lib.mpnn_msconv_wgrad_hw(w, 3, 3, 0, 0, None) == _hip.E_SHAPE


def test_ch_isa_mfma_and_no_scratch():
    """conv_gen_ch.hip compiled as the library compiles it: the forward and input-gradient kernels with one and two output
    tiles per wave (dense and on a sample list) and the scalar-g weight-gradient kernel; each contains
    v_mfma_f32_16x16x4_f32, and the metadata of each reports a zero private segment (no scratch)."""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    csrc = os.path.join(ROOT, 'multipath-nn_amd', 'csrc')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'conv_gen_ch.s')
        subprocess.check_call(['hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + os.path.join(ROOT, 'include'),
                               '-munsafe-fp-atomics', '-mllvm', '-amdgpu-kernarg-preload-count=16', '--cuda-device-only', '-S',
                               os.path.join(csrc, 'conv_gen_ch.hip'), '-o', out], cwd=csrc, stderr=subprocess.DEVNULL)
        text = open(out).read()
    bodies, cur = {}, None
    for line in text.splitlines():
        head = line.split(';')[0].strip()
        if line.startswith('_Z') and head.endswith(':'):
            cur = head[:-1]
            bodies[cur] = []
        elif cur is not None:
            bodies[cur].append(line.strip())
    kernels = [k for k in bodies if 'gen_conv_k' in k or 'gen_wgrad_k' in k]
    assert len(kernels) == 11, kernels                     # (FWD, FWD on a list, DGH_BN, DGH_RAW, DGV) x NT 1, 2; wgrad
    for k in kernels:
        assert any(l.startswith('v_mfma_f32_16x16x4_f32') for l in bodies[k]), k
    priv = [l.split(':')[1].strip() for l in text.splitlines() if l.strip().startswith('.private_segment_fixed_size:')]
    names = [l.split(':')[1].strip() for l in text.splitlines() if l.strip().startswith('.name:') and '_Z' in l]
    assert sorted(names) == sorted(kernels)
    assert len(priv) == 11 and all(p == '0' for p in priv), list(zip(names, priv))


@pytest.mark.parametrize('key', sorted(CH.CASES))
def test_oracle_matches_the_reference_graph_code_on_odd_channel_counts(key, monkeypatch):
    """The checks of test_conv_hw_cpu's oracle test (forward values in both modes and every variable after one training
    step, at 1e-9) over this module's cases and fixture."""
    monkeypatch.setattr(HW, 'R', CH)
    monkeypatch.setattr(HW, 'GOLDEN', GOLDEN)
    HW.test_oracle_matches_the_reference_graph_code_on_rectangular_images(key)


def test_stored_vectors_are_what_the_reference_graph_code_gives():
    """Where the reference tree is present: its graph code, run now, reproduces chan_ref_graph_golden.npz."""
    if not os.path.isdir(CH.REF):
        pytest.skip('the reference tree is absent')
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'fresh.npz')
        env = dict(os.environ, OMP_NUM_THREADS='2', MKL_NUM_THREADS='2')
        subprocess.check_call([sys.executable, os.path.join(HERE, 'golden', 'chan_ref_graph.py'), '--emit', path], env=env,
                              stdout=subprocess.DEVNULL)
        with np.load(path) as fresh, np.load(GOLDEN) as gold:
            assert sorted(fresh.files) == sorted(gold.files)
            for k in gold.files:
                if gold[k].dtype.kind in 'US':
                    assert list(fresh[k]) == list(gold[k]), k
                else:
                    assert np.abs(fresh[k] - gold[k]).max() <= 1e-12 * (1 + np.abs(gold[k]).max()), k
