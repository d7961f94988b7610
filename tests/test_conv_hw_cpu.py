"""CPU: the any-map entry points of the general conv kernels (csrc/conv_gen.hip: mpnn_msconv_*_hw) and the ground the GPU
tests of rectangular nets stand on.

* mpnn_msconv_hw_check / mpnn_msconv_hw_tiles: their limits, and that they extend the _gen forms (which keep theirs);
  the MPNN_E_ARG / MPNN_E_SHAPE returns of the four entry points on bad records (no GPU is touched).
* The device assembly of conv_gen.hip: every kernel runs on v_mfma_f32_16x16x4_f32 and uses no scratch.
* oracle/ref_net.py against the reference's own graph code on x0_shape (24, 40, 3) and (28, 28, 1) (a three-scale table):
  tests/golden/rect_ref_graph_golden.npz, written by tests/golden/rect_ref_graph.py; where the reference tree is
  present the vectors are also produced afresh and compared with the stored ones.
* MultiscaleConvMax.link on a 24x40 pyramid with supp = 5: clipped 3x5 filters on the coarsest map, n_ops.
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
import make_ref_graph_golden as M
import rect_ref_graph as R

GOLDEN = os.path.join(HERE, 'golden', 'rect_ref_graph_golden.npz')

# the channel / filter entries of tests/test_conv_gen.py::test_gen_check_limits' `bad` list (the map entries of that list
# are the _gen forms' own limits: the any-map forms take them, see below)
BAD_CHANNELS_FILTERS = [
    (32, 32, 3, 0, 16, 8, 7, 0, 0), (32, 32, 3, 0, 16, 7, 8, 0, 0), (4, 4, 16, 16, 16, 4, 4, 8, 5),
    (4, 4, 16, 16, 16, 4, 4, 5, 8), (32, 32, 3, 0, 16, 0, 3, 0, 0), (8, 8, 16, 16, 16, 3, 3, 0, 3),
    (32, 32, 2, 0, 16, 3, 3, 0, 0), (32, 32, 4, 0, 16, 3, 3, 0, 0), (32, 32, 24, 0, 16, 3, 3, 0, 0),
    (32, 32, 16, 8, 16, 3, 3, 3, 3), (32, 32, 16, 0, 24, 3, 3, 0, 0), (32, 32, 16, 0, 0, 3, 3, 0, 0),
    (32, 32, 528, 0, 16, 3, 3, 0, 0), (32, 32, 16, 0, 528, 3, 3, 0, 0)]


def test_hw_check_limits():
    lib = _hip.load()
    ck, gen = lib.mpnn_msconv_hw_check, lib.mpnn_msconv_gen_check
    for H, W in [(3, 3), (6, 6), (7, 7), (12, 12), (24, 40), (16, 64), (64, 16), (1, 2), (2, 1), (1, 1), (256, 1), (255, 256)]:
        assert ck(H, W, 16, 16, 32, 3, 3, 5, 5) == 0, (H, W)
        assert ck(H, W, 3, 0, 16, 7, 1, 0, 0) == 0, (H, W)
    assert ck(3, 5, 16, 16, 16, 3, 5, 5, 5) == 0                    # supp 5 clipped to the map: kh != kw
    assert ck(1, 2, 128, 128, 128, 1, 2, 3, 3) == 0
    for H, W in [(0, 8), (8, 0), (257, 8), (8, 257), (-4, 4), (0, 0)]:
        assert ck(H, W, 16, 0, 16, 3, 3, 0, 0) == _hip.E_SHAPE, (H, W)
    for args in BAD_CHANNELS_FILTERS:
        assert ck(*args) == _hip.E_SHAPE, args
    # every shape of the _gen forms is a shape of the _hw forms; the _gen forms keep their limits
    for H in [4] + list(range(8, 257, 8)):
        for rest in [(3, 0, 16, 7, 7, 0, 0), (128, 64, 128, 4, 4, 5, 5), (1, 16, 16, 1, 1, 7, 7), (16, 0, 512, 2, 2, 0, 0)]:
            assert gen(H, H, *rest) == 0 and ck(H, H, *rest) == 0
    for H, W in [(6, 6), (7, 7), (12, 12), (32, 16), (2, 2)]:
        assert gen(H, W, 16, 0, 16, 3, 3, 0, 0) == _hip.E_SHAPE and ck(H, W, 16, 0, 16, 3, 3, 0, 0) == 0


def test_hw_tiles():
    lib = _hip.load()
    hw, gen = lib.mpnn_msconv_hw_tiles, lib.mpnn_msconv_gen_tiles
    for H in [4] + list(range(8, 257, 8)):
        for n in (1, 2, 3, 4, 5, 37, 128):
            assert hw(n, H, H) == gen(n, H, H) > 0, (n, H)
    assert gen(3, 6, 6) == _hip.E_SHAPE and hw(3, 6, 6) == 3        # one 8x8 tile per image, hanging over both edges
    # tiles of 64 pixels: a side of 8 on an axis longer than 4, of 4 otherwise, as many images as fill the tile
    assert hw(5, 3, 3) == 2 and hw(5, 1, 2) == 2 and hw(4, 2, 4) == 1         # 4x4 tiles of four images
    assert hw(5, 3, 5) == 3 and hw(5, 6, 4) == 3                              # 4x8 / 8x4 tiles of two images
    assert hw(2, 12, 20) == 2 * 2 * 3 and hw(1, 24, 40) == 15 and hw(3, 16, 64) == 48 and hw(1, 7, 7) == 1
    assert hw(1, 2, 16) == 2 and hw(3, 2, 16) == 4                            # 4x8 tiles, two images each
    for n, H, W in [(0, 8, 8), (1, 0, 8), (1, 8, 257), (1, 257, 8)]:
        assert hw(n, H, W) == _hip.E_SHAPE


def test_hw_bad_records_return_codes():
    """Host-side validation only: every record here is refused before anything reaches a device."""
    lib = _hip.load()
    fake = 1 << 20                                  # (never dereferenced: the records are refused first)
    assert lib.mpnn_msconv_fwd_hw(None, 3, 3, 0, 0, None) == _hip.E_ARG
    a = _hip.ConvFwdArgs()
    a.n, a.H, a.W, a.Cout = 2, 6, 10, 16
    a.a = _hip.act(None, 16)
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_ARG           # no input map
    a.a.x, a.wa_pack, a.bias, a.out = fake, fake, fake, fake
    assert lib.mpnn_msconv_fwd_hw(a, 8, 3, 0, 0, None) == _hip.E_SHAPE         # filter beyond 7
    a.H = 0
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_SHAPE         # map size
    a.H, a.W = 6, 257
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_SHAPE
    a.H, a.W = 7, 10
    a.pool_out = fake
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_SHAPE         # odd H with pool_out
    a.H, a.W = 6, 5
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_SHAPE         # odd W with pool_out
    a.pool_out = None
    a.H, a.W = 6, 10
    a.idx = fake
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_ARG           # sample lists are not offered
    a.idx = None
    a.v, a.Cv = fake, 16
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 3, 3, None) == _hip.E_ARG           # v without w_vert
    a.a.mode = _hip.ACT_BN_BATCH
    a.v = None
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_ARG           # batch statistics without sums
    a.n = -1
    assert lib.mpnn_msconv_fwd_hw(a, 3, 3, 0, 0, None) == _hip.E_ARG

    h = _hip.DgradHorzArgs()
    h.n, h.H, h.W, h.Cout, h.Cg = 2, 3, 5, 16, 16
    assert lib.mpnn_msconv_dgrad_horz_hw(h, 3, 5, None) == _hip.E_ARG
    h.g, h.w_pack, h.out = fake, fake, fake
    ctx = _hip.BnCtx()
    h.g_ctx = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_horz_hw(h, 3, 5, None) == _hip.E_ARG         # g_ctx is not offered
    h.g_ctx = None
    h.prev = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_horz_hw(h, 3, 5, None) == _hip.E_ARG         # prev without s / red_out
    h.prev = None
    assert lib.mpnn_msconv_dgrad_horz_hw(h, 3, 9, None) == _hip.E_SHAPE
    h.W = 300
    assert lib.mpnn_msconv_dgrad_horz_hw(h, 3, 5, None) == _hip.E_SHAPE
    h.W, h.Cout = 5, 3
    assert lib.mpnn_msconv_dgrad_horz_hw(h, 3, 5, None) == _hip.E_SHAPE       # outputs: multiples of 16

    v = _hip.DgradVertArgs()
    v.n, v.H, v.W, v.Cout, v.Cg = 2, 3, 5, 16, 16
    assert lib.mpnn_msconv_dgrad_vert_hw(v, 5, 5, None) == _hip.E_ARG
    v.g, v.w_pack, v.dz_g_fine = fake, fake, fake
    v.fine = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_vert_hw(v, 5, 5, None) == _hip.E_ARG         # fine context without s
    assert lib.mpnn_msconv_dgrad_vert_hw(v, 5, 0, None) == _hip.E_SHAPE
    v.H = 0
    assert lib.mpnn_msconv_dgrad_vert_hw(v, 5, 5, None) == _hip.E_SHAPE

    w = _hip.WgradArgs()
    w.n, w.H, w.W, w.Cout, w.n_split = 2, 12, 20, 16, 1
    w.a = _hip.act(None, 16)
    assert lib.mpnn_msconv_wgrad_hw(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.a.x, w.g, w.dwa, w.db = fake, fake, fake, fake
    w.n_split = 0
    assert lib.mpnn_msconv_wgrad_hw(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.n_split = 2
    w.split_stride = 16
    assert lib.mpnn_msconv_wgrad_hw(w, 3, 3, 0, 0, None) == _hip.E_ARG         # splits would overlap
    w.split_stride = 0
    assert lib.mpnn_msconv_wgrad_hw(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.n_split = 1
    assert lib.mpnn_msconv_wgrad_hw(w, 0, 3, 0, 0, None) == _hip.E_SHAPE
    w.H = 257
    assert lib.mpnn_msconv_wgrad_hw(w, 3, 3, 0, 0, None) == _hip.E_SHAPE
    # the _gen forms still refuse the maps only the _hw forms take
    w.H, w.W = 12, 20
    assert lib.mpnn_msconv_wgrad_gen(w, 3, 3, 0, 0, None) == _hip.E_SHAPE


def test_hw_isa_mfma_and_no_scratch():
    """conv_gen.hip (the kernels behind both families) compiled as the library compiles it: every kernel contains
    v_mfma_f32_16x16x4_f32 and reports a zero private segment (no scratch)."""
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    csrc = os.path.join(ROOT, 'multipath-nn_amd', 'csrc')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'conv_gen.s')
        subprocess.check_call(['hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + os.path.join(ROOT, 'include'),
                               '-munsafe-fp-atomics', '-mllvm', '-amdgpu-kernarg-preload-count=16', '--cuda-device-only', '-S',
                               os.path.join(csrc, 'conv_gen.hip'), '-o', out], cwd=csrc, stderr=subprocess.DEVNULL)
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
    assert len(kernels) == 5, kernels                      # (one pair of kernels for both families: no second copy)
    for k in kernels:
        assert any(l.startswith('v_mfma_f32_16x16x4_f32') for l in bodies[k]), k
    priv = [l.split(':')[1].strip() for l in text.splitlines() if l.strip().startswith('.private_segment_fixed_size:')]
    names = [l.split(':')[1].strip() for l in text.splitlines() if l.strip().startswith('.name:') and '_Z' in l]
    assert len(priv) == len(names) == 5 and all(p == '0' for p in priv), list(zip(names, priv))
    assert 'scratch_' not in text and 'buffer_store_dword off' not in text


# ------------------------------------------------------------------ the oracle on the new shapes
def _ordered(net):
    out = []
    for ℓ in net.layers:
        for scope in (ℓ, ℓ.router):
            if scope is None:
                continue

            def walk(l):
                for k, v in vars(l.params).items():
                    out.append((k, v))
                for c in getattr(l, 'comps', []):
                    walk(c)
            walk(scope)
    return out


@pytest.mark.parametrize('key', sorted(R.CASES))
def test_oracle_matches_the_reference_graph_code_on_rectangular_images(key):
    """Forward values in both modes and every variable after one training step, at the bound of
    tests/test_ref_graph_golden.py (1e-9)."""
    import arch_and_hypers as A
    import lib.net_types as NT
    from oracle.ref_net import RefNet
    gold = np.load(GOLDEN)
    case = R.CASES[key]
    net = R.build(A, NT, case)
    H0, W0, _ = case['shape']
    S = len(case.get('arch', A.arch)[0])
    assert [tuple(s.shape[:2]) for s in net.root.comps[0].x] == [(H0 >> i, W0 >> i) for i in range(S)]
    params = _ordered(net)
    assert [n for n, _ in params] == list(gold['%s/names' % key])        # same parameters, same order
    rng = np.random.RandomState(case['seed'])
    vals = {id(p): M.param_value(n, p.shape, rng) for n, p in params}
    ref = RefNet(net)
    ref.load_params(vals)
    x0, y = R.case_inputs(case)
    kw = {} if case['tau'] is None else {'τ': case['tau']}
    layers = list(net.layers)
    leaves = [ℓ for ℓ in layers if not ℓ.sinks]
    switches = [ℓ for ℓ in layers if len(ℓ.sinks) > 1]

    def close(a, b, what):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, (what, a.shape, b.shape)
        assert np.abs(a - b).max() <= 1e-9 * (1 + np.abs(b).max()), (key, what, np.abs(a - b).max())
    n = len(x0)
    vec = lambda v: np.broadcast_to(v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v, np.float64), (n,))
    for mode in ('ev', 'tr'):
        res = ref.forward(x0, y, mode, **kw)
        Rs = lambda ℓ: res['out'][id(ℓ)]
        assert np.array_equal(np.stack([vec(Rs(ℓ)['p_ev']) for ℓ in layers]), gold['%s/%s/p_ev' % (key, mode)])
        close(np.stack([vec(Rs(ℓ)['c_err']) for ℓ in leaves]), gold['%s/%s/c_err' % (key, mode)], mode + ' c_err')
        assert np.array_equal(np.stack([vec(Rs(ℓ)['δ_cor']) for ℓ in leaves]), gold['%s/%s/d_cor' % (key, mode)])
        if '%s/%s/p_tr' % (key, mode) in gold:
            close(np.stack([vec(Rs(ℓ)['p_tr']) for ℓ in layers]), gold['%s/%s/p_tr' % (key, mode)], mode + ' p_tr')
            close(np.stack([Rs(ℓ.router)['x'].detach().numpy() for ℓ in switches]), gold['%s/%s/r' % (key, mode)], mode + ' router.x')
    ref.train_step(x0, y, M.LR, **kw)
    after = np.array([M.digest(ref.V(p).detach().numpy()) for _, p in params])
    g = gold['%s/after' % key]
    err = np.abs(after - g) / (1e-12 + np.abs(g).max(0, keepdims=True))
    assert err.max() <= 1e-9, (key, [params[i][0] for i in np.argwhere(err > 1e-9)[:, 0][:5]], err.max())


def test_stored_vectors_are_what_the_reference_graph_code_gives():
    """Where the reference tree is present: its graph code, run now, reproduces rect_ref_graph_golden.npz."""
    if not os.path.isdir(R.REF):
        pytest.skip('the reference tree is absent')
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'fresh.npz')
        env = dict(os.environ, OMP_NUM_THREADS='2', MKL_NUM_THREADS='2')
        subprocess.check_call([sys.executable, os.path.join(HERE, 'golden', 'rect_ref_graph.py'), '--emit', path], env=env,
                              stdout=subprocess.DEVNULL)
        with np.load(path) as fresh, np.load(GOLDEN) as gold:
            assert sorted(fresh.files) == sorted(gold.files)
            for k in gold.files:
                if gold[k].dtype.kind in 'US':
                    assert list(fresh[k]) == list(gold[k]), k
                else:
                    assert np.abs(fresh[k] - gold[k]).max() <= 1e-12 * (1 + np.abs(gold[k]).max()), k


# ------------------------------------------------------------------ operator surface
def test_multiscale_conv_links_on_a_24x40_pyramid_with_supp_5():
    from lib.layer_types import MultiscaleConvMax, ToPyramid
    from lib.net_types import Sym
    from oracle import np_ops as O
    pyr = ToPyramid(n_scales=4)
    pyr.link(Sym((24, 40, 3), None), None, None)
    assert [tuple(s.shape) for s in pyr.x] == [(24, 40, 3), (12, 20, 3), (6, 10, 3), (3, 5, 3)]
    conv = MultiscaleConvMax(n_chan=[16, 16, 32], supp=5, k_l2=0, σ_w=1)
    conv.link(pyr.x, None, None)
    assert [tuple(s.shape) for s in conv.x] == [(12, 20, 16), (6, 10, 16), (3, 5, 32)]      # the LAST three scales
    horz = [tuple(getattr(conv.params, 'w_horz_%d' % i).shape) for i in range(3)]
    vert = [tuple(getattr(conv.params, 'w_vert_%d' % i).shape) for i in range(2)]
    assert horz == [(5, 5, 3, 16), (5, 5, 3, 16), (3, 5, 3, 32)]                           # clipped to the 3x5 map
    assert vert == [(5, 5, 16, 16), (5, 5, 16, 32)]                                        # never clipped
    assert conv.n_ops == O.msconv_n_ops([(12, 20), (6, 10), (3, 5)], horz, vert)
    assert conv.n_ops == 12 * 20 * 1200 + 6 * 10 * (1200 + 6400) + 3 * 5 * (1440 + 12800)
