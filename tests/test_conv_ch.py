"""The any-channel forms of the general multiscale conv kernels (csrc/conv_gen_ch.hip: mpnn_msconv_*_ch, 1..512 channels
on every operand, output tiles fitted to the layer) and the BatchNorm elementwise launches for any C <= 512 (csrc/misc.hip)
through the C ABI, on the GPU.

Member by member against the float64 restatement (oracle/np_ops.py) with the runners of tests/test_conv_hw.py (every
output between sentinel guards, plain-store outputs pre-filled with NaN, BatchNorm inputs drawn away from ties) at the
tolerances of tests/test_conv_gen.py (_close: 2e-6 of the sum of the absolute values of an output's terms, 4e-6 where that
file uses 4e-6; _sum_close: 1e-5 for the fp64 sums).

The channel counts: tails of every kind -- 1, 3, 5, 7, 10 (no multiple of 4: scalar loads of the operand and of g), 12, 20,
24 (multiples of 4, no multiple of 16), 17 (a chunk tail of one channel), 72 (a second 64-channel group of 8 live
channels) -- on 8x8, 4x4 (four images per tile), 6x10 (overhanging tiles) and 3x5 maps; one, two and four output tiles
per wave (Cout <= 16, <= 32, above).

Bit equalities, which follow from the contraction order of an output element (chunk, tap row, tap, k-step: the same for
every tile count) and from fma(x, 0, acc) == acc: a _ch launch equals the _hw launch on every shape the latter takes, and a
10 -> 7 channel launch equals the _hw launch on operands zero-padded to 16 -> 16.

The affine maps and the evaluation head of the any-width exit kernels on the feature counts such nets bring (K = 40 on a
2x2x10 map, K = 7 on a 1x1x7 map) with the drivers and tolerances of tests/test_exit_gen_kernels.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

from lib import _hip
from test_conv_gen import _close, _sum_close
import test_conv_hw as HW

S = _hip.BN_SLOTS
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bn_quad_c32_bits.npz')

_seed, _id = HW._seed, HW._id


# ------------------------------------------------------------------ forward
# (n, H, W, Cin, act mode, shift, Cv, Cout, horz kh x kw, vert kvh x kvw, pool)
FWD = [
    (3, 8, 8, 5, 'id', 0, 0, 7, (3, 3), None, True),
    (5, 4, 4, 20, 'moving', 0, 12, 24, (4, 4), (5, 5), True),     # four images per tile, two output tiles per wave
    (2, 6, 10, 3, 'img', 1, 0, 10, (5, 5), None, True),           # overhanging tiles and a channel tail
    (2, 8, 8, 17, 'batch', 0, 0, 72, (1, 1), None, False),        # a chunk tail of 1; the second 64-channel group has 8 live channels
    (1, 3, 5, 1, 'img', 0, 0, 1, (3, 3), None, False),
]


@pytest.mark.parametrize('case', FWD, ids=list(map(_id, FWD)))
def test_fwd_ch_vs_oracle(case):
    lib = _hip.load()
    r = HW._run_fwd(lib, np.random.default_rng(_seed(case)), case, 'ch')
    n, H, W, Cout = case[0], case[1], case[2], case[7]
    out = r['out'].get().reshape(n, H, W, Cout)
    _close(out, r['ref'], r['bound'], what='out')
    ref = r['ref'].reshape(-1, Cout)
    sums = r['osum'].get().reshape(S, 2 * Cout)
    assert (sums[5:] == 0).all()                               # out_nslot = 5 slots used
    s = sums.sum(0)
    _sum_close(s[:Cout], ref.sum(0), np.abs(ref).sum(0) + r['bound'].reshape(-1, Cout).sum(0) * 2e-6, 'sum')
    _sum_close(s[Cout:], (ref ** 2).sum(0), (ref ** 2).sum(0), 'sum of squares')
    if case[10]:
        pooled = HW._oracle().pool2(out.astype(np.float64))    # the max-pool of the stored sums, exactly
        assert np.array_equal(r['pool'].get().reshape(pooled.shape), pooled)
    for b in (r['out'], r['osum']) + ((r['pool'],) if case[10] else ()):
        assert b.guards_ok()


# ------------------------------------------------------------------ input gradients
# dgrad-horz: (n, H, W, Cg, Cp, kh x kw, prev, extra, accumulate)
HORZ = [
    (3, 8, 8, 7, 10, (3, 3), True, True, False),
    (5, 4, 4, 24, 72, (4, 4), True, False, True),
    (2, 6, 10, 10, 7, (5, 5), False, True, True),
    (2, 8, 8, 72, 24, (1, 1), False, False, False),
    (5, 4, 4, 10, 24, (3, 3), True, True, True),
    (2, 6, 10, 7, 72, (3, 3), True, False, False),
]


@pytest.mark.parametrize('case', HORZ, ids=list(map(_id, HORZ)))
def test_dgrad_horz_ch_vs_oracle(case):
    import hiputil as U
    lib = _hip.load()
    Cp, prev = case[4], case[6]
    r = HW._run_horz(lib, np.random.default_rng(_seed(case)), case, 'ch')
    _close(r['out'].get().reshape(r['want'].shape), r['want'], r['bound'], what='out')
    assert r['out'].guards_ok()
    if prev:
        got = r['red'].get().reshape(S, 2 * Cp)
        assert (got[3:] == 0).all()
        dz, bm = r['dz'], r['bm']
        want_red = U.red_of(dz, bm.xh)
        terms = np.concatenate([np.abs(dz).reshape(-1, Cp).sum(0), np.abs(dz * bm.xh).reshape(-1, Cp).sum(0)])
        _sum_close(got.sum(0), want_red, terms + 1e-3, 'red_out')
        assert r['red'].guards_ok()


# dgrad-vert: (n, coarse H, coarse W, Cg, Cf, kvh x kvw, fine_has_dz); the fine (pooled) map is 2H x 2W
VERT = [
    (5, 4, 4, 24, 10, (5, 5), True),
    (2, 8, 8, 7, 72, (3, 3), False),
    (2, 6, 10, 72, 7, (4, 4), True),
    (3, 4, 4, 10, 24, (1, 1), True),
    (5, 4, 4, 10, 7, (3, 3), True, 'ties'),     # the finer map on a grid of 1/2: tied 2x2 maxima go to the FIRST one
]


@pytest.mark.parametrize('case', VERT, ids=list(map(_id, VERT)))
def test_dgrad_vert_ch_vs_oracle(case):
    lib = _hip.load()
    r = HW._run_vert(lib, np.random.default_rng(_seed(case)), case, 'ch')
    _close(r['buf'].get().reshape(r['want'].shape), r['want'], r['bound'], rel=4e-6, what='g_fine')
    assert r['buf'].guards_ok()


# ------------------------------------------------------------------ weight gradients
# (n, H, W, Cin, act mode, shift, Cv, Cout, horz, vert, n_split)
WGRAD = [
    (3, 8, 8, 17, 'batch', 0, 12, 7, (3, 3), (3, 3), 1),
    (3, 8, 8, 17, 'batch', 0, 12, 7, (3, 3), (3, 3), 3),          # (slabs of 4 x ceil(total / 4) floats, summed in order)
    (5, 4, 4, 17, 'moving', 0, 12, 10, (4, 4), (5, 5), 3),
    (2, 6, 10, 17, 'id', 0, 12, 24, (5, 5), (2, 2), 1),
    (2, 6, 10, 3, 'img', 1, 0, 10, (3, 3), None, 3),
    (2, 8, 8, 5, 'id', 0, 0, 72, (1, 1), None, 3),                # (two 64-channel groups; a scalar-loaded operand)
]


@pytest.mark.parametrize('case', WGRAD, ids=list(map(_id, WGRAD)))
def test_wgrad_ch_vs_oracle(case):
    lib = _hip.load()
    parts, want, bound, bufs = HW._run_wgrad(lib, np.random.default_rng(_seed(case)), case, 'ch')
    for got, w, b, name in zip(parts, want, bound, ['dw_horz', 'dw_vert', 'db'] if len(parts) == 3 else ['dw_horz', 'db']):
        _close(got.reshape(w.shape), w, b, rel=4e-6, what=name)
    assert all(b.guards_ok() for b in bufs[:2])


def test_wgrad_ch_twice_gives_equal_bits():
    """Two launches of the same record give the same bits (no fp32 atomics), with Cout % 4 != 0 and channel tails."""
    lib = _hip.load()
    case = (5, 6, 10, 17, 'batch', 0, 12, 10, (5, 5), (3, 3), 3)
    p1, _, _, _ = HW._run_wgrad(lib, np.random.default_rng(11), case, 'ch')
    p2, _, _, _ = HW._run_wgrad(lib, np.random.default_rng(11), case, 'ch')
    assert all(a.tobytes() == b.tobytes() for a, b in zip(p1, p2))


# ------------------------------------------------------------------ bit equalities
@pytest.mark.parametrize('H,Cin,Cv,Cout', [(8, 16, 0, 32), (4, 16, 16, 80)])
def test_ch_and_hw_give_equal_bits(H, Cin, Cv, Cout):
    """16 -> 32 at 8x8 (two output tiles per wave against four) and 16 + 16 -> 80 at 4x4: every output of every _ch entry
    point equals the _hw one."""
    lib = _hip.load()
    n, kv = 5, ((5, 5) if Cv else None)
    both = lambda run, case, seed: [run(lib, np.random.default_rng(seed), case, fam) for fam in ('ch', 'hw')]
    a, b = both(HW._run_fwd, (n, H, H, Cin, 'batch', 0, Cv, Cout, (3, 3), kv, True), 1)
    for k in ('out', 'osum', 'pool'):
        assert np.array_equal(a[k].get(), b[k].get()), 'fwd ' + k
    a, b = both(HW._run_horz, (n, H, H, Cout, Cin, (3, 3), True, True, False), 3)      # (output: Cin = 16, one tile per wave)
    for k in ('out', 'red'):
        assert np.array_equal(a[k].get(), b[k].get()), 'dgrad-horz ' + k
    a, b = both(HW._run_horz, (n, H, H, 16, 32, (2, 2), False, False, True), 4)
    assert np.array_equal(a['out'].get(), b['out'].get()), 'dgrad-horz (raw)'
    a, b = both(HW._run_vert, (n, H, H, Cout, 32, (5, 5), True), 5)
    assert np.array_equal(a['buf'].get(), b['buf'].get()), 'dgrad-vert'
    a, b = both(HW._run_wgrad, (n, H, H, Cin, 'batch', 0, Cv, Cout, (3, 3), kv, 3), 6)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), 'wgrad'


def test_ch_equals_hw_on_zero_padded_operands():
    """Cin 10 -> Cout 7 against the _hw launch on inputs and weights zero-padded to 16 -> 16 (identity activation), sliced to
    the live channels: bit for bit."""
    import torch
    import hiputil as U
    lib = _hip.load()
    rng = np.random.default_rng(5)
    n, H, W, Ci, Co = 3, 8, 8, 10, 7
    x = rng.standard_normal((n, H, W, Ci)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Ci, Co)) * 0.2).astype(np.float32)
    b = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    xp, wp, bp = np.zeros((n, H, W, 16), np.float32), np.zeros((3, 3, 16, 16), np.float32), np.zeros(16, np.float32)
    xp[..., :Ci], wp[:, :, :Ci, :Co], bp[:Co] = x, w, b
    outs = {}
    for fam, (x_, w_, b_) in (('ch', (x, w, b)), ('hw', (xp, wp, bp))):
        ci, co = x_.shape[3], w_.shape[3]
        xd, wd, bd = U.dev(x_), U.dev(w_), U.dev(b_)
        out = U.Guarded(n * H * W * co); out.fill(float('nan'))
        pool = U.Guarded(n * (H // 2) * (W // 2) * co); pool.fill(float('nan'))
        osum = U.Guarded(S * 2 * co, dtype=torch.float64); osum.fill(0.0)
        rec = _hip.ConvFwdArgs()
        rec.a = _hip.act(xd, ci, _hip.ACT_IDENTITY, 0)
        rec.wa_pack, rec.bias, rec.out, rec.pool_out = wd.data_ptr(), bd.data_ptr(), out.ptr(), pool.ptr()
        rec.out_sum, rec.out_nslot = osum.ptr(), 3
        rec.n, rec.H, rec.W, rec.Cout = n, H, W, co
        _hip.check(getattr(lib, 'mpnn_msconv_fwd_' + fam)(C.byref(rec), 3, 3, 0, 0, U.stream()), 'fwd_' + fam)
        torch.cuda.synchronize()
        assert out.guards_ok() and pool.guards_ok() and osum.guards_ok()
        sums = osum.get().reshape(S, 2, co)
        outs[fam] = (out.get().reshape(n, H, W, co)[..., :Co], pool.get().reshape(n, H // 2, W // 2, co)[..., :Co], sums[:, :, :Co])
    assert np.isfinite(outs['ch'][0]).all()
    for a, b_, what in zip(outs['ch'], outs['hw'], ('out', 'pool', 'sums')):
        assert np.array_equal(a, b_), what


# ------------------------------------------------------------------ sample lists
@pytest.mark.parametrize('count', [0, 1, 5])
@pytest.mark.parametrize('shape', ['4x4', '8x8'])
def test_fwd_ch_on_a_sample_list(shape, count):
    """Capacity 8: the listed images get the bits of the dense _ch launch, every other row keeps its NaN fill; an index
    beyond the buffers is no image."""
    import torch
    import hiputil as U
    lib = _hip.load()
    N = 8
    # (n, H, W, Cin, act mode, shift, Cv, Cout, horz, vert, pool)
    case = (N, 4, 4, 20, 'moving', 0, 12, 24, (4, 4), (5, 5), True) if shape == '4x4' else \
        (N, 8, 8, 5, 'id', 0, 0, 7, (3, 3), None, True)
    n, H, W, Cout = case[0], case[1], case[2], case[7]
    dense = HW._run_fwd(lib, np.random.default_rng(_seed(case)), case, 'ch')
    want = dense['out'].get().reshape(n, -1).copy()
    want_pool = dense['pool'].get().reshape(n, -1).copy()
    assert np.isfinite(want).all()
    rec = dense['rec']
    listed = [6, 2, 9, 0, 5][:count]                           # (9: beyond the buffers)
    idx = U.dev(np.array(listed + [3] * (N - count), np.int32), torch.int32)      # (behind the count: never read as a sample)
    cnt = U.dev(np.array([count], np.int32), torch.int32)
    out = U.Guarded(n * H * W * Cout); out.fill(float('nan'))
    pool = U.Guarded(n * (H // 2) * (W // 2) * Cout); pool.fill(float('nan'))
    rec.out, rec.pool_out, rec.out_sum = out.ptr(), pool.ptr(), None
    rec.idx, rec.cnt = idx.data_ptr(), cnt.data_ptr()
    _hip.check(lib.mpnn_msconv_fwd_ch(C.byref(rec), *case[8], *(case[9] or (0, 0)), U.stream()), 'fwd_ch list')
    torch.cuda.synchronize()
    assert out.guards_ok() and pool.guards_ok()
    got, got_pool = out.get().reshape(n, -1), pool.get().reshape(n, -1)
    live = [i for i in listed if i < N]
    for i in range(N):
        if i in live:
            assert np.array_equal(got[i], want[i]) and np.array_equal(got_pool[i], want_pool[i]), i
        else:
            assert np.isnan(got[i]).all() and np.isnan(got_pool[i]).all(), i


# ------------------------------------------------------------------ BatchNorm elementwise launches
def _bn_case(C_, seed=0, shape=(3, 5, 7)):
    import hiputil as U
    rng = np.random.default_rng(1000 * C_ + seed)
    bm = U.BnMap(rng, shape + (C_,), 8)
    dy, dy64 = U.f32(rng.standard_normal(shape + (C_,)))
    red64 = rng.standard_normal(2 * C_) * 10
    return bm, dy, dy64, red64


@pytest.mark.parametrize('C_', [7, 10, 48, 300])
def test_bn_launches_any_c_vs_float64(C_):
    import torch
    import hiputil as U
    lib = _hip.load()
    bm, dy, dy64, red64 = _bn_case(C_)
    # mpnn_bn_bwd_reduce: dz = dy where relu(bn(s)) > 0, red = [sum dz, sum dz * xhat]
    dz, red = U.bn_bwd_reduce(dy, bm.s, bm.dev, bm.cnt)
    want = dy64 * (bm.y > 0)
    assert np.array_equal(dz.astype(np.float64), want)
    terms = np.concatenate([np.abs(want).reshape(-1, C_).sum(0), np.abs(want * bm.xh).reshape(-1, C_).sum(0)])
    _sum_close(red, U.red_of(want, bm.xh), terms + 1e-3, 'red')
    # mpnn_bn_bwd_apply
    g = U.bn_bwd_apply(dy, bm.s, bm.dev, bm.cnt, red64)
    bound = np.abs(bm.gamma64 * bm.rstd) * (np.abs(dy64) + np.abs(red64[:C_]) / bm.cnt + np.abs(bm.xh * red64[C_:]) / bm.cnt)
    _close(g, bm.apply(dy64, red64), bound, what='bn_bwd_apply')
    # mpnn_bn_relu_fwd, between guards
    y = U.Guarded(bm.s.size); y.fill(float('nan'))
    a = _hip.act(bm.sd, C_, _hip.ACT_BN_BATCH, 0, bm.dev, bm.cnt)
    _hip.check(lib.mpnn_bn_relu_fwd(C.byref(a), y.ptr(), bm.cnt, U.stream()), 'bn_relu_fwd')
    torch.cuda.synchronize()
    assert y.guards_ok()
    ybound = np.abs(bm.gamma64 * bm.rstd) * (np.abs(bm.s64) + np.abs(bm.m)) + np.abs(bm.beta64)
    _close(y.get().reshape(bm.y.shape), np.maximum(bm.y, 0.0), ybound, what='bn_relu_fwd')
    assert np.array_equal(y.get().reshape(bm.y.shape) > 0, bm.y > 0)


def _bn_c32_bits():
    """The three launches at C = 32 (the quad kernels) on a seeded input of 2 x 8 x 8 pixels: one workgroup, so the fp64
    atomics of the reduction add to zeros in a fixed order."""
    import torch
    import hiputil as U
    lib = _hip.load()
    bm, dy, dy64, red64 = _bn_case(32, shape=(2, 8, 8))
    dz, red = U.bn_bwd_reduce(dy, bm.s, bm.dev, bm.cnt)
    g = U.bn_bwd_apply(dy, bm.s, bm.dev, bm.cnt, red64)
    y = torch.full((bm.s.size,), float('nan'), device=U.DEV)
    a = _hip.act(bm.sd, 32, _hip.ACT_BN_BATCH, 0, bm.dev, bm.cnt)
    _hip.check(lib.mpnn_bn_relu_fwd(C.byref(a), y.data_ptr(), bm.cnt, U.stream()), 'bn_relu_fwd')
    torch.cuda.synchronize()
    return dict(dz=dz.reshape(-1), red=red, g=g.reshape(-1), y=y.cpu().numpy())


def test_bn_launches_at_c32_keep_their_bits():
    """On the shapes the quad kernels take, they still run: the bits of tests/golden/bn_quad_c32_bits.npz, which
    _bn_c32_bits() wrote with the library as it was before the any-C kernels existed."""
    got = _bn_c32_bits()
    with np.load(GOLDEN) as gold:
        for k in ('dz', 'red', 'g', 'y'):
            assert np.array_equal(got[k], gold[k]), k


# ------------------------------------------------------------------ exits on such maps
@pytest.mark.parametrize('case', [(9, 4, 10, 'batch', 10, 16, 'r'), (6, 1, 7, 'moving', 10, 16, ''), (19, 4, 10, 'moving', 10, 0, '')],
                         ids=['2x2x10', '1x1x7', '2x2x10-head'])
def test_lin_gen_on_odd_feature_counts(case):
    """mpnn_lin_fwd_gen / mpnn_lin_bwd_gen with K = 40 (a 2x2x10 map) and K = 7 (a 1x1x7 map)."""
    from test_exit_gen_kernels import Lin, check_lin
    check_lin([Lin(case)])


@pytest.mark.parametrize('HW_,C_', [(4, 10), (1, 7)], ids=['2x2x10', '1x1x7'])
def test_exit_ev_gen_on_odd_feature_counts(HW_, C_):
    """The evaluation head and router (mpnn_exit_ev_gen) on the same two maps."""
    from test_exit_gen_kernels import check_ev
    from test_predict_kernels import Exit, check_label_free
    ex = Exit(31 + C_, N=70, count=41, C_=C_, nc=10, R=16, R2=16, S=2, HW=HW_, eps=(1e-6, 1e-3))
    out = ex.launch(True, labels=True, lists=(1,))
    check_ev(ex, (1,), out, '%dx%d' % (HW_, C_))
    check_label_free(ex, gen=True)
