"""The general multiscale conv kernels (csrc/conv_gen.hip: filters of any size from 1x1 to 7x7) through the C ABI.

CPU: mpnn_msconv_gen_check's limits, the MPNN_E_ARG / MPNN_E_SHAPE returns of the four entry points on bad records (no
GPU is touched), and the device assembly of conv_gen.hip (every kernel runs on v_mfma_f32_16x16x4_f32 and uses no
scratch).

GPU: member by member against a float64 restatement (oracle/np_ops.py: TensorFlow SAME padding, even sizes included),
with every output between sentinel guards (tests/hiputil.py: Guarded) and plain-store outputs pre-filled with NaN.  Errors
are held to 2e-6 of the sum of the absolute values of the terms of each output (fp32 MFMA chains over up to 49 x 128
products); the fp64 BatchNorm sums / reductions to 1e-5 of theirs.  The pre-BN maps of ReLU masks and max-pools are drawn
so that no decision is within 1e-3 of a tie (hiputil.BnMap).  At 3x3 the general forms match the tuned entry points on
the same inputs to fp32 rounding.
"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from lib import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = _hip.BN_SLOTS


# ------------------------------------------------------------------ CPU
def test_gen_check_limits():
    lib = _hip.load()
    ck = lib.mpnn_msconv_gen_check
    assert ck(32, 32, 3, 0, 16, 7, 7, 0, 0) == 0
    assert ck(4, 4, 128, 64, 128, 4, 4, 5, 5) == 0
    assert ck(8, 8, 1, 16, 16, 1, 1, 7, 7) == 0
    assert ck(256, 256, 16, 0, 512, 2, 2, 0, 0) == 0
    bad = [(32, 32, 3, 0, 16, 8, 7, 0, 0), (32, 32, 3, 0, 16, 7, 8, 0, 0), (4, 4, 16, 16, 16, 4, 4, 8, 5),
           (4, 4, 16, 16, 16, 4, 4, 5, 8), (32, 32, 3, 0, 16, 0, 3, 0, 0), (8, 8, 16, 16, 16, 3, 3, 0, 3),
           (7, 7, 16, 0, 16, 3, 3, 0, 0), (6, 6, 16, 0, 16, 3, 3, 0, 0), (2, 2, 16, 0, 16, 1, 1, 0, 0),
           (12, 12, 16, 0, 16, 3, 3, 0, 0), (32, 16, 16, 0, 16, 3, 3, 0, 0),
           (32, 32, 2, 0, 16, 3, 3, 0, 0), (32, 32, 4, 0, 16, 3, 3, 0, 0), (32, 32, 24, 0, 16, 3, 3, 0, 0),
           (32, 32, 16, 8, 16, 3, 3, 3, 3), (32, 32, 16, 0, 24, 3, 3, 0, 0), (32, 32, 16, 0, 0, 3, 3, 0, 0),
           (32, 32, 528, 0, 16, 3, 3, 0, 0), (32, 32, 16, 0, 528, 3, 3, 0, 0)]
    for args in bad:
        assert ck(*args) == _hip.E_SHAPE, args
    assert lib.mpnn_msconv_gen_tiles(5, 4, 4) == 2 and lib.mpnn_msconv_gen_tiles(3, 32, 32) == 48
    assert lib.mpnn_msconv_gen_tiles(3, 6, 6) == _hip.E_SHAPE


def test_gen_bad_records_return_codes():
    """Host-side validation only: every record here is refused before anything reaches a device."""
    lib = _hip.load()
    fake = 1 << 20                                  # (never dereferenced: the records are refused first)
    assert lib.mpnn_msconv_fwd_gen(None, 3, 3, 0, 0, None) == _hip.E_ARG
    a = _hip.ConvFwdArgs()
    a.n, a.H, a.W, a.Cout = 2, 8, 8, 16
    a.a = _hip.act(None, 16)
    assert lib.mpnn_msconv_fwd_gen(a, 3, 3, 0, 0, None) == _hip.E_ARG          # no input map
    a.a.x, a.wa_pack, a.bias, a.out = fake, fake, fake, fake
    assert lib.mpnn_msconv_fwd_gen(a, 8, 3, 0, 0, None) == _hip.E_SHAPE        # filter beyond 7
    a.H = a.W = 6
    assert lib.mpnn_msconv_fwd_gen(a, 3, 3, 0, 0, None) == _hip.E_SHAPE        # map size
    a.H = a.W = 8
    a.idx = fake
    assert lib.mpnn_msconv_fwd_gen(a, 3, 3, 0, 0, None) == _hip.E_ARG          # sample lists are not offered
    a.idx = None
    a.v, a.Cv = fake, 16
    assert lib.mpnn_msconv_fwd_gen(a, 3, 3, 3, 3, None) == _hip.E_ARG          # v without w_vert
    a.a.mode = _hip.ACT_BN_BATCH
    a.v = None
    assert lib.mpnn_msconv_fwd_gen(a, 3, 3, 0, 0, None) == _hip.E_ARG          # batch statistics without sums
    a.n = -1
    assert lib.mpnn_msconv_fwd_gen(a, 3, 3, 0, 0, None) == _hip.E_ARG

    h = _hip.DgradHorzArgs()
    h.n, h.H, h.W, h.Cout, h.Cg = 2, 8, 8, 16, 16
    assert lib.mpnn_msconv_dgrad_horz_gen(h, 3, 3, None) == _hip.E_ARG
    h.g, h.w_pack, h.out = fake, fake, fake
    ctx = _hip.BnCtx()
    h.g_ctx = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_horz_gen(h, 3, 3, None) == _hip.E_ARG        # g_ctx is not offered
    h.g_ctx = None
    h.prev = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_horz_gen(h, 3, 3, None) == _hip.E_ARG        # prev without s / red_out
    h.prev = None
    assert lib.mpnn_msconv_dgrad_horz_gen(h, 3, 9, None) == _hip.E_SHAPE
    h.Cout = 3
    assert lib.mpnn_msconv_dgrad_horz_gen(h, 3, 3, None) == _hip.E_SHAPE      # outputs: multiples of 16

    v = _hip.DgradVertArgs()
    v.n, v.H, v.W, v.Cout, v.Cg = 2, 4, 4, 16, 16
    assert lib.mpnn_msconv_dgrad_vert_gen(v, 5, 5, None) == _hip.E_ARG
    v.g, v.w_pack, v.dz_g_fine = fake, fake, fake
    v.fine = C.pointer(ctx)
    assert lib.mpnn_msconv_dgrad_vert_gen(v, 5, 5, None) == _hip.E_ARG        # fine context without s
    assert lib.mpnn_msconv_dgrad_vert_gen(v, 5, 0, None) == _hip.E_SHAPE

    w = _hip.WgradArgs()
    w.n, w.H, w.W, w.Cout, w.n_split = 2, 8, 8, 16, 1
    w.a = _hip.act(None, 16)
    assert lib.mpnn_msconv_wgrad_gen(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.a.x, w.g, w.dwa, w.db = fake, fake, fake, fake
    w.n_split = 0
    assert lib.mpnn_msconv_wgrad_gen(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.n_split = 2
    w.split_stride = 16
    assert lib.mpnn_msconv_wgrad_gen(w, 3, 3, 0, 0, None) == _hip.E_ARG        # splits would overlap
    w.split_stride = 0
    assert lib.mpnn_msconv_wgrad_gen(w, 3, 3, 0, 0, None) == _hip.E_ARG
    w.n_split = 1
    assert lib.mpnn_msconv_wgrad_gen(w, 0, 3, 0, 0, None) == _hip.E_SHAPE


def test_gen_isa_mfma_and_no_scratch():
    """conv_gen.hip compiled as the library compiles it: every kernel contains v_mfma_f32_16x16x4_f32 and reports a zero
    private segment (no scratch)."""
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
    assert len(kernels) == 5, kernels
    for k in kernels:
        assert any(l.startswith('v_mfma_f32_16x16x4_f32') for l in bodies[k]), k
    priv = [l.split(':')[1].strip() for l in text.splitlines() if l.strip().startswith('.private_segment_fixed_size:')]
    names = [l.split(':')[1].strip() for l in text.splitlines() if l.strip().startswith('.name:') and '_Z' in l]
    assert len(priv) == len(names) == 5 and all(p == '0' for p in priv), list(zip(names, priv))
    assert 'scratch_' not in text and 'buffer_store_dword off' not in text


# ------------------------------------------------------------------ GPU helpers
def _oracle():
    from oracle import np_ops as O
    return O


def _conv_abs(x, w):
    O = _oracle()
    return O.conv_same(np.abs(x), np.abs(w))


def _dconv(g, w, cin):
    """Input gradient of conv_same with filter w (HWIO [kh][kw][cin][cout]) for output gradient g, and its absolute bound."""
    O = _oracle()
    n, H, W, _ = g.shape
    z = np.zeros((n, H, W, cin))
    dx = O.conv_same_bwd(z, w, g)[0]
    bound = O.conv_same_bwd(z, np.abs(w), np.abs(g))[0]
    return dx, bound


def _act(rng, n, H, C_, mode, shift, nslot=8):
    """An input operand: (device act, fp64 activation as the kernel sees it at H x H, keep-alive)."""
    import hiputil as U
    if C_ in (1, 3):
        x, x64 = U.f32(rng.random((n, H << shift, H << shift, C_)))
        xd = U.dev(x)
        return _hip.act(xd, C_, _hip.ACT_IDENTITY, shift), x64[:, ::1 << shift, ::1 << shift], [xd]
    if mode == 'id':
        x, x64 = U.f32(rng.standard_normal((n, H, H, C_)))
        xd = U.dev(x)
        return _hip.act(xd, C_, _hip.ACT_IDENTITY, 0), x64, [xd]
    if mode == 'batch':
        bm = U.BnMap(rng, (n, H, H, C_), nslot)
        return _hip.act(bm.sd, C_, _hip.ACT_BN_BATCH, 0, bm.dev, bm.cnt), np.maximum(bm.y, 0.0), [bm]
    # moving averages
    s, s64 = U.f32(rng.standard_normal((n, H, H, C_)))
    g_, g64 = U.f32(rng.uniform(0.5, 1.5, C_))
    b_, b64 = U.f32(rng.standard_normal(C_) * 0.3)
    m_, m64 = U.f32(rng.standard_normal(C_) * 0.2)
    v_, v64 = U.f32(rng.uniform(0.5, 2.0, C_))
    bn = dict(sum=None, gamma=U.dev(g_), beta=U.dev(b_), m_avg=U.dev(m_), v_avg=U.dev(v_), eps=1e-6, nslot=1)
    y = np.maximum(g64 * (s64 - m64) / np.sqrt(v64 + np.float32(1e-6).astype(np.float64)) + b64, 0.0)
    sd = U.dev(s)
    return _hip.act(sd, C_, _hip.ACT_BN_MOVING, 0, bn, 1), y, [sd, bn]


def _close(got, ref, bound, rel=2e-6, what=''):
    err = np.abs(np.asarray(got, np.float64) - ref)
    lim = rel * bound + 1e-6
    assert np.all(np.isfinite(got)), what + ': not every element written'
    assert (err <= lim).all(), '%s: worst %.3g (limit %.3g)' % (what, float((err - lim).max()), float(lim.max()))


def _sum_close(got, ref, bound, what):
    err = np.abs(got - ref)
    assert (err <= 1e-5 * bound + 1e-9).all(), '%s: worst %.3g' % (what, float(err.max()))


# ------------------------------------------------------------------ forward
# (n, H, Cin, act mode, shift, Cv, Cout, horz kh x kw, vert kvh x kvw, pool)
FWD = [
    (3, 32, 3, 'img', 1, 0, 16, (5, 5), None, True),
    (2, 32, 1, 'img', 0, 0, 32, (7, 7), None, True),
    (3, 16, 16, 'batch', 0, 16, 32, (2, 2), (2, 2), True),
    (2, 8, 64, 'moving', 0, 32, 64, (7, 7), (7, 7), True),
    (5, 4, 128, 'batch', 0, 64, 128, (4, 4), (5, 5), True),
    (6, 8, 3, 'img', 2, 16, 16, (1, 1), (1, 1), False),
    (2, 16, 32, 'id', 0, 0, 48, (4, 2), None, True),
    (5, 4, 16, 'moving', 0, 16, 80, (3, 3), (6, 6), False),
    (2, 32, 16, 'batch', 0, 16, 16, (5, 5), (5, 5), True),
]


def _run_fwd(lib, rng, case, tuned=False):
    import torch
    import hiputil as U
    n, H, Cin, mode, shift, Cv, Cout, kh, kv, pool = case
    a, act64, keep = _act(rng, n, H, Cin, mode, shift)
    wh, wh64 = U.f32(rng.standard_normal(kh + (Cin, Cout)) * 0.2)
    b, b64 = U.f32(rng.standard_normal(Cout) * 0.1)
    rec = _hip.ConvFwdArgs()
    rec.a = a
    whd, bd = U.dev(wh), U.dev(b)
    rec.wa_pack, rec.bias = whd.data_ptr(), bd.data_ptr()
    ref = _oracle().conv_same(act64, wh64) + b64
    bound = _conv_abs(act64, wh64) + np.abs(b64)
    keep += [whd, bd]
    if Cv:
        v, v64 = U.f32(rng.standard_normal((n, H, H, Cv)))
        wv, wv64 = U.f32(rng.standard_normal(kv + (Cv, Cout)) * 0.2)
        vd, wvd = U.dev(v), U.dev(wv)
        keep += [vd, wvd]
        rec.v, rec.Cv, rec.wv_pack = vd.data_ptr(), Cv, wvd.data_ptr()
        ref = ref + _oracle().conv_same(v64, wv64)
        bound = bound + _conv_abs(v64, wv64)
    out = U.Guarded(n * H * H * Cout); out.fill(float('nan'))
    osum = U.Guarded(S * 2 * Cout, dtype=torch.float64); osum.fill(0.0)
    pl = U.Guarded(n * (H // 2) * (H // 2) * Cout) if pool else None
    if pl is not None:
        pl.fill(float('nan'))
    rec.out, rec.out_sum, rec.out_nslot = out.ptr(), osum.ptr(), 5
    rec.pool_out = pl.ptr() if pl is not None else None
    rec.n, rec.H, rec.W, rec.Cout = n, H, H, Cout
    kvv = kv or (0, 0)
    _hip.check(lib.mpnn_msconv_fwd_gen(C.byref(rec), *kh, *kvv, U.stream()), 'msconv_fwd_gen')
    torch.cuda.synchronize()
    return dict(out=out, osum=osum, pool=pl, ref=ref, bound=bound, keep=keep, rec=rec)


@pytest.mark.gpu
@pytest.mark.parametrize('case', FWD, ids=['-'.join(map(str, c[:4])) + '-k%s-v%s' % (c[7], c[8]) for c in FWD])
def test_fwd_gen_vs_oracle(case):
    lib = _hip.load()
    rng = np.random.default_rng(hash(case) % (1 << 31))
    r = _run_fwd(lib, rng, case)
    n, H, Cout = case[0], case[1], case[6]
    out = r['out'].get().reshape(n, H, H, Cout)
    _close(out, r['ref'], r['bound'], what='out')
    ref = r['ref'].reshape(-1, Cout)
    sums = r['osum'].get().reshape(S, 2 * Cout)
    assert (sums[5:] == 0).all()                               # out_nslot = 5 slots used
    s = sums.sum(0)
    _sum_close(s[:Cout], ref.sum(0), np.abs(ref).sum(0) + r['bound'].reshape(-1, Cout).sum(0) * 2e-6, 'sum')
    _sum_close(s[Cout:], (ref ** 2).sum(0), (ref ** 2).sum(0), 'sum of squares')
    if case[9]:
        pooled = _oracle().pool2(out.astype(np.float64))       # the max-pool of the stored sums, exactly
        assert np.array_equal(r['pool'].get().reshape(pooled.shape), pooled)
    for b in (r['out'], r['osum']) + ((r['pool'],) if case[9] else ()):
        assert b.guards_ok()


# ------------------------------------------------------------------ input gradients
# dgrad-horz: (n, H, Cg, Cp, kh x kw, prev, extra, accumulate)
HORZ = [
    (3, 16, 32, 16, (5, 5), True, True, False),
    (5, 4, 128, 64, (4, 4), True, False, True),
    (2, 8, 16, 32, (2, 2), False, True, True),
    (2, 32, 16, 16, (7, 7), True, False, False),
    (3, 8, 64, 128, (1, 1), True, True, False),
    (2, 16, 48, 32, (3, 3), False, False, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', HORZ, ids=['h%d-%d-%d-k%d-%s%s%s' % (c[1], c[2], c[3], c[4][0], 'p' if c[5] else 'r',
                                                                       'x' if c[6] else '', 'a' if c[7] else '') for c in HORZ])
def test_dgrad_horz_gen_vs_oracle(case):
    import torch
    import hiputil as U
    lib = _hip.load()
    n, H, Cg, Cp, k, prev, extra, acc = case
    rng = np.random.default_rng(sum(map(hash, map(str, case))) % (1 << 31))
    g, g64 = U.f32(rng.standard_normal((n, H, H, Cg)))
    w, w64 = U.f32(rng.standard_normal(k + (Cp, Cg)) * 0.2)
    gd, wd = U.dev(g), U.dev(w)
    dy, bound = _dconv(g64, w64, Cp)
    rec = _hip.DgradHorzArgs()
    rec.g, rec.Cg, rec.w_pack = gd.data_ptr(), Cg, wd.data_ptr()
    keep = []
    if extra:
        e, e64 = U.f32(rng.standard_normal((n, H, H, Cp)))
        ed = U.dev(e); keep.append(ed)
        rec.dy_extra = ed.data_ptr()
        dy, bound = dy + e64, bound + np.abs(e64)
    out = U.Guarded(n * H * H * Cp)
    prior64 = np.zeros((n, H, H, Cp))
    if acc:
        prior, prior64 = U.f32(rng.standard_normal((n, H, H, Cp)))
        out.fill(prior)
    else:
        out.fill(float('nan'))
    red = None
    if prev:
        bm = U.BnMap(rng, (n, H, H, Cp), 8)
        ctx = bm.ctx(red_nslot=3)
        red = U.Guarded(S * 2 * Cp, dtype=torch.float64); red.fill(0.0)
        rec.prev, rec.red_out = C.pointer(ctx), red.ptr()
        keep += [bm, ctx]
        dz = dy * (bm.y > 0)
        want = prior64 + dz
        bound = bound * (bm.y > 0) + np.abs(prior64)
    else:
        want = prior64 + dy
        bound = bound + np.abs(prior64)
    rec.out, rec.accumulate = out.ptr(), 1 if acc else 0
    rec.n, rec.H, rec.W, rec.Cout = n, H, H, Cp
    _hip.check(lib.mpnn_msconv_dgrad_horz_gen(C.byref(rec), *k, U.stream()), 'dgrad_horz_gen')
    torch.cuda.synchronize()
    _close(out.get().reshape(want.shape), want, bound, what='out')
    assert out.guards_ok()
    if prev:
        got = red.get().reshape(S, 2 * Cp)
        assert (got[3:] == 0).all()
        want_red = U.red_of(dz, bm.xh)
        terms = np.concatenate([np.abs(dz).reshape(-1, Cp).sum(0), np.abs(dz * bm.xh).reshape(-1, Cp).sum(0)])
        _sum_close(got.sum(0), want_red, terms + 1e-3, 'red_out')
        assert red.guards_ok()


# dgrad-vert: (n, coarse H, Cg, Cf, kvh x kvw, fine_has_dz)
VERT = [
    (5, 4, 64, 32, (5, 5), True),
    (2, 8, 32, 16, (2, 2), False),
    (2, 16, 16, 16, (7, 7), True),
    (3, 4, 128, 128, (1, 1), True),
    (2, 8, 16, 64, (4, 4), False),
    (3, 8, 16, 16, (3, 3), True, 'ties'),       # the finer map on a grid of 1/2: tied 2x2 maxima go to the FIRST one
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', VERT, ids=['h%d-%d-%d-k%d-dz%d%s' % (c[1], c[2], c[3], c[4][0], c[5], '-ties' if len(c) > 6 else '')
                                            for c in VERT])
def test_dgrad_vert_gen_vs_oracle(case):
    import torch
    import hiputil as U
    lib = _hip.load()
    O = _oracle()
    n, H, Cg, Cf, k, has_dz = case[:6]
    rng = np.random.default_rng(sum(map(hash, map(str, case))) % (1 << 31))
    g, g64 = U.f32(rng.standard_normal((n, H, H, Cg)))
    w, w64 = U.f32(rng.standard_normal(k + (Cf, Cg)) * 0.2)
    gd, wd = U.dev(g), U.dev(w)
    dv, bound = _dconv(g64, w64, Cf)
    if len(case) > 6:                                    # max-pool ties (no ReLU decision of the map is used here)
        bm = U.BnMap(rng, (n, 2 * H, 2 * H, Cf), 8, s=U.grid_map(np.random.default_rng(0), (n, 2 * H, 2 * H, Cf)))
        share, first, later, _ = U.tie_stats(bm.s)
        assert share >= 0.25 and first == {0, 1, 2} and later == {1, 2, 3}
    else:
        bm = U.BnMap(rng, (n, 2 * H, 2 * H, Cf), 8)
    buf = U.Guarded(n * 4 * H * H * Cf)
    red64 = None
    if has_dz:
        dz, dz64 = U.f32(rng.standard_normal((n, 2 * H, 2 * H, Cf)))
        red64 = rng.standard_normal(2 * Cf) * 10
        buf.fill(dz)
        ctx = bm.ctx(red=red64, red_nslot=5)
        base = bm.apply(dz64, red64)
        bbound = np.abs(bm.gamma64 * bm.rstd) * (np.abs(dz64) + np.abs(red64[:Cf]) / bm.cnt + np.abs(bm.xh * red64[Cf:]) / bm.cnt)
    else:
        buf.fill(float('nan'))
        ctx = bm.ctx()
        base, bbound = 0.0, 0.0
    want = base + O.pool2_bwd(bm.s64, dv)
    wbound = bbound + O.pool2_bwd(bm.s64, bound)
    rec = _hip.DgradVertArgs()
    rec.g, rec.Cg, rec.w_pack, rec.fine = gd.data_ptr(), Cg, wd.data_ptr(), C.pointer(ctx)
    rec.fine_has_dz, rec.dz_g_fine = 1 if has_dz else 0, buf.ptr()
    rec.n, rec.H, rec.W, rec.Cout = n, H, H, Cf
    _hip.check(lib.mpnn_msconv_dgrad_vert_gen(C.byref(rec), *k, U.stream()), 'dgrad_vert_gen')
    torch.cuda.synchronize()
    _close(buf.get().reshape(want.shape), want, wbound, rel=4e-6, what='g_fine')
    assert buf.guards_ok()


# ------------------------------------------------------------------ weight gradients
# (n, H, Cin, act mode, shift, Cv, Cout, horz, vert, n_split)
WGRAD = [
    (2, 32, 3, 'img', 1, 0, 16, (5, 5), None, 1),
    (3, 16, 16, 'batch', 0, 16, 32, (2, 2), (2, 2), 5),
    (2, 8, 64, 'batch', 0, 32, 64, (7, 7), (7, 7), 3),
    (5, 4, 128, 'batch', 0, 64, 128, (4, 4), (5, 5), 2),
    (3, 8, 1, 'img', 2, 0, 16, (1, 1), None, 4),            # (more splits than tiles: the empty splits write zeros)
    (2, 16, 32, 'moving', 0, 16, 80, (3, 3), (6, 6), 1),
]


def _run_wgrad(lib, rng, case):
    import torch
    import hiputil as U
    O = _oracle()
    n, H, Cin, mode, shift, Cv, Cout, kh, kv, n_split = case
    a, act64, keep = _act(rng, n, H, Cin, mode, shift)
    g, g64 = U.f32(rng.standard_normal((n, H, H, Cout)))
    gd = U.dev(g)
    sizes = [kh[0] * kh[1] * Cin * Cout, (kv[0] * kv[1] * Cv * Cout) if Cv else 0, Cout]
    offs = [0, sizes[0], sizes[0] + sizes[1]]
    total = sum(sizes)
    stride = (total + 3) // 4 * 4
    grads = U.Guarded(total); grads.fill(float('nan'))
    slab = grads if n_split == 1 else U.Guarded(n_split * stride)
    if n_split > 1:
        slab.fill(float('nan'))
    rec = _hip.WgradArgs()
    rec.a = a
    rec.g = gd.data_ptr()
    rec.dwa, rec.db = slab.ptr(offs[0]), slab.ptr(offs[2])
    want = [O.conv_same_bwd(act64, np.zeros(kh + (Cin, Cout)), g64)[1]]
    bound = [O.conv_same_bwd(np.abs(act64), np.zeros(kh + (Cin, Cout)), np.abs(g64))[1]]
    if Cv:
        v, v64 = U.f32(rng.standard_normal((n, H, H, Cv)))
        vd = U.dev(v); keep.append(vd)
        rec.v, rec.Cv, rec.dwv = vd.data_ptr(), Cv, slab.ptr(offs[1])
        want.append(O.conv_same_bwd(v64, np.zeros(kv + (Cv, Cout)), g64)[1])
        bound.append(O.conv_same_bwd(np.abs(v64), np.zeros(kv + (Cv, Cout)), np.abs(g64))[1])
    want.append(g64.reshape(-1, Cout).sum(0))
    bound.append(np.abs(g64).reshape(-1, Cout).sum(0))
    rec.split_stride = stride if n_split > 1 else 0
    rec.n, rec.H, rec.W, rec.Cout, rec.n_split = n, H, H, Cout, n_split
    kvv = kv or (0, 0)
    _hip.check(lib.mpnn_msconv_wgrad_gen(C.byref(rec), *kh, *kvv, U.stream()), 'wgrad_gen')
    if n_split > 1:
        tab = []
        for o, sz in zip(offs, sizes):
            item = _hip.slab_item_size(n_split)
            for k in range(0, sz, item):
                tab += [o + k, o + k, min(item, sz - k), n_split, stride, 0]
        t = U.dev(np.array(tab, np.int32), torch.int32)
        _hip.check(lib.mpnn_slab_reduce(slab.ptr(), grads.ptr(), t.data_ptr(), len(tab) // 6, U.stream()), 'slab_reduce')
    torch.cuda.synchronize()
    got = grads.get()
    parts = [got[offs[0]:offs[0] + sizes[0]]] + ([got[offs[1]:offs[2]]] if Cv else []) + [got[offs[2]:]]
    return parts, want, bound, [grads, slab] + keep


@pytest.mark.gpu
@pytest.mark.parametrize('case', WGRAD, ids=['h%d-%d-%s-%d-k%s-v%s-s%d' % (c[1], c[2], c[3], c[6], c[7][0], c[8] and c[8][0], c[9])
                                             for c in WGRAD])
def test_wgrad_gen_vs_oracle(case):
    lib = _hip.load()
    rng = np.random.default_rng(sum(map(hash, map(str, case))) % (1 << 31))
    parts, want, bound, bufs = _run_wgrad(lib, rng, case)
    for got, w, b, name in zip(parts, want, bound, ['dw_horz', 'dw_vert', 'db'] if len(parts) == 3 else ['dw_horz', 'db']):
        _close(got.reshape(w.shape), w, b, rel=4e-6, what=name)
    assert all(b.guards_ok() for b in bufs[:2])


@pytest.mark.gpu
def test_wgrad_gen_split_sums_are_deterministic():
    """Two launches of the same record give the same bits (no fp32 atomics); different splits agree to rounding."""
    lib = _hip.load()
    case = (3, 16, 16, 'batch', 0, 16, 32, (5, 5), (5, 5), 4)
    p1, want, bound, _ = _run_wgrad(lib, np.random.default_rng(11), case)
    p2, _, _, _ = _run_wgrad(lib, np.random.default_rng(11), case)
    assert all(np.array_equal(a, b) for a, b in zip(p1, p2))
    p3, _, _, _ = _run_wgrad(lib, np.random.default_rng(11), case[:9] + (1,))
    for a, b, bd in zip(p1, p3, bound):
        _close(a.reshape(bd.shape), b.reshape(bd.shape).astype(np.float64), bd, rel=4e-6, what='split 4 vs 1')


# ------------------------------------------------------------------ 3x3: the general forms against the tuned ones
@pytest.mark.gpu
@pytest.mark.parametrize('H,Cin,Cv,Cout', [(16, 32, 16, 64), (4, 32, 64, 64), (32, 3, 0, 16)])
def test_gen_3x3_matches_tuned(H, Cin, Cv, Cout):
    import hiputil as U
    lib = _hip.load()
    O = _oracle()
    rng = np.random.default_rng(H * 1000 + Cin)
    n = 4
    img = Cin in (1, 3)
    bm = None if img else U.BnMap(rng, (n, H, H, Cin), 8)
    x = rng.random((n, H, H, Cin)).astype(np.float32) if img else bm.s
    bn = None if img else bm.dev
    mode = _hip.ACT_IDENTITY if img else _hip.ACT_BN_BATCH
    cnt = 1 if img else bm.cnt
    act64 = x.astype(np.float64) if img else np.maximum(bm.y, 0.0)
    wh = (rng.standard_normal((3, 3, Cin, Cout)) * 0.2).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    vfine = rng.standard_normal((n, 2 * H, 2 * H, Cv)).astype(np.float32) if Cv else None
    wv = (rng.standard_normal((3, 3, Cv, Cout)) * 0.2).astype(np.float32) if Cv else None
    # tuned forward (hiputil pools the finer map itself; the tuned pool_out needs maps of 8 and more)
    t_out, t_sum = U.conv_fwd(x, wh, b, v=vfine, wv=wv, bn=bn, mode=mode, bn_cnt=cnt)[:2]
    import torch
    rec = _hip.ConvFwdArgs()
    xd, whd, bd = U.dev(x), U.dev(wh), U.dev(b)
    rec.a = _hip.act(xd, Cin, mode, 0, bn, cnt)
    rec.wa_pack, rec.bias = whd.data_ptr(), bd.data_ptr()
    keep = [xd, whd, bd]
    bound = _conv_abs(act64, wh.astype(np.float64)) + np.abs(b)
    if Cv:
        vp = U.pool2_np(vfine)
        vd, wvd = U.dev(vp), U.dev(wv)
        keep += [vd, wvd]
        rec.v, rec.Cv, rec.wv_pack = vd.data_ptr(), Cv, wvd.data_ptr()
        bound = bound + _conv_abs(vp.astype(np.float64), wv.astype(np.float64))
    out = torch.empty((n, H, H, Cout), device=U.DEV)
    osum = torch.zeros(S * 2 * Cout, device=U.DEV, dtype=torch.float64)
    pool = torch.empty((n, H // 2, H // 2, Cout), device=U.DEV)
    rec.out, rec.out_sum, rec.out_nslot, rec.pool_out = out.data_ptr(), osum.data_ptr(), S, pool.data_ptr()
    rec.n, rec.H, rec.W, rec.Cout = n, H, H, Cout
    _hip.check(lib.mpnn_msconv_fwd_gen(C.byref(rec), 3, 3, 3, 3, U.stream()), 'fwd_gen')
    torch.cuda.synchronize()
    _close(out.cpu().numpy(), t_out.astype(np.float64), bound, rel=1e-6, what='fwd vs tuned')
    g_pool = pool.cpu().numpy()
    assert np.array_equal(g_pool, O.pool2(out.cpu().numpy().astype(np.float64)).astype(np.float32))
    s = U.unslot(osum, 2 * Cout)
    assert np.allclose(s, t_sum, rtol=1e-5, atol=1e-3)
    # weight gradients, one split on both sides
    g = rng.standard_normal((n, H, H, Cout)).astype(np.float32)
    t_dwa, t_dwv, t_db = U.wgrad(x, g, v=vfine, bn=bn, mode=mode, bn_cnt=cnt, n_split=1)
    gd = U.dev(g)
    total = 9 * Cin * Cout + 9 * Cv * Cout + Cout
    buf = torch.full((total,), float('nan'), device=U.DEV)
    w = _hip.WgradArgs()
    w.a = rec.a
    w.g = gd.data_ptr()
    w.dwa, w.db = buf.data_ptr(), buf[9 * Cin * Cout + 9 * Cv * Cout:].data_ptr()
    if Cv:
        w.v, w.Cv, w.dwv = rec.v, Cv, buf[9 * Cin * Cout:].data_ptr()
    w.n, w.H, w.W, w.Cout, w.n_split = n, H, H, Cout, 1
    _hip.check(lib.mpnn_msconv_wgrad_gen(C.byref(w), 3, 3, 3, 3, U.stream()), 'wgrad_gen')
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    wb = O.conv_same_bwd(np.abs(act64), np.zeros((3, 3, Cin, Cout)), np.abs(g.astype(np.float64)))[1]
    _close(got[:9 * Cin * Cout].reshape(wb.shape), t_dwa.astype(np.float64), wb, rel=4e-6, what='dW vs tuned')
    assert np.allclose(got[-Cout:], t_db, rtol=1e-5, atol=1e-4)
    if img:
        return
    # input gradients: dgrad-horz with the producer's BatchNorm, dgrad-vert onto this map as the finer scale
    wt = (rng.standard_normal((3, 3, Cin, Cout)) * 0.2).astype(np.float32)
    t_dz, t_red = U.dgrad_horz(g, wt, s_prev=bm.s, bn=bm.dev, cnt=bm.cnt)
    h = _hip.DgradHorzArgs()
    wtd = U.dev(wt)
    outh = torch.full((n, H, H, Cin), float('nan'), device=U.DEV)
    red = torch.zeros(S * 2 * Cin, device=U.DEV, dtype=torch.float64)
    ctx = U.bn_ctx(bm.sd, Cin, bm.dev, bm.cnt)
    h.g, h.Cg, h.w_pack, h.out, h.prev, h.red_out = gd.data_ptr(), Cout, wtd.data_ptr(), outh.data_ptr(), C.pointer(ctx), red.data_ptr()
    h.n, h.H, h.W, h.Cout = n, H, H, Cin
    _hip.check(lib.mpnn_msconv_dgrad_horz_gen(C.byref(h), 3, 3, U.stream()), 'dgrad_horz_gen')
    torch.cuda.synchronize()
    _, hb = _dconv(np.abs(g.astype(np.float64)), np.abs(wt.astype(np.float64)), Cin)
    _close(outh.cpu().numpy(), t_dz.astype(np.float64), hb, rel=1e-6, what='dgrad-horz vs tuned')
    assert np.allclose(U.unslot(red, 2 * Cin), t_red, rtol=1e-4, atol=1e-3)
