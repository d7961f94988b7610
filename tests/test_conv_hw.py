"""The any-map forms of the general multiscale conv kernels (csrc/conv_gen.hip: mpnn_msconv_*_hw, maps of any size from 1
to 256 per axis) through the C ABI, on the GPU.

Member by member against the float64 restatement (oracle/np_ops.py), built on tests/hiputil.py exactly as
tests/test_conv_gen.py is: every output between sentinel guards (Guarded), plain-store outputs pre-filled with NaN (an
element a masked tile forgot stays NaN; an element stored beyond the map's edge lands in a neighbour row, another image
or a guard), BatchNorm inputs drawn so that no ReLU / max-pool decision is within 1e-3 of a tie (BnMap).  The tolerances
are those of tests/test_conv_gen.py: 2e-6 of the sum of the absolute values of the terms of each output (4e-6 where that
file uses 4e-6: the pooled input gradient and the weight gradients), 1e-5 for the fp64 sums.

The maps: odd and one-pixel sides (3x3, 7x7, 3x5, 1x2), sides that are no multiple of the tile (6, 12, 20, 24, 40),
rectangles in both orientations (16x64, 64x16), ragged batches (5 and 1 images against tiles of 1, 2 or 4 images),
filters clipped to the map with kh != kw, pyramid shifts 1..3 on the image operand.  The pooled output and the vert input
gradient only appear where the pooled map is even on both axes.

On the shapes both families accept, _hw and _gen write equal bits (they are the same kernels with the same pixel-to-lane
assignment); two runs of mpnn_msconv_wgrad_hw write equal bits.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

from lib import _hip

S = _hip.BN_SLOTS
pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import np_ops as O
    return O


def _fn(lib, name, fam):
    return getattr(lib, 'mpnn_msconv_%s_%s' % (name, fam))


def _conv_abs(x, w):
    return _oracle().conv_same(np.abs(x), np.abs(w))


def _dconv(g, w, cin):
    """Input gradient of conv_same with filter w (HWIO) for output gradient g, and its absolute bound."""
    O = _oracle()
    n, H, W, _ = g.shape
    z = np.zeros((n, H, W, cin))
    return O.conv_same_bwd(z, w, g)[0], O.conv_same_bwd(z, np.abs(w), np.abs(g))[0]


def _act(rng, n, H, W, C_, mode, shift, nslot=8):
    """An input operand: (device act, fp64 activation as the kernel sees it at H x W, keep-alive)."""
    import hiputil as U
    if C_ in (1, 3):
        x, x64 = U.f32(rng.random((n, H << shift, W << shift, C_)))
        xd = U.dev(x)
        return _hip.act(xd, C_, _hip.ACT_IDENTITY, shift), x64[:, ::1 << shift, ::1 << shift], [xd]
    if mode == 'id':
        x, x64 = U.f32(rng.standard_normal((n, H, W, C_)))
        xd = U.dev(x)
        return _hip.act(xd, C_, _hip.ACT_IDENTITY, 0), x64, [xd]
    if mode == 'batch':
        bm = U.BnMap(rng, (n, H, W, C_), nslot)
        return _hip.act(bm.sd, C_, _hip.ACT_BN_BATCH, 0, bm.dev, bm.cnt), np.maximum(bm.y, 0.0), [bm]
    s, s64 = U.f32(rng.standard_normal((n, H, W, C_)))            # moving averages
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


def _seed(case):
    return zlib.crc32(repr(case).encode())


def _id(case):
    return '-'.join(str(f).replace(' ', '').replace('(', '').replace(')', '').replace(',', 'x') for f in case)


# ------------------------------------------------------------------ forward
# (n, H, W, Cin, act mode, shift, Cv, Cout, horz kh x kw, vert kvh x kvw, pool)
FWD = [
    (5, 3, 3, 16, 'batch', 0, 16, 16, (3, 3), (3, 3), False),
    (5, 6, 6, 3, 'img', 2, 0, 16, (3, 3), None, True),
    (1, 7, 7, 48, 'moving', 0, 0, 80, (5, 5), None, False),
    (5, 12, 12, 16, 'batch', 0, 16, 80, (4, 4), (4, 4), True),
    (1, 24, 24, 3, 'img', 1, 0, 16, (5, 5), None, True),
    (5, 3, 5, 48, 'id', 0, 16, 16, (3, 5), (5, 5), False),        # (supp 5 clipped to the 3x5 map: kh != kw)
    (5, 6, 10, 16, 'batch', 0, 16, 16, (5, 5), (5, 5), True),
    (1, 12, 20, 3, 'img', 3, 0, 16, (3, 3), None, True),
    (5, 24, 40, 3, 'img', 1, 0, 16, (4, 4), None, True),
    (1, 16, 64, 16, 'moving', 0, 16, 80, (3, 3), (3, 3), True),
    (5, 64, 16, 3, 'img', 0, 0, 16, (3, 3), None, True),
    (5, 2, 4, 48, 'batch', 0, 16, 80, (2, 4), (5, 5), True),      # (pooled to 1x2)
    (5, 1, 2, 16, 'id', 0, 16, 16, (1, 2), (3, 3), False),
    (1, 1, 2, 3, 'img', 3, 0, 16, (1, 2), None, False),
    (5, 7, 7, 16, 'id', 0, 16, 16, (4, 4), (5, 5), False),
]


def _run_fwd(lib, rng, case, fam='hw'):
    import torch
    import hiputil as U
    n, H, W, Cin, mode, shift, Cv, Cout, kh, kv, pool = case
    a, act64, keep = _act(rng, n, H, W, Cin, mode, shift)
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
        v, v64 = U.f32(rng.standard_normal((n, H, W, Cv)))
        wv, wv64 = U.f32(rng.standard_normal(kv + (Cv, Cout)) * 0.2)
        vd, wvd = U.dev(v), U.dev(wv)
        keep += [vd, wvd]
        rec.v, rec.Cv, rec.wv_pack = vd.data_ptr(), Cv, wvd.data_ptr()
        ref = ref + _oracle().conv_same(v64, wv64)
        bound = bound + _conv_abs(v64, wv64)
    out = U.Guarded(n * H * W * Cout); out.fill(float('nan'))
    osum = U.Guarded(S * 2 * Cout, dtype=torch.float64); osum.fill(0.0)
    pl = U.Guarded(n * (H // 2) * (W // 2) * Cout) if pool else None
    if pl is not None:
        pl.fill(float('nan'))
    rec.out, rec.out_sum, rec.out_nslot = out.ptr(), osum.ptr(), 5
    rec.pool_out = pl.ptr() if pl is not None else None
    rec.n, rec.H, rec.W, rec.Cout = n, H, W, Cout
    _hip.check(_fn(lib, 'fwd', fam)(C.byref(rec), *kh, *(kv or (0, 0)), U.stream()), 'msconv_fwd_' + fam)
    torch.cuda.synchronize()
    return dict(out=out, osum=osum, pool=pl, ref=ref, bound=bound, keep=keep, rec=rec)


@pytest.mark.parametrize('case', FWD, ids=list(map(_id, FWD)))
def test_fwd_hw_vs_oracle(case):
    lib = _hip.load()
    r = _run_fwd(lib, np.random.default_rng(_seed(case)), case)
    n, H, W, Cout = case[0], case[1], case[2], case[7]
    out = r['out'].get().reshape(n, H, W, Cout)
    _close(out, r['ref'], r['bound'], what='out')
    ref = r['ref'].reshape(-1, Cout)
    sums = r['osum'].get().reshape(S, 2 * Cout)
    assert (sums[5:] == 0).all()                               # out_nslot = 5 slots used
    s = sums.sum(0)                                            # (pixels of a tile beyond the map's edge add nothing)
    _sum_close(s[:Cout], ref.sum(0), np.abs(ref).sum(0) + r['bound'].reshape(-1, Cout).sum(0) * 2e-6, 'sum')
    _sum_close(s[Cout:], (ref ** 2).sum(0), (ref ** 2).sum(0), 'sum of squares')
    if case[10]:
        pooled = _oracle().pool2(out.astype(np.float64))       # the max-pool of the stored sums, exactly
        assert np.array_equal(r['pool'].get().reshape(pooled.shape), pooled)
    for b in (r['out'], r['osum']) + ((r['pool'],) if case[10] else ()):
        assert b.guards_ok()


# ------------------------------------------------------------------ input gradients
# dgrad-horz: (n, H, W, Cg, Cp, kh x kw, prev, extra, accumulate)
HORZ = [
    (5, 3, 3, 16, 16, (3, 3), True, True, False),
    (5, 6, 6, 80, 48, (4, 4), True, False, True),
    (1, 7, 7, 16, 16, (5, 5), False, True, True),
    (5, 12, 12, 16, 48, (3, 3), True, False, False),
    (1, 24, 24, 16, 16, (5, 5), True, True, False),
    (5, 3, 5, 80, 16, (3, 5), True, False, False),
    (5, 6, 10, 16, 16, (5, 5), False, False, False),
    (1, 12, 20, 16, 48, (4, 4), True, True, True),
    (5, 24, 40, 16, 16, (3, 3), True, False, False),
    (1, 16, 64, 80, 16, (3, 3), True, False, False),
    (5, 64, 16, 16, 16, (4, 4), False, True, False),
    (5, 2, 4, 16, 48, (2, 4), True, True, False),
    (5, 1, 2, 80, 16, (1, 2), False, False, True),
]


def _run_horz(lib, rng, case, fam='hw'):
    import torch
    import hiputil as U
    n, H, W, Cg, Cp, k, prev, extra, acc = case
    g, g64 = U.f32(rng.standard_normal((n, H, W, Cg)))
    w, w64 = U.f32(rng.standard_normal(k + (Cp, Cg)) * 0.2)
    gd, wd = U.dev(g), U.dev(w)
    dy, bound = _dconv(g64, w64, Cp)
    rec = _hip.DgradHorzArgs()
    rec.g, rec.Cg, rec.w_pack = gd.data_ptr(), Cg, wd.data_ptr()
    keep = [gd, wd]
    if extra:
        e, e64 = U.f32(rng.standard_normal((n, H, W, Cp)))
        ed = U.dev(e); keep.append(ed)
        rec.dy_extra = ed.data_ptr()
        dy, bound = dy + e64, bound + np.abs(e64)
    out = U.Guarded(n * H * W * Cp)
    prior64 = np.zeros((n, H, W, Cp))
    if acc:
        prior, prior64 = U.f32(rng.standard_normal((n, H, W, Cp)))
        out.fill(prior)
    else:
        out.fill(float('nan'))
    red = bm = dz = None
    if prev:
        bm = U.BnMap(rng, (n, H, W, Cp), 8)
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
    rec.n, rec.H, rec.W, rec.Cout = n, H, W, Cp
    _hip.check(_fn(lib, 'dgrad_horz', fam)(C.byref(rec), *k, U.stream()), 'dgrad_horz_' + fam)
    torch.cuda.synchronize()
    return dict(out=out, red=red, want=want, bound=bound, bm=bm, dz=dz, keep=keep)


@pytest.mark.parametrize('case', HORZ, ids=list(map(_id, HORZ)))
def test_dgrad_horz_hw_vs_oracle(case):
    import hiputil as U
    lib = _hip.load()
    Cp, prev = case[4], case[6]
    r = _run_horz(lib, np.random.default_rng(_seed(case)), case)
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
    (5, 3, 3, 16, 16, (3, 3), True),
    (5, 6, 6, 80, 16, (4, 4), False),
    (1, 7, 7, 16, 48, (5, 5), True),
    (5, 12, 12, 16, 16, (3, 3), True),
    (5, 3, 5, 16, 48, (5, 5), False),
    (1, 6, 10, 80, 16, (5, 5), True),
    (5, 12, 20, 16, 16, (4, 4), True),
    (1, 8, 32, 16, 16, (3, 3), False),
    (5, 32, 8, 16, 16, (3, 3), True),
    (5, 2, 4, 16, 16, (5, 5), True),
    (5, 1, 2, 80, 48, (3, 3), False),
    (3, 6, 10, 16, 16, (3, 3), True, 'ties'),   # the finer map on a grid of 1/2: tied 2x2 maxima go to the FIRST one
]


def _run_vert(lib, rng, case, fam='hw'):
    import torch
    import hiputil as U
    O = _oracle()
    n, H, W, Cg, Cf, k, has_dz = case[:7]
    g, g64 = U.f32(rng.standard_normal((n, H, W, Cg)))
    w, w64 = U.f32(rng.standard_normal(k + (Cf, Cg)) * 0.2)
    gd, wd = U.dev(g), U.dev(w)
    dv, bound = _dconv(g64, w64, Cf)
    if len(case) > 7:                                    # max-pool ties (no ReLU decision of the map is used here)
        bm = U.BnMap(rng, (n, 2 * H, 2 * W, Cf), 8, s=U.grid_map(np.random.default_rng(0), (n, 2 * H, 2 * W, Cf)))
        share, first, later, _ = U.tie_stats(bm.s)
        assert share >= 0.25 and first == {0, 1, 2} and later == {1, 2, 3}
    else:
        bm = U.BnMap(rng, (n, 2 * H, 2 * W, Cf), 8)
    buf = U.Guarded(n * 4 * H * W * Cf)
    if has_dz:
        dz, dz64 = U.f32(rng.standard_normal((n, 2 * H, 2 * W, Cf)))
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
    rec.n, rec.H, rec.W, rec.Cout = n, H, W, Cf
    _hip.check(_fn(lib, 'dgrad_vert', fam)(C.byref(rec), *k, U.stream()), 'dgrad_vert_' + fam)
    torch.cuda.synchronize()
    return dict(buf=buf, want=want, bound=wbound, keep=[gd, wd, bm, ctx])


@pytest.mark.parametrize('case', VERT, ids=list(map(_id, VERT)))
def test_dgrad_vert_hw_vs_oracle(case):
    lib = _hip.load()
    r = _run_vert(lib, np.random.default_rng(_seed(case)), case)
    _close(r['buf'].get().reshape(r['want'].shape), r['want'], r['bound'], rel=4e-6, what='g_fine')
    assert r['buf'].guards_ok()


# ------------------------------------------------------------------ weight gradients
# (n, H, W, Cin, act mode, shift, Cv, Cout, horz, vert, n_split)
WGRAD = [
    (5, 3, 3, 16, 'batch', 0, 16, 16, (3, 3), (3, 3), 2),
    (5, 6, 6, 3, 'img', 2, 0, 16, (3, 3), None, 3),
    (1, 7, 7, 48, 'moving', 0, 0, 80, (5, 5), None, 1),
    (5, 12, 12, 16, 'batch', 0, 16, 80, (4, 4), (4, 4), 5),
    (1, 24, 24, 3, 'img', 1, 0, 16, (5, 5), None, 4),
    (5, 3, 5, 48, 'id', 0, 16, 16, (3, 5), (5, 5), 2),
    (5, 6, 10, 16, 'batch', 0, 16, 16, (5, 5), (5, 5), 1),
    (1, 12, 20, 3, 'img', 3, 0, 16, (3, 3), None, 7),           # (more splits than tiles: the empty splits write zeros)
    (5, 24, 40, 3, 'img', 1, 0, 16, (4, 4), None, 6),
    (1, 16, 64, 16, 'moving', 0, 16, 80, (3, 3), (3, 3), 3),
    (5, 64, 16, 3, 'img', 0, 0, 16, (3, 3), None, 8),
    (5, 2, 4, 48, 'batch', 0, 16, 80, (2, 4), (5, 5), 2),
    (5, 1, 2, 16, 'id', 0, 16, 16, (1, 2), (3, 3), 1),
]


def _run_wgrad(lib, rng, case, fam='hw'):
    import torch
    import hiputil as U
    O = _oracle()
    n, H, W, Cin, mode, shift, Cv, Cout, kh, kv, n_split = case
    a, act64, keep = _act(rng, n, H, W, Cin, mode, shift)
    g, g64 = U.f32(rng.standard_normal((n, H, W, Cout)))
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
        v, v64 = U.f32(rng.standard_normal((n, H, W, Cv)))
        vd = U.dev(v); keep.append(vd)
        rec.v, rec.Cv, rec.dwv = vd.data_ptr(), Cv, slab.ptr(offs[1])
        want.append(O.conv_same_bwd(v64, np.zeros(kv + (Cv, Cout)), g64)[1])
        bound.append(O.conv_same_bwd(np.abs(v64), np.zeros(kv + (Cv, Cout)), np.abs(g64))[1])
    want.append(g64.reshape(-1, Cout).sum(0))
    bound.append(np.abs(g64).reshape(-1, Cout).sum(0))
    rec.split_stride = stride if n_split > 1 else 0
    rec.n, rec.H, rec.W, rec.Cout, rec.n_split = n, H, W, Cout, n_split
    _hip.check(_fn(lib, 'wgrad', fam)(C.byref(rec), *kh, *(kv or (0, 0)), U.stream()), 'wgrad_' + fam)
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


@pytest.mark.parametrize('case', WGRAD, ids=list(map(_id, WGRAD)))
def test_wgrad_hw_vs_oracle(case):
    lib = _hip.load()
    parts, want, bound, bufs = _run_wgrad(lib, np.random.default_rng(_seed(case)), case)
    for got, w, b, name in zip(parts, want, bound, ['dw_horz', 'dw_vert', 'db'] if len(parts) == 3 else ['dw_horz', 'db']):
        _close(got.reshape(w.shape), w, b, rel=4e-6, what=name)
    assert all(b.guards_ok() for b in bufs[:2])


def test_wgrad_hw_twice_gives_equal_bits():
    """Two launches of the same record give the same bits (no fp32 atomics), on a map whose tiles hang over both edges."""
    lib = _hip.load()
    case = (5, 12, 20, 16, 'batch', 0, 16, 32, (5, 5), (5, 5), 4)
    p1, _, _, _ = _run_wgrad(lib, np.random.default_rng(11), case)
    p2, _, _, _ = _run_wgrad(lib, np.random.default_rng(11), case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(p1, p2))


# ------------------------------------------------------------------ _hw == _gen, bit for bit, where both are defined
@pytest.mark.parametrize('H', [4, 8, 16, 32])
def test_hw_and_gen_give_equal_bits(H):
    lib = _hip.load()
    n = 5 if H < 32 else 2
    both = lambda run, case, seed: [run(lib, np.random.default_rng(seed), case, fam) for fam in ('hw', 'gen')]
    a, b = both(_run_fwd, (n, H, H, 16, 'batch', 0, 16, 80, (5, 5), (4, 4), True), 1)
    for k in ('out', 'osum', 'pool'):
        assert a[k].get().tobytes() == b[k].get().tobytes(), 'fwd ' + k
    a, b = both(_run_fwd, (n, H, H, 3, 'img', 1, 0, 16, (3, 3), None, False), 2)
    for k in ('out', 'osum'):
        assert a[k].get().tobytes() == b[k].get().tobytes(), 'fwd (image) ' + k
    a, b = both(_run_horz, (n, H, H, 80, 16, (5, 5), True, True, False), 3)
    for k in ('out', 'red'):
        assert a[k].get().tobytes() == b[k].get().tobytes(), 'dgrad-horz ' + k
    a, b = both(_run_horz, (n, H, H, 16, 48, (2, 2), False, False, True), 4)
    assert a['out'].get().tobytes() == b['out'].get().tobytes(), 'dgrad-horz (raw)'
    a, b = both(_run_vert, (n, H, H, 16, 48, (5, 5), True), 5)
    assert a['buf'].get().tobytes() == b['buf'].get().tobytes(), 'dgrad-vert'
    a, b = both(_run_wgrad, (n, H, H, 16, 'batch', 0, 16, 80, (5, 5), (4, 4), 3), 6)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])), 'wgrad'
