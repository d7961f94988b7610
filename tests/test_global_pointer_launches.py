"""The record-driven launches at their smallest shapes, with every optional pointer of the record NULL and with every
optional pointer set, against float64.

The kernels behind these entry points read their pointers from records in device memory and carry them as global-typed
pointers (gptr, csrc/common.h); a plain pointer becomes a global one where the record is read.  Two things can go wrong
there and nowhere else: a NULL optional pointer that no longer compares equal to NULL after the conversion (the kernel
then dereferences it), and a member of the record converted to the wrong field.  So every entry point is launched
twice, with the optional pointers of its record all absent and all present, on shapes of one or a few workgroups:

  mpnn_msconv_fwd_group     one member and four members: 4 images of 16x16, 8x8 and 4x4 maps at 16 and 32 channels;
                            optional: operand V (+ its pack), pool_out (maps of 8x8 and up), out_sum, BatchNorm on load
  ... its K-split form      a 4x4 map of 64 channels under batch statistics, alone in its launch; optional: V, out_sum
  mpnn_msconv_bwd_level     one and two members; optional: g_ctx, dgrad-horz (with dy_extra), dgrad-vert (with the finer
                            map's dz and reductions), operand V of the weight gradients
  mpnn_lin_fwd_ks / _bwd    16 rows; optional: the second weight set, k_cpt with its extra column, the K-slice scratch,
                            dx / the fused dz_out + red_out
  mpnn_exit_tail_fwd / _bwd 2 sinks at 16 samples; optional: the head (z, y, c_err, d_cor, dz), bn_save (forward),
                            clear_f / clear_d, hyp_src / hyp_dst

Tolerances are those of the existing tests of each entry point (tests/test_conv_fwd_rep.py, tests/test_bwd_launches.py,
tests/test_exit_kernels.py), whose helpers do the comparing."""
import ctypes as C

import numpy as np
import pytest

from lib import _hip

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- forward conv group
# member: (H, W, Ca, act mode, shift, Cv, Cout, pool, out_nslot) as in tests/test_conv_fwd_rep.py
BARE = {16: (16, 16, 16, 'id', 0, 0, 16, False, None), 8: (8, 8, 32, 'id', 0, 0, 32, False, None),
        4: (4, 4, 16, 'id', 0, 0, 16, False, None), 44: (4, 4, 32, 'id', 0, 0, 32, False, None)}
FULL = {16: (16, 16, 16, 'batch', 0, 16, 32, True, 8), 8: (8, 8, 32, 'batch', 0, 16, 16, True, 8),
        4: (4, 4, 16, 'batch', 0, 16, 32, False, 8), 44: (4, 4, 32, 'batch', 0, 16, 16, False, 5)}
KS_BARE, KS_FULL = (4, 4, 64, 'batch', 0, 0, 16, False, None), (4, 4, 64, 'batch', 0, 64, 32, False, 8)
FWD_ROWS = {'one member, 16x16': [16], 'one member, 8x8': [8], 'one member, 4x4': [4], 'four members': [16, 8, 4, 44]}


def _fwd(mcs, n, ks=False):
    import test_conv_fwd_rep as R
    from test_conv_fwd_lists import Member, launch
    want = ['ks4'] * len(mcs) if ks else [{16: 'g16', 8: 'g8', 4: 'g4'}[mc[0]] for mc in mcs]
    assert R.bodies_of([mc[:8] + (mc[8] or 1,) for mc in mcs], n, 1, 1) == want, 'another body than this row is about'
    ms = [Member(('m%d' % k,) + mc[:8], n, salt=k + 1, out_nslot=mc[8]) for k, mc in enumerate(mcs)]
    got = launch(ms, entry='group')
    for k, (m, mc) in enumerate(zip(ms, mcs)):
        what = 'member %d' % k
        out, pool = got[k]
        assert np.isfinite(out).all(), what + ': out not written everywhere'
        R._check_oracle(m, m.ref(np.arange(n)), out, what)
        if mc[7]:
            R._check_buffers(m, mc[:8] + (mc[8],), got[k], m.sums(), what)
        if mc[8] is not None:
            assert (m.sums()[mc[8]:] == 0).all(), what + ': a slot >= out_nslot of out_sum was written'
            R._check_stats(m, out, m.sums(), what)


@pytest.mark.parametrize('full', [False, True], ids=['optional-null', 'optional-set'])
@pytest.mark.parametrize('row', list(FWD_ROWS))
def test_fwd_group(row, full):
    _fwd([(FULL if full else BARE)[k] for k in FWD_ROWS[row]], 4)


@pytest.mark.parametrize('full', [False, True], ids=['optional-null', 'optional-set'])
def test_fwd_k_split(full):
    _fwd([KS_FULL if full else KS_BARE], 4, ks=True)


# ---------------------------------------------------------------------------------------------- backward level
def _level_specs(full):
    from test_bwd_launches import M, hz, vt
    if not full:                                   # weight gradients only: no g_ctx, no input gradients, no operand V
        return [M(4, 8, 8, 16, a=('bn', 16, 8), split=1), M(4, 4, 4, 32, a=('bn', 16, 8), split=1)]
    return [M(4, 8, 8, 16, gctx=8, horz=hz(16, extra=True, acc=True), vert=vt(16), a=('bn', 16, 8), Cv=16, split=2,
              wg_horz=2, wg_vert=2),
            M(4, 4, 4, 32, gctx=8, horz=hz(16, extra=True), vert=vt(32), a=('bn', 16, 8), Cv=32, split=1)]


@pytest.mark.parametrize('full', [False, True], ids=['optional-null', 'optional-set'])
@pytest.mark.parametrize('count', [1, 2])
def test_bwd_level(count, full):
    import hiputil as U
    from test_bwd_launches import check_oracle
    rng = np.random.default_rng(100 * count + full)
    cases = [U.BwdCase(rng, s) for s in _level_specs(full)[:count]]
    for cs, r in zip(cases, U.run_level(cases)):
        check_oracle(cs, r, worst=None)


# ---------------------------------------------------------------------------------------------- exit path: lin
@pytest.mark.parametrize('full', [False, True], ids=['optional-null', 'optional-set'])
def test_lin_fwd_ks_and_bwd(full):
    import torch
    from hiputil import DEV, bn_dict, dev, stream, unslot
    from test_exit_kernels import bn_relu, close, gclose
    lib = _hip.load()
    rng = np.random.default_rng(5 + full)
    n, C_, HW, M0, M1 = 16, 32, 16, 10, 16
    K = HW * C_                                     # 512: two K-slices where the record carries scratch
    x = rng.standard_normal((n, 4, 4, C_)).astype(np.float32)
    g, be = rng.random(C_).astype(np.float32) + 0.5, (rng.standard_normal(C_) * 0.2).astype(np.float32)
    w0 = (rng.standard_normal((K, M0)) / np.sqrt(K)).astype(np.float32)
    w1 = (rng.standard_normal((K + 1, M1)) / np.sqrt(K)).astype(np.float32)
    b0, b1 = rng.standard_normal(M0).astype(np.float32), rng.standard_normal(M1).astype(np.float32)
    kc = rng.choice([0.0, 1e-9, 6.4e-8], n).astype(np.float32)
    alpha = 1e7
    bn, cnt = bn_dict(x, g, be)
    xd, w0d, w1d, b0d, b1d, kcd = dev(x), dev(w0), dev(w1), dev(b0), dev(b1), dev(kc)
    y0, y1 = torch.full((n, M0), 7.0, device=DEV), torch.full((n, M1), 7.0, device=DEV)
    rg = (n + 15) // 16
    kpart = torch.full((rg * _hip.LIN_KSLICES * 512,), float('nan'), device=DEV)
    kcnt = torch.zeros(rg, dtype=torch.int32, device=DEV)
    lf = _hip.LinFwdArgs()
    lf.a = _hip.act(xd, C_, _hip.ACT_BN_BATCH, 0, bn, cnt) if full else _hip.act(xd, C_, _hip.ACT_IDENTITY, 0)
    lf.HW, lf.n = HW, n
    lf.w[0], lf.b[0], lf.y[0], lf.M[0] = w0d.data_ptr(), b0d.data_ptr(), y0.data_ptr(), M0
    if full:
        lf.w[1], lf.b[1], lf.y[1], lf.M[1] = w1d.data_ptr(), b1d.data_ptr(), y1.data_ptr(), M1
        lf.k_cpt, lf.alpha_cpt, lf.extra_col[1] = kcd.data_ptr(), alpha, 1
        lf.kpart, lf.kcnt = kpart.data_ptr(), kcnt.data_ptr()
    tab = _hip.to_device_table([lf], DEV)
    _hip.check(lib.mpnn_lin_fwd_ks(tab.data_ptr(), 1, n, K, stream()), 'lin_fwd_ks')
    torch.cuda.synchronize()
    a, xh = bn_relu(x, g, be) if full else (x.astype(np.float64), None)
    af = a.reshape(n, K)
    close(y0.cpu().numpy(), af @ w0.astype(np.float64) + b0, 2e-5, 'head logits')
    if full:
        close(y1.cpu().numpy(), af @ w1[:K].astype(np.float64) + b1 + alpha * kc[:, None].astype(np.float64) * w1[K], 2e-5, 'router h1')
        assert int(kcnt.abs().sum()) == 0
    else:
        assert (y1 == 7.0).all(), 'the absent weight set was written'

    dy0, dy1 = rng.standard_normal((n, M0)).astype(np.float32), rng.standard_normal((n, M1)).astype(np.float32)
    dy0d, dy1d = dev(dy0), dev(dy1)
    dw0, dw1 = torch.zeros_like(w0d), torch.full_like(w1d, 7.0)
    db0, db1 = torch.zeros(M0, device=DEV), torch.full((M1,), 7.0, device=DEV)
    dx, dz = torch.full((n, K), 9.0, device=DEV), torch.full((n, K), 9.0, device=DEV)
    red = torch.zeros(_hip.BN_SLOTS * 2 * C_, device=DEV, dtype=torch.float64)
    lb = _hip.LinBwdArgs()
    lb.a, lb.HW, lb.n = lf.a, HW, n
    lb.w[0], lb.dy[0], lb.M[0], lb.dw[0], lb.db[0] = w0d.data_ptr(), dy0d.data_ptr(), M0, dw0.data_ptr(), db0.data_ptr()
    if full:
        lb.w[1], lb.dy[1], lb.M[1], lb.dw[1], lb.db[1] = w1d.data_ptr(), dy1d.data_ptr(), M1, dw1.data_ptr(), db1.data_ptr()
        lb.k_cpt, lb.alpha_cpt, lb.extra_col[1] = kcd.data_ptr(), alpha, 1
        lb.dx, lb.dz_out, lb.red_out, lb.red_nslot = dx.data_ptr(), dz.data_ptr(), red.data_ptr(), _hip.BN_SLOTS
    else:
        lb.dx = dx.data_ptr()
    tb = _hip.to_device_table([lb], DEV)
    _hip.check(lib.mpnn_lin_bwd(tb.data_ptr(), 1, n, K, stream()), 'lin_bwd')
    torch.cuda.synchronize()
    dxr = dy0.astype(np.float64) @ w0.T + (dy1.astype(np.float64) @ w1[:K].T if full else 0.0)
    gclose(dw0.cpu().numpy(), af.T @ dy0, 'dW head')
    gclose(db0.cpu().numpy(), dy0.sum(0, dtype=np.float64), 'db head')
    gclose(dx.cpu().numpy(), dxr, 'dX')
    if full:
        gclose(dw1.cpu().numpy(), np.concatenate([af, alpha * kc[:, None].astype(np.float64)], 1).T @ dy1, 'dW router')
        gclose(db1.cpu().numpy(), dy1.sum(0, dtype=np.float64), 'db router')
        dzr = dxr * (af > 0)
        gclose(dz.cpu().numpy(), dzr, 'dz (masked dX)')
        dz4 = dzr.reshape(n, 4, 4, C_)
        gclose(unslot(red, 2 * C_), np.concatenate([dz4.sum((0, 1, 2)), (dz4 * xh).sum((0, 1, 2))]), 'BN reductions')
    else:
        assert (dw1 == 7.0).all() and (db1 == 7.0).all() and (dz == 9.0).all() and not red.any(), 'an absent output was written'


# ---------------------------------------------------------------------------------------------- exit path: tail
@pytest.mark.parametrize('full', [False, True], ids=['optional-null', 'optional-set'])
def test_exit_tail_fwd_and_bwd(full):
    import torch
    from hiputil import DEV, dev, stream
    from test_exit_kernels import close, gclose, tail_params, tail_ref
    lib = _hip.load()
    n, S, R, nc, MS = 16, 2, 16, 10, 4
    rng = np.random.default_rng(31 + full)
    z = rng.standard_normal((n, nc)).astype(np.float32) * 2
    y = np.eye(nc, dtype=np.float32)[rng.integers(0, nc, n)]
    h1 = rng.standard_normal((n, R)).astype(np.float32)
    P = tail_params(rng, R, S)
    eps_ce, bn_eps, decay, bn_eps2, decay2 = 1e-6, 1e-6, 0.9, 1e-3, 0.99
    d = {k: dev(v) for k, v in P.items()}
    zd, yd, h1d = dev(z), dev(y), dev(h1)
    mv = [dev(rng.standard_normal(R) * 0.1), dev(rng.random(R) + 0.5), dev(rng.standard_normal(R) * 0.1), dev(rng.random(R) + 0.5)]
    c_err, d_cor = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
    h2, r, save = torch.empty((n, R), device=DEV), torch.zeros((n, MS), device=DEV), torch.full((4 * R,), 7.0, device=DEV)
    clear_f, clear_d = torch.full((37,), 3.0, device=DEV), torch.full((5,), 3.0, device=DEV, dtype=torch.float64)
    hyp_src = dev(rng.random(_hip.HYP_N).astype(np.float32))
    hyp_dst = torch.full((_hip.HYP_N,), 7.0, device=DEV)
    tf = _hip.ExitTailArgs()
    tf.n_cls, tf.eps_ce = nc, eps_ce
    tf.h1, tf.R, tf.n_sinks = h1d.data_ptr(), R, S
    tf.g1, tf.b1, tf.m1, tf.v1 = d['g1'].data_ptr(), d['b1'].data_ptr(), mv[0].data_ptr(), mv[1].data_ptr()
    tf.w2, tf.bias2 = d['w2'].data_ptr(), d['bias2'].data_ptr()
    tf.g2, tf.b2, tf.m2, tf.v2 = d['g2'].data_ptr(), d['b2'].data_ptr(), mv[2].data_ptr(), mv[3].data_ptr()
    tf.w3, tf.bias3 = d['w3'].data_ptr(), d['bias3'].data_ptr()
    tf.h2, tf.r, tf.r_stride = h2.data_ptr(), r.data_ptr(), MS
    tf.bn_eps, tf.bn_decay, tf.mode, tf.n = bn_eps, decay, _hip.ACT_BN_BATCH, n
    tf.bn_eps2, tf.bn_decay2 = bn_eps2, decay2
    if full:
        tf.z, tf.y, tf.c_err, tf.d_cor = zd.data_ptr(), yd.data_ptr(), c_err.data_ptr(), d_cor.data_ptr()
        tf.bn_save = save.data_ptr()
        tf.clear_f, tf.n_clear_f, tf.clear_d, tf.n_clear_d = clear_f.data_ptr(), 37, clear_d.data_ptr(), 5
        tf.hyp_src, tf.hyp_dst = hyp_src.data_ptr(), hyp_dst.data_ptr()
    tab = _hip.to_device_table([tf], DEV)
    _hip.check(lib.mpnn_exit_tail_fwd(tab.data_ptr(), 1, n, stream()), 'exit_tail_fwd')
    torch.cuda.synchronize()
    w_cerr = rng.random(n).astype(np.float32) / n
    dr = (rng.standard_normal((n, S)) / n).astype(np.float32)
    ref = tail_ref(z, y, h1, P, eps_ce, bn_eps, w_cerr, dr, S, bn_eps2=bn_eps2)
    close(h2.cpu().numpy(), ref['h2'], 2e-5, 'h2')
    close(r.cpu().numpy()[:, :S], ref['r'], 2e-5, 'r')
    (mm1, vv1), (mm2, vv2) = ref['stats']
    if full:
        close(c_err.cpu().numpy(), ref['c_err'], 2e-5, 'c_err')
        assert np.array_equal(d_cor.cpu().numpy(), ref['d_cor'])
        sv = save.cpu().numpy()
        close(sv[:R], mm1, 2e-5, 'bn1 mean'); close(sv[R:2 * R], 1 / np.sqrt(vv1 + bn_eps), 2e-5, 'bn1 rstd')
        close(sv[2 * R:3 * R], mm2, 2e-5, 'bn2 mean'); close(sv[3 * R:], 1 / np.sqrt(vv2 + bn_eps2), 2e-5, 'bn2 rstd')
        assert not clear_f.any() and not clear_d.any(), 'clear_f / clear_d not cleared'
        assert torch.equal(hyp_dst, hyp_src), 'the schedule values were not copied'
    else:
        assert (c_err == 7.0).all() and (d_cor == 7.0).all() and (save == 7.0).all(), 'an absent output was written'
        assert (clear_f == 3.0).all() and (clear_d == 3.0).all() and (hyp_dst == 7.0).all(), 'an absent output was written'
        # the backward reads bn_save: the statistics of this batch, as the forward with bn_save leaves them
        save.copy_(dev(np.concatenate([mm1, 1 / np.sqrt(vv1 + bn_eps), mm2, 1 / np.sqrt(vv2 + bn_eps2)])))
        tf.bn_save = save.data_ptr()

    drp = np.zeros((n, MS), np.float32); drp[:, :S] = dr
    tb = _hip.ExitTailBwdArgs()
    tb.f = tf
    gr = {k: torch.full(v.shape, 9.0, device=DEV) for k, v in P.items()}
    dz, dh1 = torch.full((n, nc), 9.0, device=DEV), torch.empty((n, R), device=DEV)
    wcd, drd = dev(w_cerr), dev(drp)
    tb.dr, tb.dh1 = drd.data_ptr(), dh1.data_ptr()
    if full:
        tb.w_cerr, tb.dz = wcd.data_ptr(), dz.data_ptr()
    tb.dg1, tb.db1, tb.dw2, tb.dbias2 = gr['g1'].data_ptr(), gr['b1'].data_ptr(), gr['w2'].data_ptr(), gr['bias2'].data_ptr()
    tb.dg2, tb.db2, tb.dw3, tb.dbias3 = gr['g2'].data_ptr(), gr['b2'].data_ptr(), gr['w3'].data_ptr(), gr['bias3'].data_ptr()
    tbb = _hip.to_device_table([tb], DEV)
    _hip.check(lib.mpnn_exit_tail_bwd(tbb.data_ptr(), 1, n, stream()), 'exit_tail_bwd')
    torch.cuda.synchronize()
    if full:
        gclose(dz.cpu().numpy(), ref['dz'], 'dz')
    else:
        assert (dz == 9.0).all(), 'the absent head gradient was written'
    gclose(dh1.cpu().numpy(), ref['dh1'], 'dh1')
    for k in P:
        gclose(gr[k].cpu().numpy(), ref['d' + k], 'd' + k)
