"""GPU parity: the fused backward launches -- mpnn_msconv_bwd_level (and its co-training form _rep),
mpnn_msconv_bwd_scale and mpnn_msconv_dgrad_pair -- through the C ABI against a float64 restatement
(oracle/np_ops.py), member by member.

Every member gets random fp32 inputs (cast exactly to float64 for the oracle).  The pre-BN map of every
BatchNorm context is drawn so that no fp64 BatchNorm output lies within 1e-3 of zero: ReLU masks are then the
same on both sides, and the fp64 reductions are held to 1e-5 of the sum of the absolute values of their terms.
Outputs sit between sentinel guard regions, which must come back unchanged; outputs that are plain stores are
pre-filled with NaN, so every element must be written.  Tolerances as in test_hip_conv.py:
  dgrad (out, dz_g_fine) : max|err| <= 2e-5 (3e-5 with a BatchNorm applied to g or dz) * (1 + max|ref|)
  wgrad (dW, db)         : max|err| <= 1e-4 * (1 + max|ref|)
  red_out (fp64)         : |err| <= 1e-5 * sum|term| per channel

Cross-launch identities.  One workgroup computes each dgrad output tile whole, in a fixed contraction order, so
`out` and `dz_g_fine` are bit-identical whatever the budgets, the other members of the level, or the entry point.
The weight gradients of one split are sums over that split's tiles: bit-identical whenever the split and the
tile order (bwd_bodies.h: XCD-aware when n % 32 == 0, the split % 8 == 0 and the launch is not a _rep form) are
the same, and the same body runs -- a block-0 member (1- or 3-channel image) runs the swapped-role SMALLC body by
itself but the general body in a level that also holds a 64-channel member, so there it is held to fp32
rounding.  red_out: every workgroup sums its own tiles' terms in fp32 and adds them to the slots with fp64 atomics,
so launches with the same workgroup partition (equal budgets) agree to 1e-12 relative, and launches with different
budgets or entry points to the oracle's bound (1e-5 * sum|term|), not bit for bit.
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from lib import _hip

S = _hip.BN_SLOTS


def M(n, H, W, Cg, **kw):
    return dict(n=n, H=H, W=W, Cg=Cg, **kw)


def hz(Cp, extra=False, acc=False, nslot=8):
    return dict(Cp=Cp, extra=extra, acc=acc, nslot=nslot)


def vt(Cf, has_dz=True, nslot=8):
    return dict(Cf=Cf, has_dz=has_dz, nslot=nslot)


# level sets: GKMASK 1..7, OTMASK 1..3, members with horz / vert / both / neither, red_nslot 1 / 8 / BN_SLOTS,
# budgets 0 (clamped to 1), 1, odd, == tiles and > tiles, splits 1 / 3 / 8k / tiles, ragged batches
LEVELS = {
    # GKMASK 1 (32x32), OTMASK 1: both input gradients, g_ctx, accumulate
    'g1_32x32_both': [M(2, 32, 32, 16, gctx=S, horz=hz(16, extra=True, acc=True, nslot=S), vert=vt(16, nslot=S),
                        a=('bn', 16, S), Cv=16, split=3, wg_horz=3, wg_vert=5)],
    # GKMASK 2 (8x8, ragged n = 11), OTMASK 1: horz only (budget == tiles) + vert only (finer map without dz)
    'g2_8x8_ragged': [M(11, 8, 8, 32, horz=hz(32, nslot=1), a=('bn', 32, 8), split=8, wg_horz=11),
                      M(11, 8, 8, 16, gctx=1, vert=vt(16, has_dz=False, nslot=1), a=('bn', 16, 1), Cv=16, split=1,
                        wg_vert=0)],
    # GKMASK 4 (4x4, ragged n = 5), OTMASK 2: 64 / 128 channels, both + wgrad only, split = tiles
    'g4_4x4_wide': [M(5, 4, 4, 64, gctx=8, horz=hz(32, acc=True), vert=vt(64), a=('bn', 32, 8), Cv=64, split=2,
                      wg_horz=9, wg_vert=1),
                    M(5, 4, 4, 128, a=('bn', 64, S), split=1)],
    # GKMASK 3 (16x16 + 8x8), OTMASK 3
    'g3_16x16_8x8_mixed': [M(4, 16, 16, 16, gctx=8, horz=hz(16, acc=True, nslot=S), a=('bn', 16, 8), split=16,
                             wg_horz=7),
                           M(4, 8, 8, 64, horz=hz(32, extra=True), vert=vt(32, nslot=1), a=('bn', 32, 8), Cv=32,
                             split=3, wg_horz=4, wg_vert=3)],
    # GKMASK 5 (12x16 non-square + 4x4 ragged), OTMASK 1
    'g5_12x16_4x4': [M(2, 12, 16, 32, vert=vt(16, nslot=S), a=('bn', 16, 8), Cv=16, split=3, wg_vert=5),
                     M(5, 4, 4, 16, gctx=8, horz=hz(16, extra=True), a=('bn', 16, 8), split=2, wg_horz=100)],
    # GKMASK 6 (8x8 + 4x4), three members, OTMASK 3
    'g6_8x8_4x4_three': [M(5, 8, 8, 128, gctx=8, a=('bn', 128, 8), split=5),
                         M(11, 4, 4, 16, horz=hz(16, acc=True, nslot=1), vert=vt(16), a=('bn', 16, 8), Cv=16,
                           split=3, wg_horz=3, wg_vert=2),
                         M(11, 4, 4, 32, horz=hz(64, nslot=S), a=('bn', 64, S), split=1, wg_horz=1)],
    # GKMASK 7: four members; the 16x16 one at n = 32 with a split of 8 takes the XCD-aware tile order
    'g7_four': [M(32, 16, 16, 16, horz=hz(16), vert=vt(16), a=('bn', 16, 8), Cv=16, split=8, wg_horz=9, wg_vert=16),
                M(4, 8, 8, 32, gctx=S, vert=vt(32, has_dz=False, nslot=S), a=('bn', 32, S), Cv=32, split=4, wg_vert=3),
                M(5, 4, 4, 64, horz=hz(32), a=('bn', 32, 8), split=2, wg_horz=2),
                M(2, 16, 48, 32, gctx=8, a=('bn', 16, 8), split=1)],
    # SMALLC: block-0 members (pyramid image operand A) in the SMALLC variants
    'smallc_img3_noV': [M(2, 32, 32, 16, a=('img', 3, 0), split=3),
                        M(5, 8, 8, 16, horz=hz(16), vert=vt(16), a=('bn', 16, 8), Cv=16, split=2, wg_horz=2,
                          wg_vert=3)],
    'smallc_img1_V': [M(2, 16, 16, 16, gctx=8, vert=vt(16), a=('img', 1, 1), Cv=16, split=7, wg_vert=3),
                      M(5, 4, 4, 16, horz=hz(16), a=('bn', 16, 8), split=1, wg_horz=2)],
    'smallc_img3_V_alone': [M(5, 4, 4, 16, gctx=8, vert=vt(16), a=('img', 3, 3), Cv=16, split=2, wg_vert=1)],
    # the same kind of members beside a 64-channel member: the general weight-gradient body (never built by a shipped net)
    'smallc_img3_V_with_wide': [M(3, 8, 8, 16, gctx=8, vert=vt(16), a=('img', 3, 2), Cv=16, split=3, wg_vert=2),
                                M(5, 4, 4, 64, horz=hz(32), a=('bn', 32, 8), split=2, wg_horz=3)],
    'smallc_img1_noV_with_wide': [M(2, 32, 32, 16, a=('img', 1, 0), split=8),
                                  M(4, 8, 8, 64, vert=vt(64), a=('bn', 64, 8), Cv=64, split=2, wg_vert=2)],
}


def close(got, ref, tol, what):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), (what, 'not every element written')
    err = np.abs(got - ref).max()
    assert err <= tol * (1.0 + np.abs(ref).max()), (what, err, np.abs(ref).max())
    return err / (1.0 + np.abs(ref).max())


WORST = {}          # worst relative error per output type over the module (MPNN_BWD_WORST=path: written there as JSON)


def check_oracle(cs, r, worst=WORST):
    """Every output of one member against its float64 reference (and the guards)."""
    assert cs.guards_ok(), 'a write outside the outputs'
    wide_g = 3e-5 if cs.g_ctx is not None else 2e-5
    errs = {}
    if cs.h is not None:
        Cp = cs.spec['horz']['Cp']
        errs['out'] = close(r['out'].reshape(cs.out_ref.shape), cs.out_ref, wide_g, 'out')
        red = r['red'].sum(0)
        bad = np.abs(red - cs.red_ref) > 1e-5 * cs.red_abs + 1e-300
        assert not bad.any(), ('red_out', np.flatnonzero(bad)[:8], Cp)
        errs['red_out'] = float((np.abs(red - cs.red_ref) / np.maximum(cs.red_abs, 1e-300)).max())
    if cs.v is not None:
        errs['dz_g_fine'] = close(r['dzg'].reshape(cs.dzg_ref.shape), cs.dzg_ref, 3e-5, 'dz_g_fine')
    if cs.w is not None:                                  # (a member built with wgrad=False has none)
        errs['dWa'] = close(r['dwa'], cs.dwa_ref.reshape(-1), 1e-4, 'dWa')
        if cs.dwv_ref is not None:
            errs['dWv'] = close(r['dwv'], cs.dwv_ref.reshape(-1), 1e-4, 'dWv')
        errs['db'] = close(r['db'], cs.db_ref, 1e-4, 'db')
    if worst is not None:
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if os.environ.get('MPNN_BWD_WORST'):
            import json
            with open(os.environ['MPNN_BWD_WORST'], 'w') as f:
                json.dump(worst, f, indent=1)
    return errs


def same_dgrad(a, b, what, red_abs=None):
    """red_abs None: the same workgroup partition on both sides (only the order of the fp64 atomics differs): 1e-12
    relative.  Otherwise a different partition: each workgroup's partial sums are fp32 (conv_kernel.h epilogue), so
    the two agree to 1e-5 * sum|term| per channel, as each agrees with the oracle."""
    for k in ('out', 'dzg'):
        if k in a:
            assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max())
    if 'red' in a:
        ra, rb = a['red'].sum(0), b['red'].sum(0)
        tol = 1e-12 * np.abs(ra).max() + 1e-12 * np.abs(ra) if red_abs is None else 1e-5 * red_abs
        assert (np.abs(ra - rb) <= tol).all(), (what, 'red_out', np.abs(ra - rb).max())


def same_wgrad(a, b, what, exact=True):
    for k in ('dwa', 'dwv', 'db'):
        if not a[k].size:
            continue
        if exact:
            assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max())
        else:                     # another summation order: both are within the oracle's tolerance, and of each other
            assert np.abs(a[k] - b[k]).max() <= 1e-4 * (1 + np.abs(b[k]).max()), (what, k)


def smallc_fallback(cases, cs):
    """The member's weight gradients run a different body in this level than alone (see the module docstring)."""
    return cs.spec['a'][0] == 'img' and cs.Cg % 64 and any(c.Cg % 64 == 0 for c in cases)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(LEVELS))
def test_level_vs_oracle(name):
    """One level launch against the oracle; each member run alone (a one-member level with the same budgets)
    gives bit-identical input gradients and, with the same body, bit-identical weight gradients."""
    import hiputil as U
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cases = [U.BwdCase(rng, s) for s in LEVELS[name]]
    res = U.run_level(cases)
    for cs, r in zip(cases, res):
        check_oracle(cs, r)
    if len(cases) > 1:
        for cs, r in zip(cases, res):
            alone = U.run_level([cs])[0]
            assert cs.guards_ok()
            same_dgrad(alone, r, 'alone vs in the level')
            same_wgrad(alone, r, 'alone vs in the level', exact=not smallc_fallback(cases, cs))


BUDGET_CASES = {
    '16x16': M(4, 16, 16, 16, gctx=8, horz=hz(16, extra=True), vert=vt(16), a=('bn', 16, 8), Cv=16, split=3),
    '12x16_acc': M(3, 12, 16, 32, horz=hz(16, acc=True, nslot=S), vert=vt(32, has_dz=False, nslot=1),
                   a=('bn', 16, 8), Cv=32, split=1),
    '8x8_wide': M(5, 8, 8, 64, gctx=S, horz=hz(32, nslot=1), vert=vt(64, nslot=S), a=('bn', 32, 8), Cv=64, split=5),
    '4x4_ragged': M(11, 4, 4, 32, horz=hz(16), vert=vt(16), a=('bn', 16, 8), Cv=16, split=3),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(BUDGET_CASES))
def test_budgets_and_entry_points_bit_identical(name):
    """wg_horz / wg_vert = 0 (clamped to 1), 1, odd, == tiles, > tiles (clamped): identical input gradients and
    weight gradients; the same member through mpnn_msconv_bwd_scale (its own budgets, the same split and tile
    order) and mpnn_msconv_dgrad_pair: identical again."""
    import hiputil as U
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cs = U.BwdCase(rng, BUDGET_CASES[name])
    t = cs.tiles
    runs = []
    for b in [(1, 1), (0, 0), (3, 5), (t, t), (t + 1, 4 * t + 3)]:
        r = U.run_level([cs], budgets=[b])[0]
        check_oracle(cs, r)
        runs.append((b, r))
    for b, r in runs[1:]:
        same_dgrad(runs[0][1], r, 'budget %s' % (b,), cs.red_abs)
        same_wgrad(runs[0][1], r, 'budget %s' % (b,))
    r = U.run_scale(cs)
    check_oracle(cs, r)
    same_dgrad(runs[0][1], r, 'bwd_scale', cs.red_abs)
    same_wgrad(runs[0][1], r, 'bwd_scale')
    r = U.run_pair(cs)
    assert cs.guards_ok()
    same_dgrad(runs[0][1], r, 'dgrad_pair', cs.red_abs)


@pytest.mark.gpu
@pytest.mark.parametrize('n,split', [(5, 2), (32, 8)])
def test_rep_form(n, split):
    """reps = 3 nets of one shape, each with its own buffers: every net's outputs are bit-identical to a reps = 1
    _rep launch on that net's buffers.  Against the level form: identical input gradients; the weight gradients
    are identical unless the level form takes the XCD-aware tile order (n % 32 == 0, split % 8 == 0), which the
    _rep form never does -- then they agree to fp32 rounding."""
    import hiputil as U
    rng = np.random.default_rng(n * 100 + split)
    specs = [M(n, 8, 8, 16, gctx=8, horz=hz(16, acc=True), vert=vt(16), a=('bn', 16, 8), Cv=16, split=split,
               wg_horz=3, wg_vert=2),
             M(n, 4, 4, 64, horz=hz(32), a=('bn', 32, 8), split=split, wg_horz=2)]
    nets = [[U.BwdCase(rng, s) for s in specs] for _ in range(3)]
    joint = U.run_level_rep([cs for net in nets for cs in net], 3)
    for k, net in enumerate(nets):
        single = U.run_level_rep(net, 1)
        for j, (cs, r1) in enumerate(zip(net, single)):
            check_oracle(cs, r1)
            same_dgrad(joint[k * 2 + j], r1, 'reps 3 vs 1')
            same_wgrad(joint[k * 2 + j], r1, 'reps 3 vs 1')
    level = U.run_level(nets[0])
    xcd = n % 32 == 0 and split % 8 == 0
    for cs, r1, rl in zip(nets[0], U.run_level_rep(nets[0], 1), level):
        check_oracle(cs, rl)
        same_dgrad(rl, r1, 'level vs _rep')
        same_wgrad(rl, r1, 'level vs _rep', exact=not xcd)


def production_specs(net, n):
    """(level sets with their budgets) exactly as Engine._bwd_schedule returns them for `net` at batch n."""
    eng = net.engine()
    order = [(kb, b, i) for kb, b in enumerate(reversed(eng.blocks)) for i in range(b.L - 1, -1, -1)]
    levels = []
    for grp in eng._bwd_schedule(order, n):
        if grp[0][1] is None:
            continue                                  # a plain mpnn_msconv_bwd_scale launch (not a level)
        specs = []
        for (kb, b, i), bud in grp:
            L1 = b.L - 1
            sp = M(n, b.H[i], b.W[i], b.C[i], gctx=eng._nslot(b, L1) if i == L1 else None, split=bud['split'],
                   wg_horz=bud['gxh'], wg_vert=bud['gxv'], Cv=b.C[i - 1] if i > 0 else 0)
            if b.parent is not None:
                pb, j = b.parent, b.in_map[i]
                sp['horz'] = hz(pb.C[j], extra=bool(pb.has_exit and j == pb.L - 1), nslot=eng._nslot(pb, j))
                sp['a'] = ('bn', b.Cin[i], eng._nslot(pb, j))
            else:
                sp['a'] = ('img', eng.x0_shape[2], b.in_shift[i])
            if i > 0:
                sp['vert'] = vt(b.C[i - 1], has_dz=bool(b.has_dz[i - 1]), nslot=eng._nslot(b, i - 1))
            specs.append(sp)
        levels.append(specs)
    return levels


@pytest.mark.gpu
@pytest.mark.parametrize('arch', ['ac_chain', 'sr_chain'])
def test_production_levels(arch):
    """The level sets and budgets the planner emits for the shipped chains at n = 128, with random data."""
    import arch_and_hypers as A
    import hiputil as U
    mk = {'ac_chain': lambda: A.ac_chain(k_cpt=1.6e-8), 'sr_chain': lambda: A.sr_chain(8)}[arch]
    levels = production_specs(mk()((32, 32, 3), (10,)), 128)
    assert levels, 'the planner emitted no level launch'
    rng = np.random.default_rng(5)
    for specs in levels:
        cases = [U.BwdCase(rng, s) for s in specs]
        for cs, r in zip(cases, U.run_level(cases)):
            check_oracle(cs, r)
        del cases


def test_argument_errors():
    """The documented error returns of the level launchers (host-side checks: no device needed, nothing launches).
    Pointers are placeholders that the host code only tests for NULL."""
    from lib import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load()
    P = 0x1000                                           # never dereferenced: nothing here reaches a launch
    keep = []

    def act(C_):
        return _hip.act(None, C_, _hip.ACT_IDENTITY, 0)

    def member(H=8, W=8, Cg=16, Ca=16, horz=True, prev=True, hCg=None, n=4):
        ctx = _hip.BnCtx()
        ctx.s, ctx.red_nslot = P, 8
        ctx.bn = _hip.act(None, 16, _hip.ACT_BN_BATCH, 0)
        w = _hip.WgradArgs()
        w.a = act(Ca)
        w.a.x = P
        w.g, w.dwa, w.db = P, P, P
        w.n, w.H, w.W, w.Cout, w.n_split = n, H, W, Cg, 1
        m = _hip.BwdMember()
        m.wgrad = C.pointer(w)
        m.wg_horz = m.wg_vert = 1
        keep.extend([ctx, w])
        if horz:
            h = _hip.DgradHorzArgs()
            h.g, h.Cg, h.w_pack, h.out, h.red_out = P, Cg if hCg is None else hCg, P, P, P
            h.prev = C.pointer(ctx) if prev else None
            h.n, h.H, h.W, h.Cout = n, H, W, 16
            m.horz = C.pointer(h)
            keep.append(h)
        return m

    size = lib.mpnn_msconv_bwd_level_record_size()
    host = (C.c_char * (size * 2 * _hip.BWD_LEVEL_MAX * 3))()

    def prep(ms, count=None):
        arr = (_hip.BwdMember * max(1, len(ms)))(*ms)
        return lib.mpnn_msconv_bwd_level_prepare(arr, len(ms) if count is None else count, host)

    def prep_rep(ms, reps):
        arr = (_hip.BwdMember * len(ms))(*ms)
        return lib.mpnn_msconv_bwd_level_prepare_rep(arr, len(ms) // reps, reps, host)

    assert prep([member()]) == 0 and prep_rep([member(), member()], 2) == 0          # (the baseline is valid)
    # MPNN_E_ARG
    assert prep([member()], count=0) == _hip.E_ARG
    assert prep([member() for _ in range(5)]) == _hip.E_ARG
    assert prep([member(prev=False)]) == _hip.E_ARG                                 # horz without prev
    assert prep([member(hCg=18)]) == _hip.E_ARG                                     # Cg & 3
    assert prep([member(n=0)]) == _hip.E_ARG
    assert prep_rep([member(Cg=16), member(Cg=32)], 2) == _hip.E_ARG                # shapes differ between nets
    assert prep_rep([member(H=8, W=8), member(H=4, W=4)], 2) == _hip.E_ARG
    arr = (_hip.BwdMember * 1)(member())
    assert lib.mpnn_msconv_bwd_level_prepare(arr, 1, None) == _hip.E_ARG          # NULL record pointers
    assert lib.mpnn_msconv_bwd_level_prepare_rep(arr, 1, 1, None) == _hip.E_ARG
    assert lib.mpnn_msconv_bwd_level(arr, 1, None, None) == _hip.E_ARG
    assert lib.mpnn_msconv_bwd_level_rep(arr, 1, 1, None, None) == _hip.E_ARG
    assert lib.mpnn_msconv_bwd_level_prepare(None, 1, host) == _hip.E_ARG
    # MPNN_E_SHAPE
    assert prep([member(H=5, W=5, horz=False)]) == _hip.E_SHAPE                    # 5x5 map
    assert prep([member(Cg=24, horz=False)]) == _hip.E_SHAPE                       # Cout % 16
    assert prep([member(Ca=6, horz=False)]) == _hip.E_SHAPE                        # operand A: > 4 channels, not 4k
    assert prep([member(), member(H=5, W=5, horz=False)]) == _hip.E_SHAPE
