"""Sample lists on the TUNED forward conv group (csrc/conv_fwd.hip: mpnn_msconv_fwd_group with mpnn_conv_fwd_args.idx /
cnt), through the C ABI, on the GPU -- the launch of routed evaluation, alone and at kernel-level shapes.

(tests/test_conv_gen_lists.py does the same for the general kernels; the net tests of tests/test_routed_eval.py reach the
tuned group only at whole-net shapes, where the host sizes everything from a capacity of 200-4 096 and a wrong row can hide.)

One record per case with NaN-poisoned, sentinel-guarded `out` / `pool_out`, launched as a one-member group without a list
and then with lists of 0, 1, 5, n - 1, n and a device count of n + 9 (clamped to the capacity n) over a random
permutation of ALL n images -- entries past the count name real images whose rows must stay poisoned:

  * the rows of the listed images are BIT-equal to the launch without a list at the same capacity (the header's contract:
    the host sizes grid, rows per strip and work shares from n, the device clamps to *cnt; the dense launch walks its
    tiles in the XCD-aware order where n % 32 == 0, a listed launch of a conv_body only where the COUNT % 32 == 0 and a
    listed strip never -- speed only);
  * every other row is still NaN (ghost slots of a four-image 4x4 tile read idx[0] and must be masked on every store
    path: out, pool_out, both M-tiles of the 32-channel tile, the strips' pooled rows); a count of 0 writes nothing;
  * pool_out of the listed rows is the 2x2 max of the launch's own out;
  * one count per case against the float64 conv of oracle/np_ops.py within the limit tests/test_hip_conv.py applies to the
    dense output of the same kernels: 3e-5 (BatchNorm) / 2e-5 (identity, image) x (1 + max |ref|);
  * the count is read on the device; members of a 2-, 3- or 4-member group (own permutation, own count, a count of 0
    beside a full one) get the bits of the member launched alone;
  * refusals (MPNN_E_ARG, nothing written): tests/test_host_cpu.py has them without a GPU, here the outputs stay NaN.

CASES: the smallest shapes that select each body of fwd_group_launch; `body_of` restates the launcher's selection from
the shapes and the capacity and every case asserts the body it is listed for (STRIP_MIN / WIDE_MIN are the thresholds).
Selection as found in the code, where it says more than the list of bodies: W % 16 == 0 and H % 4 == 0 make the 16-wide
geometry (so 4x16, 8x16 and 4x32 maps are '16-wide tile' members below 512 samples); the image + V strip form needs an
IDENTITY (image) operand and V; a lone image -> 16 conv without V at shift 0 would leave for conv_first.hip when it carries
no list -- the SMALL cases have shift 1 / 2, which never does, so dense and listed launches run the same body."""
import ctypes as C

import numpy as np
import pytest

from lib import _hip
from test_conv_gen_lists import _check
from test_conv_hw import _seed

pytestmark = pytest.mark.gpu

STRIP_MIN, WIDE_MIN, STRIP_KMAX = 512, 1024, 3

# (body, H, W, Ca, act mode, shift, Cv, Cout, pool)
G16 = ('g16', 16, 16, 16, 'moving', 0, 16, 16, True)
G8 = ('g8', 8, 8, 32, 'moving', 0, 16, 32, True)
G4 = ('g4', 4, 4, 64, 'moving', 0, 0, 32, False)
G4I = ('g4', 4, 4, 32, 'id', 0, 32, 16, False)
S16 = ('g16+small', 16, 16, 3, 'img', 1, 16, 16, True)
S8 = ('g8+small', 8, 8, 1, 'img', 2, 0, 16, False)
ST1 = ('strip16', 4, 16, 16, 'moving', 0, 0, 16, False)
ST1P = ('strip16', 8, 16, 16, 'moving', 0, 0, 32, True)
STK2 = ('stripk', 8, 16, 16, 'moving', 0, 16, 16, True)             # two 16-channel chunks
STK3 = ('stripk', 4, 32, 32, 'moving', 0, 16, 32, False)            # three
STKI = ('stripk+small', 8, 16, 3, 'img', 1, 16, 16, True)
W4 = ('wide4', 4, 4, 32, 'moving', 0, 0, 32, False)
W8 = ('wide8', 8, 8, 32, 'moving', 0, 32, 64, True)
G8N = ('g8', 8, 8, 32, 'moving', 0, 16, 16, True)                    # (Cout % 32 != 0: keeps its group on 16-channel tiles)

CASES = [(c, 7) for c in (G16, G8, G4, G4I, S16, S8)] + \
        [(c, n) for c in (ST1, ST1P, STK2, STK3, STKI) for n in (512, 517)] + \
        [(c, n) for c in (W4, W8) for n in (1024, 1031)]


def _cid(cn):
    case, n = cn
    return '%s-%dx%d-%d+%d-%d-%s%s-n%d' % (case[0], case[1], case[2], case[3], case[6], case[7], case[4], '-pool' if case[8] else '', n)


def body_of(case, n):
    """fwd_group_launch's choice for one member (csrc/conv_fwd.hip), without the group-level 'wide'."""
    _, H, W, Ca, mode, shift, Cv, Cout, pool = case
    small = Ca <= 4
    big = W >= 16 and W % 16 == 0 and H % 4 == 0
    kch = Ca // 16 + Cv // 16
    if n >= STRIP_MIN and small and Cv and Cv % 16 == 0 and 1 + Cv // 16 <= STRIP_KMAX and big and (not pool or H % 2 == 0):
        return 'stripk+small'
    if n >= STRIP_MIN and big and Ca % 16 == 0 and Ca >= 16 and Cv % 16 == 0 and kch <= STRIP_KMAX and (not pool or H % 2 == 0):
        return 'strip16' if kch == 1 else 'stripk'
    g = 'g16' if big else 'g8' if (H, W) == (8, 8) else 'g4' if (H, W) == (4, 4) else None
    return g + ('+small' if small else '')


def wide_of(cases, n):
    """The 32-channel output tiles: EVERY member an 8x8 / 4x4 conv with Cout % 32 == 0 at a capacity >= 1 024."""
    return all(body_of(c, n) in ('g8', 'g4') and c[7] % 32 == 0 and n >= WIDE_MIN for c in cases)


def expected_body(case, n, group=None):
    b = body_of(case, n)
    if wide_of(group or [case], n):
        b = {'g8': 'wide8', 'g4': 'wide4'}[b]
    return b


class Member:
    """One record of a forward group on n images with NaN-poisoned, guarded outputs and its float64 reference."""

    def __init__(self, case, n, salt=0, out_nslot=None):
        """out_nslot: the member carries out_sum -- a zero-filled, guarded [BN_SLOTS][2 Cout] float64 -- over that many slots."""
        import torch
        import hiputil as U
        from oracle import np_ops as O
        self.case, self.n = case, n
        _, H, W, Ca, mode, shift, Cv, Cout, pool = case
        rng = np.random.default_rng(_seed((case, n, salt)))
        self.H, self.W, self.Cout = H, W, Cout
        self.row, self.prow = H * W * Cout, (H // 2) * (W // 2) * Cout
        self.bn = mode in ('moving', 'batch')
        rec = self.rec = _hip.ConvFwdArgs()
        self.keep = []
        if Ca <= 4:                                            # the pyramid image: ToPyramid's strided pick
            x = rng.random((n, H << shift, W << shift, Ca)).astype(np.float32)
            xd = U.dev(x)
            rec.a = _hip.act(xd, Ca, _hip.ACT_IDENTITY, shift)
            self.a64 = lambda rows: x[rows][:, ::1 << shift, ::1 << shift].astype(np.float64)
            self.keep.append(xd)
        elif mode == 'batch':                                  # batch statistics: BnMap, no ReLU decision within 1e-3 of a tie
            from test_conv_hw import _act
            rec.a, y64, keep = _act(rng, n, H, W, Ca, 'batch', 0)
            self.a64 = lambda rows: y64[rows]                  # (max(bm.y, 0))
            self.keep += keep
        else:
            s = rng.standard_normal((n, H, W, Ca)).astype(np.float32)
            sd = U.dev(s)
            self.keep.append(sd)
            if mode == 'id':
                rec.a = _hip.act(sd, Ca, _hip.ACT_IDENTITY, 0)
                self.a64 = lambda rows: s[rows].astype(np.float64)
            elif mode == 'relu':                               # the Rect after a plain Conv: no coefficients are read
                rec.a = _hip.act(sd, Ca, _hip.ACT_RELU, 0)
                self.a64 = lambda rows: O.relu(s[rows].astype(np.float64))
            else:                                             # BatchNorm with moving averages + ReLU on load
                (g, g64), (b_, b64) = U.f32(rng.uniform(0.5, 1.5, Ca)), U.f32(rng.standard_normal(Ca) * 0.3)
                (m, m64), (v_, v64) = U.f32(rng.standard_normal(Ca) * 0.2), U.f32(rng.uniform(0.5, 2.0, Ca))
                bn, cnt = U.bn_dict(s[:1], g, b_, m, v_)
                rec.a = _hip.act(sd, Ca, _hip.ACT_BN_MOVING, 0, bn, cnt)
                self.a64 = lambda rows: O.relu(O.bn_eval(s[rows].astype(np.float64), g64, b64, m64, v64))
                self.keep.append(bn)
        wh, self.wh64 = U.f32(rng.standard_normal((3, 3, Ca, Cout)) / 3 / np.sqrt(Ca))
        bias, self.b64 = U.f32(rng.standard_normal(Cout) * 0.1)
        ws = [wh]
        self.v = None
        if Cv:
            self.v = rng.standard_normal((n, H, W, Cv)).astype(np.float32)      # the finer map, pooled by its producer
            wv, self.wv64 = U.f32(rng.standard_normal((3, 3, Cv, Cout)) / 3 / np.sqrt(Cv))
            ws.append(wv)
            vd = U.dev(self.v)
            rec.v, rec.Cv = vd.data_ptr(), Cv
            self.keep.append(vd)
        packs, _ = U.pack_weights(ws, want_bwd=False)
        bd = U.dev(bias)
        self.keep += [packs, bd]
        rec.wa_pack, rec.bias = packs[0].data_ptr(), bd.data_ptr()
        if Cv:
            rec.wv_pack = packs[1].data_ptr()
        self.out = U.Guarded(n * self.row)
        self.pool = U.Guarded(n * self.prow) if pool else None
        rec.out = self.out.ptr()
        rec.pool_out = self.pool.ptr() if pool else None
        rec.n, rec.H, rec.W, rec.Cout = n, H, W, Cout
        self.osum = None
        if out_nslot is not None:
            self.osum = U.Guarded(_hip.BN_SLOTS * 2 * Cout, torch.float64)
            rec.out_sum, rec.out_nslot = self.osum.ptr(), out_nslot

    def set_list(self, idx, cnt):
        """idx, cnt: device int32 tensors (or None); kept alive here -- the record holds bare pointers."""
        self.list = (idx, cnt)
        self.rec.idx = idx.data_ptr() if idx is not None else None
        self.rec.cnt = cnt.data_ptr() if cnt is not None else None

    def poison(self):
        self.out.fill(float('nan'))
        if self.pool is not None:
            self.pool.fill(float('nan'))
        if self.osum is not None:
            self.osum.fill(0.0)

    def rows(self):
        assert self.out.guards_ok() and (self.pool is None or self.pool.guards_ok()), 'a guard was overwritten'
        assert self.osum is None or self.osum.guards_ok(), 'a guard of out_sum was overwritten'
        return (self.out.get().reshape(self.n, self.row),
                self.pool.get().reshape(self.n, self.prow) if self.pool is not None else None)

    def sums(self):
        """out_sum as [BN_SLOTS][2 Cout] float64."""
        return self.osum.get().reshape(_hip.BN_SLOTS, 2 * self.Cout)

    def ref(self, rows):
        """float64: bias + conv(act(a)) [+ conv(v)] of the images `rows` (tests/test_hip_conv.py: ref_fwd)."""
        from oracle import np_ops as O
        out = self.b64 + O.conv_same(self.a64(rows), self.wh64)
        if self.v is not None:
            out = out + O.conv_same(self.v[rows].astype(np.float64), self.wv64)
        return out


def launch(members, expect=0, entry='group', reps=1, share=1):
    """Poison every member's outputs, launch them as ONE group (host array + device table), return their rows.
    entry 'rep': mpnn_msconv_fwd_group_rep with `reps` / `share`; `members` may then be a list of NETS (each a list of
    members): host array and device table hold reps * count records in net order, and the rows come back per net."""
    import torch
    import hiputil as U
    lib = _hip.load()
    nets = members if members and isinstance(members[0], (list, tuple)) else None
    if nets is not None:
        members = [m for net in nets for m in net]
    for m in members:
        m.poison()
    recs = [m.rec for m in members]
    arr = (_hip.ConvFwdArgs * len(recs))(*recs)
    tab = _hip.to_device_table(recs, U.DEV)
    if entry == 'group':
        rc = lib.mpnn_msconv_fwd_group(arr, tab.data_ptr(), len(recs), U.stream())
    elif entry == 'rep':
        rc = lib.mpnn_msconv_fwd_group_rep(arr, tab.data_ptr(), len(recs) // reps, reps, share, U.stream())
    else:
        rc = lib.mpnn_msconv_fwd(C.byref(recs[0]), U.stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    rows = [m.rows() for m in members]
    if nets is None:
        return rows
    return [rows[r * len(nets[0]):(r + 1) * len(nets[0])] for r in range(len(nets))]


def _dev_list(perm, count):
    import torch
    import hiputil as U
    return U.dev(np.asarray(perm, np.int32), torch.int32), torch.full((1,), count, dtype=torch.int32, device=U.DEV)


def _all_nan(got):
    return all(np.isnan(g).all() for g in got if g is not None)


@pytest.mark.parametrize('cn', CASES, ids=list(map(_cid, CASES)))
def test_listed_rows_equal_the_dense_launch_and_the_rest_is_untouched(cn):
    import hiputil as U
    case, n = cn
    assert expected_body(case, n) == case[0], 'the launcher selects another body for this case than it is listed for'
    m = Member(case, n)
    dense, = launch([m])
    assert np.isfinite(dense[0]).all() and (dense[1] is None or np.isfinite(dense[1]).all())
    if dense[1] is not None:
        assert np.array_equal(dense[1], U.pool2_np(dense[0].reshape(n, m.H, m.W, m.Cout)).reshape(n, -1))
    rng = np.random.default_rng(_seed(cn) + 1)
    for c in (0, 1, 5, n - 1, n, n + 9):
        perm = rng.permutation(n)
        m.set_list(*_dev_list(perm, c))
        listed = perm[:min(c, n)]
        got, = launch([m])
        what = 'count %d' % c
        _check(got, dense, listed, n, what)
        if c == 0:
            assert _all_nan(got)
        else:                                                  # idx[0]: the image every ghost slot reads
            assert np.array_equal(got[0][perm[0]], dense[0][perm[0]]), what
        if c >= n:                                             # a permutation of every image: the dense launch everywhere
            assert np.array_equal(got[0], dense[0]) and (got[1] is None or np.array_equal(got[1], dense[1])), what
        if got[1] is not None and len(listed):
            mine = U.pool2_np(got[0][listed].reshape(len(listed), m.H, m.W, m.Cout))
            assert np.array_equal(got[1][listed], mine.reshape(len(listed), -1)), what + ': pool_out is not the 2x2 max of out'
        if c == 5:                                             # the float64 anchor
            from oracle import np_ops as O
            ref = m.ref(listed)
            tol = 3e-5 if m.bn else 2e-5
            lim = tol * (1.0 + np.abs(ref).max())
            err = np.abs(got[0][listed].reshape(ref.shape) - ref).max()
            print('%s: out  worst error / limit = %.3f' % (_cid(cn), err / lim))
            worst = err / lim
            if got[1] is not None:
                perr = np.abs(got[1][listed].reshape(5, m.H // 2, m.W // 2, m.Cout) - O.pool2(ref)).max()
                print('%s: pool worst error / limit = %.3f' % (_cid(cn), perr / lim))
                worst = max(worst, perr / lim)
            assert worst <= 1.0, worst


@pytest.mark.parametrize('cn', [(G8, 7), (STK2, 517), (W8, 1031)], ids=_cid)
def test_the_count_is_read_on_the_device(cn):
    """The same record, launched three times; only the device count tensor changes in between."""
    case, n = cn
    m = Member(case, n)
    dense, = launch([m])
    perm = np.random.default_rng(_seed(cn) + 2).permutation(n)
    idx, cnt = _dev_list(perm, 5)
    m.set_list(idx, cnt)
    _check(launch([m])[0], dense, perm[:5], n, 'count 5')
    cnt.fill_(2)
    _check(launch([m])[0], dense, perm[:2], n, 'count 2 (the record unchanged)')
    cnt.fill_(n - 1)
    _check(launch([m])[0], dense, perm[:n - 1], n, 'count n - 1 (the record unchanged)')
    cnt.fill_(0)
    assert _all_nan(launch([m])[0]), 'count 0 (the record unchanged)'


# (members, capacity, counts: None = n)
GROUPS = [
    ('small+g16', [S16, G16], 7, [3, None]),
    ('g16+g8+g4+g4', [G16, G8, G4, G4I], 7, [None, 0, 5, 6]),
    ('strip16+g8+g4', [ST1P, G8, G4], 517, [200, None, 0]),
    ('stripk+stripk_img+strip16+g8', [STK2, STKI, ST1, G8N], 517, [0, 516, None, 33]),
    ('wide4+wide8', [W4, W8], 1031, [1029, 64]),
    ('g8(wide alone)+g8', [W8, G8N], 1031, [None, 0]),
]


@pytest.mark.parametrize('grp', GROUPS, ids=[g[0] for g in GROUPS])
def test_members_of_a_group_equal_the_member_alone(grp):
    """2-, 3- and 4-member launches of mixed bodies: every member has its own permutation and its own count, and its rows
    are bit-equal to the same member launched alone with the same list (and, listed rows, without one)."""
    _, cases, n, counts = grp
    for c in cases:                                            # (beside a member that is not wide, W8 runs the 16-channel tile)
        want = c[0] if wide_of(cases, n) else {'wide8': 'g8', 'wide4': 'g4'}.get(c[0], c[0])
        assert expected_body(c, n, cases) == want and (not c[0].startswith('wide') or wide_of([c], n))
    ms =[Member(c, n, salt=k) for k, c in enumerate(cases)]
    rng = np.random.default_rng(_seed((grp[0], n)))
    lists = []
    for m, c in zip(ms, counts):
        perm = rng.permutation(n)
        lists.append((perm, n if c is None else c, _dev_list(perm, n if c is None else c)))
        m.set_list(*lists[-1][2])
    together = launch(ms)
    for m, got, (perm, c, _) in zip(ms, together, lists):
        alone, = launch([m])
        m.set_list(None, None)
        dense, = launch([m])
        what = '%s of %s, count %d' % (m.case[0], grp[0], c)
        _check(got, dense, perm[:c], n, what)
        for a, b in zip(got, alone):                           # NaN rows included: the same bytes
            assert a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)), what + ': differs from the member alone'


def test_refusals_leave_the_outputs_alone():
    """One of idx / cnt alone, a group where only some members carry a list, a list on mpnn_msconv_fwd or
    mpnn_msconv_fwd_group_rep, a list with out_sum, a list under batch statistics: MPNN_E_ARG, nothing written."""
    import torch
    import hiputil as U
    E_ARG, n = _hip.E_ARG, 7
    idx, cnt = _dev_list(np.arange(n), 3)
    a, b = Member(G8, n), Member(G4, n, salt=1)
    dense, = launch([a])
    for only in ((idx, None), (None, cnt)):
        a.set_list(*only)
        assert _all_nan(launch([a], expect=E_ARG)[0])
    for first, second in ((a, b), (b, a)):                    # only one member of two with a list
        first.set_list(idx, cnt); second.set_list(None, None)
        assert all(_all_nan(g) for g in launch([first, second], expect=E_ARG))
    a.set_list(idx, cnt); b.set_list(None, None)
    assert _all_nan(launch([a], expect=E_ARG, entry='fwd')[0])
    assert _all_nan(launch([a], expect=E_ARG, entry='rep')[0])
    osum = torch.zeros(_hip.BN_SLOTS * 2 * a.Cout, dtype=torch.float64, device=U.DEV)
    a.rec.out_sum, a.rec.out_nslot = osum.data_ptr(), 4
    assert _all_nan(launch([a], expect=E_ARG)[0]) and not osum.any()
    a.rec.out_sum = None
    _check(launch([a])[0], dense, np.arange(3), n, 'the record without out_sum')
    bt = Member(('g8', 8, 8, 32, 'batch', 0, 16, 32, True), n)
    assert np.isfinite(launch([bt])[0][0]).all()
    bt.set_list(idx, cnt)
    assert _all_nan(launch([bt], expect=E_ARG)[0])
