"""CPU: the builders, references and limits of tests/small_launch_ref.py, which the GPU tests of the BatchNorm launches
(tests/test_bn_launches.py) and of the 1x1 conv kernels (tests/test_conv1x1_kernels.py) rely on.

Every table case builds; the redraw leaves no element of a ReLU-feeding map inside the margin, in every mode, and the
only exact zeros are the planted ones (+0 and -0 both present); a float32 numpy evaluation of each operation stays below
HALF of the limit the GPU test applies, so the limits are not set by the kernels; the kernel-selection table restates
the two predicates of csrc/misc.hip; and hiputil.BnMap, which this work leaves alone, still draws what it drew.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_launch_ref as R

worst = lambda got, ref, limit: float((np.abs(np.asarray(got, np.float64) - ref) / limit).max())


def check_margin(a):
    if a.mode == 'id':
        return
    near = np.abs(a.pre) < R.MARGIN
    assert np.array_equal(near, a.planted), 'elements inside the margin'
    assert (a.pre[a.planted] == 0).all() and not a.on[a.planted].any()
    if a.mode == 'relu':
        z = a.s[a.planted]
        assert z.size >= 1 and (z == 0).all()
        if z.size > 1:
            assert np.signbit(z).any() and not np.signbit(z).all()                 # +0 and -0
        assert abs(z.size - 0.01 * a.s.size) <= 3 + 0.01 * a.s.size                # about 1 %
    else:
        assert not a.planted.any()


def check_slots(a):
    if a.mode != 'batch':
        assert a.sums is None
        return
    assert a.sums.shape == (R.SLOTS, 2 * a.C) and np.isnan(a.sums[a.nslot:]).all() and np.isfinite(a.sums[:a.nslot]).all()
    tot = np.concatenate([a.s64.sum(0), (a.s64 ** 2).sum(0)])
    assert np.allclose(a.sums[:a.nslot].sum(0), tot, rtol=1e-12, atol=1e-12)
    if a.nslot > 1:
        assert np.abs(a.sums[0] - a.sums[1]).max() > 0                             # spread unevenly


def test_kernel_selection_table_matches_the_predicates():
    assert set(R.BN_C) | set(R.BN_C_MODES) | {c[0] for c in R.CONTRACT_CASES} <= set(R.KERNELS)
    for C, want in R.KERNELS.items():
        assert R.selected(C) == want, C
        # bn_shape_ok of csrc/misc.hip, and the branch mpnn_bn_relu_fwd takes, written out again
        q_bwd = C % 4 == 0 and 256 % (C // 4) == 0 and C <= 256
        q_fwd = C % 4 == 0 and C <= 256
        assert (want[1] == 'quad') == q_bwd and (want[0] == 'quad') == q_fwd
        assert (want[0] == 'any4') == (not q_fwd and C % 4 == 0) and (want[1] == 'any4') == (not q_bwd and C % 4 == 0)
    assert R.KERNELS[12] == R.KERNELS[48] == ('quad', 'any4')                      # where the two rules part
    for launch in (0, 1):                                                          # every kernel, in every mode
        assert {R.KERNELS[C][launch] for C in R.BN_C_MODES} == {'quad', 'any4', 'any1'}
    assert {R.KERNELS[c[0]][1] for c in R.CONTRACT_CASES} == {'quad', 'any4'}
    assert [R.side(C) for C in (1, 4, 12, 200, 256, 257, 512)] == [256, 256, 21, 1, 4, 1, 1]
    for C in R.BN_C:
        counts = R._pixel_counts(C)
        assert counts[0] == 1 and counts[-1] == 48 * R.side(C) + 5 and R.reduce_blocks(C, counts[-1]) == 4
        assert counts[-1] * C <= 1 << 20
    assert any(128 < c[0] <= 256 and not R.quad_bwd(c[0]) for c in R.BN_CASES)     # one pixel per round, idle threads


@pytest.mark.parametrize('case', R.BN_CASES, ids=list(map(R.case_id, R.BN_CASES)))
def test_bn_case_builds_and_float32_keeps_half_of_every_limit(case):
    d = R.bn_inputs(case)
    a = d['a']
    check_margin(a)
    check_slots(a)
    y, yb = a.fwd()
    top = dict(y=worst(a.fwd32(), y, R.lim(yb)))
    if a.mode == 'id':
        assert np.array_equal(a.fwd32(), a.s)
    else:
        assert np.array_equal(a.fwd32() > 0, a.on)
        dz, red, terms = a.reduce(d['dy64'])
        dz32, red32 = a.reduce32(d['dy'])
        assert np.array_equal(dz32.astype(np.float64), dz)
        top['red'] = worst(red32, red, R.sum_lim(terms + 1e-3))
        for red64 in (d['red64'], None):
            g, gb = a.apply(d['dz64'], red64)
            top['g'] = max(top.get('g', 0), worst(a.apply32(d['dz'], red64), g, R.lim(gb)))
        assert np.isnan(d['red'][d['rn']:]).all() and np.allclose(d['red'][:d['rn']].sum(0), d['red64'], rtol=1e-12, atol=1e-12)
        assert np.isfinite(d['prior']).all() and (d['prior'] != 0).all()
    assert max(top.values()) <= 0.5, top


@pytest.mark.parametrize('case', R.CONTRACT_CASES, ids=list(map(R.case_id, R.CONTRACT_CASES)))
def test_contract_case_builds(case):
    a, dy = R.contract_inputs(case)
    assert (dy != 0).all() and a.pre.shape == dy.shape
    assert (np.abs(a.pre) < R.MARGIN).sum() > (0 if a.mode != 'relu' else 1)       # no margin here: near-ties are the point


def test_conv_tables_cover_what_they_promise():
    ks = {c[3] for c in R.CONV_CASES} | {c[4] for c in R.CONV_CASES}
    assert {1, 15, 17, 18, 255, 256} <= ks
    assert {c[0] * c[1] * c[2] for c in R.CONV_CASES} >= {1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 65600, 131200}
    assert {c[5] for c in R.CONV_CASES} == set(R.ACTS)
    for pair in R.PAIRS:                                                           # every act mode meets 16-byte and scalar loads
        assert sum(c[3:5] == pair for c in R.CONV_CASES) >= 2
    for act in R.ACTS:
        assert {c[3] % 4 == 0 for c in R.CONV_CASES if c[5] == act} == {True, False}, act
    assert {(c[3] % 4 == 0, c[5]) for c in R.DGRAD_CASES} == {(a, b) for a in (True, False) for b in (True, False)}


def conv_ratios(case):
    d = R.conv_inputs(case)
    a = d['a']
    check_margin(a)
    check_slots(a)
    y32 = a.fwd32()
    out, ob = R.conv_fwd_ref(d)
    top = dict(out=worst(y32 @ d['w'] + d['b'], out, R.lim(ob)))
    dw, dwb, db, dbb = R.conv_wgrad_ref(d)
    one = np.ones((d['M'], 1), np.float32)
    top['dw'] = worst(R.matmul32(y32, d['g']), dw, R.lim(dwb, R.REL_W))
    top['db'] = worst(R.matmul32(one, d['g'])[0], db, R.lim(dbb, R.REL_W))
    # from a known prior
    top['dw+'] = worst(d['dw0'] + R.matmul32(y32, d['g']), d['dw064'] + dw, R.lim(dwb + np.abs(d['dw064']), R.REL_W))
    return top


@pytest.mark.parametrize('case', R.CONV_CASES, ids=list(map(R.case_id, R.CONV_CASES)))
def test_conv_case_builds_and_float32_keeps_half_of_every_limit(case):
    top = conv_ratios(case)
    assert max(top.values()) <= 0.5, top


@pytest.mark.parametrize('case', R.DGRAD_CASES, ids=list(map(R.case_id, R.DGRAD_CASES)))
def test_dgrad_case_builds_and_float32_keeps_half_of_every_limit(case):
    d = R.dgrad_inputs(case)
    dx, bound = R.conv_dgrad_ref(d)
    got = d['g'] @ d['w'].T
    if d['src'] is not None:
        check_margin(d['src'])
        assert d['src'].planted.any()
        got = np.where(d['src'].s > 0, got, np.float32(0))
        assert not dx[d['src'].planted].any()
    assert worst(got, dx, R.lim(bound)) <= 0.5


@pytest.mark.parametrize('case', R.IDENT_CASES, ids=list(map(R.case_id, R.IDENT_CASES)))
def test_identity_case_builds(case):
    n, H, W, C, act = case
    a = R.act_of(np.random.default_rng(R.seed(case)), n * H * W, C, act)
    check_margin(a)
    check_slots(a)
    assert R.KERNELS[C][0] == 'quad'


# ------------------------------------------------------------------ hiputil.BnMap is left as it was
# sha256 (first 16 hex digits) of what BnMap draws, taken before this file came
BNMAP_DRAWS = {
    (0, (3, 5, 7, 7), 8): '1a0c8c5311974133',
    (1, (2, 8, 8, 32), 8): 'f33d173db43ab984',
    (2, (5, 4, 4, 48), 3): 'ef3ceaa200ee7837',
}


def bnmap_digest(seed, shape, nslot, monkeypatch):
    import hiputil as U
    sent = {}
    monkeypatch.setattr(U, 'dev', lambda a, dtype=None: sent.setdefault(len(sent), np.ascontiguousarray(a)))
    bm = U.BnMap(np.random.default_rng(seed), shape, nslot)
    h = hashlib.sha256()
    for a in (bm.s, bm.gamma, bm.beta, bm.y, bm.m, bm.var, bm.xh) + tuple(sent[k] for k in sorted(sent)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def test_existing_bnmap_draws_are_unchanged(monkeypatch):
    for (seed, shape, nslot), want in BNMAP_DRAWS.items():
        assert bnmap_digest(seed, shape, nslot, monkeypatch) == want, (seed, shape, nslot)
