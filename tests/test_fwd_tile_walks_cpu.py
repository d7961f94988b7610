"""The CPU half of tests/test_fwd_tile_walks.py: the restated grid rule (grid_rule) and the restated walk of the first
conv (first_walk) on hand-computed rows, and, for every row of that file's tables, the property the row is listed for
at every slot count the row can meet -- so the GPU table cannot silently stop reaching an nt, a strip height, three
rounds, the XCD-aware order or a carry."""
import pytest

import test_fwd_tile_walks as T
import test_conv_fwd_rep as R


def _first(H, W, C=3, pool=True):
    return (H, W, C, 'img', 0, 0, 16, pool, 16)


def test_grid_rule_of_the_first_conv_by_hand():
    # production, 4 096 images of 32x32: 65 536 tiles, grid = the slots, XCD-aware: 8 192 tiles an XCD over slots / 2 waves
    r, = T.grid_rule([_first(32, 32)], 4096, 1, 1, 2048)
    assert (r['gx'], r['xcd'], r['busiest'], r['idlest']) == (2048, True, 8, 8) and r['carries'] == (64, 0, 0)
    # the cap (n_tiles + 3) / 4: 5 images of 8x16 = 10 tiles -> 3 workgroups, waves 0 .. 9 one tile each, two idle
    r, = T.grid_rule([_first(8, 16)], 5, 3, 3, 1024)
    assert (r['gx'], r['xcd'], r['nt']) == (3, False, [1] * 10 + [0, 0])
    # xcd_round: 23 workgroups wanted -> 16; n % 32 != 0 keeps the plain order
    r, = T.grid_rule([_first(8, 16)], 46, 1, 1, 1024)
    assert (r['gx'], r['xcd']) == (16, False)
    # one workgroup, 4 waves, 6 / 14 / 22 tiles
    assert T.grid_rule([_first(8, 48)], 1, 1, 4096, 2048)[0]['nt'] == [2, 2, 1, 1]
    assert T.grid_rule([_first(8, 16)], 7, 1, 4096, 2048)[0]['nt'] == [4, 4, 3, 3]
    assert T.grid_rule([_first(44, 32)], 1, 1, 4096, 2048)[0]['nt'] == [6, 6, 5, 5]
    # the carries of nw = 4 on 3 tiles a row, 9 an image; of nw = 8 (two workgroups)
    assert T.grid_rule([_first(12, 48)], 2, 1, 4096, 8)[0]['carries'] == (0, 1, 1)
    assert T.grid_rule([_first(12, 48)], 3, 1, 16, 32)[0]['carries'] == (0, 2, 2)
    # n 96, 32x16 under the reservation: 768 tiles, 96 an XCD
    for slots, nt in ((8, 24), (16, 12), (24, 8), (32, 6), (48, 4), (64, 3)):
        r, = T.grid_rule([_first(32, 16)], 96, 1, 1, slots)
        assert (r['gx'], r['xcd'], r['busiest'], r['idlest']) == (slots, True, nt, nt)


def test_first_walk_visits_every_tile_once_and_its_carries_agree_with_division():
    for (H, W), n, gx, xa in (((8, 48), 1, 1, False), ((8, 16), 7, 1, False), ((44, 32), 1, 1, False), ((4, 48), 5, 1, False),
                              ((12, 48), 2, 1, False), ((12, 48), 3, 3, False), ((4, 16), 9, 1, False), ((12, 48), 5, 7, False),
                              ((32, 16), 96, 8, True), ((32, 16), 96, 64, True), ((12, 48), 32, 24, True)):
        walks, _ = T.first_walk(n, H, W, gx, xa)
        seen = sorted(t for seq in walks.values() for t in seq)
        assert seen == sorted((i, y, x) for i in range(n) for y in range(0, H, 4) for x in range(0, W, 16)), (H, W, n, gx)
        tx_n, tpi = W // 16, (W // 16) * (H // 4)
        for (b, w), seq in walks.items():                      # `origin` of tile c0 + k nw, by division
            for k, (img, y0, x0) in enumerate(seq):
                j = ((b // 8 if xa else b) * 4 + w) + k * ((gx // 8 if xa else gx) * 4)
                ij, rem = divmod(j, tpi)
                want_img = (ij >> 2 << 5) + 4 * (b & 7) + (ij & 3) if xa else ij
                assert (img, y0, x0) == (want_img, rem // tx_n * 4, rem % tx_n * 16), (H, W, n, gx, b, w, k)
    # one advance that wraps a column, a row and the image: tile 5 = (row 1, column 2) of image 0 + 4 -> tile 0 of image 1
    walks, events = T.first_walk(2, 12, 48, 1, False)
    assert walks[(0, 1)][1:3] == [(0, 4, 32), (1, 0, 0)] and 'col+row' in events


def test_grid_rule_of_the_strips_by_hand():
    st = lambda H, W, Cv=0: (H, W, 16, 'moving', 0, Cv, 16, True, 16)
    rh = lambda H, W, n, share=4096, slots=1024: T.grid_rule([st(H, W)], n, 1, share, slots)[0]['rh']
    # one workgroup: "the longest strip that still gives every wave a strip"
    assert [rh(12, 16, n) for n in (1, 2, 3, 4)] == [4, 6, 6, 12]              # H 12: 12 / 6 / 4
    assert [rh(20, 16, n) for n in (1, 2, 3, 4)] == [4, 10, 10, 20]            # H 20: 20 / 10 / 4 (5 is odd)
    assert [rh(24, 16, n) for n in (1, 2, 3, 4)] == [6, 12, 12, 24]            # H 24: 24 / 12 / 6 / 4
    assert rh(24, 32, 1) == 12 and rh(12, 32, 1) == 6 and rh(8, 32, 2) == 8 and rh(32, 32, 2) == 32 and rh(8, 16, 1) == 4
    # production, 4 096 images of 32x32 on 1 024 slots: rh == H
    r, = T.grid_rule([(32, 32, 16, 'moving', 0, 0, 16, True, 8)], 4096, 1, 1, 1024)
    assert (r['body'], r['gx'], r['rh'], r['xcd'], r['busiest'], r['idlest']) == ('strip16', 1024, 32, True, 2, 2)
    # the cap (n_tiles + 3) / 4: 22 images of 8x16 at share 24 = 44 tiles -> 11 workgroups at most
    r, = T.grid_rule([(8, 16, 16, 'batch', 0, 0, 16, True, 8)], 22, 1, 24, 1024)
    assert (r['body'], r['gx'], r['rh'], r['per']) == ('strip16', 11, 4, [1] * 44)
    # 64 images of 8x16 at share 8 on 32 slots: 4 workgroups, 16 waves, 64 strips of 8 rows
    r, = T.grid_rule([st(8, 16)], 64, 1, 8, 32)
    assert (r['gx'], r['rh'], r['per']) == (4, 8, [4] * 16)


def test_grid_rule_of_the_general_body_by_hand():
    g8 = (8, 8, 32, 'moving', 0, 16, 32, True, 16)
    # one member: slots / gy workgroups a tile row, at most the tiles; xcd_round; XCD-aware only on multiples of 8
    r, = T.grid_rule([g8], 64, 1, 1, 32)
    assert (r['body'], r['gx'], r['gy'], r['xcd'], r['upt'], r['per']) == ('g8', 16, 2, True, 3, [4] * 16)
    r, = T.grid_rule([g8], 64, 1, 1, 24)
    assert (r['gx'], r['xcd'], r['busiest'], r['idlest']) == (12, False, 6, 5)
    r, = T.grid_rule([g8], 64, 1, 1, 1024)
    assert (r['gx'], r['xcd'], r['busiest']) == (64, True, 1)
    r, = T.grid_rule([g8], 7, 1, 4096, 1024)
    assert (r['gx'], r['xcd'], r['per']) == (1, False, [7])
    # the split by work: 'four bodies' of tests/test_conv_fwd_rep.py, 5 images, one net on 1 024 slots
    # work = tiles x tile rows x chunks: 10 x 2 x 2, 5 x 2 x 3, 2 x 2 x 4, 2 x 1 x 4 = 40, 30, 16, 8 of 94
    rule = T.grid_rule([R.B16W, R.B8, R.B4, R.B4V], 5, 1, 1, 1024)
    assert [r['body'] for r in rule] == ['g16', 'g8', 'g4', 'g4'] and [r['gx'] for r in rule] == [10, 5, 2, 2]
    rule = T.grid_rule([R.B16W, R.B8, R.B4, R.B4V], 32, 1, 1, 32)               # 64 x 2 x 2, 32 x 2 x 3, 8 x 2 x 4, 8 x 4 = 256, 192, 64, 32 of 544
    assert [r['gx'] for r in rule] == [7, 5, 1, 1] and not any(r['xcd'] for r in rule)
    # K-split: gx x gy within the slots
    r, = T.grid_rule([(8, 8, 64, 'batch', 0, 0, 64, True, 16)], 96, 1, 1, 32)
    assert (r['body'], r['gx'], r['gy'], r['xcd'], r['upt'], r['per']) == ('ks8', 8, 4, True, 2, [12] * 8)
    r, = T.grid_rule([(4, 4, 64, 'batch', 0, 64, 128, False, 16)], 96, 1, 1, 24)
    assert (r['body'], r['gx'], r['xcd'], r['per']) == ('ks4', 3, False, [8, 8, 8])
    # a list: the host sizes the grid from the capacity, the device walks the count's tiles
    r, = T.grid_rule([(8, 8, 32, 'moving', 0, 16, 64, True, None)], 40, 1, 1, 64, counts=[17])
    assert (r['body'], r['gx'], r['xcd'], r['busiest'], r['idlest']) == ('g8', 16, False, 2, 1)


@pytest.mark.parametrize('name', list(T.ROWS))
def test_every_row_reaches_what_it_is_listed_for(name):
    members, n, reps, share, how, want = T.ROWS[name]
    mcs = [mb[0] for mb in members]
    assert R.bodies_of(mcs, n, reps, share) == [mb[1] for mb in members]
    assert n <= 96 and want
    for slots in T.slots_of(how):
        rule = T.check_want(want, mcs, n, reps, share, slots, name)
        assert [r['body'] for r in rule] == [mb[1] for mb in members]
        if how == 'forced':
            assert all(r['gx'] == 1 for r in rule)
        else:
            assert all(1 <= r['gx'] <= 64 for r in rule)
        if how == 'readback':                                  # out_nslot = 16 must show every workgroup
            for r, mc in zip(rule, mcs):
                waves = len(r['per']) // r['gx']               # (4: the wave-per-tile kernels)
                assert r['gx'] <= 8 and mc[8] == 16 and all(sum(r['per'][b * waves:(b + 1) * waves]) for b in range(r['gx']))
    s2 = T.alt_share(mcs, n, reps, share)                      # (d) runs the same bodies
    assert R.bodies_of(mcs, n, reps, s2) == [mb[1] for mb in members] and (share > 1 or s2 == 1)


def test_the_table_covers_the_issue():
    """Every nt of 1 .. 6 on one workgroup, every listed strip height, every body, C = 1, 2, 3, with and without
    pool_out / out_sum, the plain and the REP first conv."""
    rows = T.ROWS.values()
    first = [r for r in rows if r[0][0][1] == 'first' and r[4] == 'forced']
    assert set().union(*(r[5]['nt'] for r in first)) == {1, 2, 3, 4, 5, 6}
    assert {r[0][0][0][2] for r in first} == {1, 2, 3}
    assert {(r[0][0][0][7], r[0][0][0][8] is not None, r[2] > 1) for r in first} >= \
        {(True, True, False), (False, True, False), (True, False, False), (True, True, True), (False, False, True)}
    assert {r[0][0][0][1] for r in first} >= {16, 48} and {r[0][0][0][0] for r in first} >= {4, 12}
    strips = [r for r in rows if r[0][0][1].startswith('strip') and r[4] == 'forced' and len(r[0]) == 1]
    assert {(r[0][0][0][0], r[5]['rh'][0]) for r in strips} >= {(8, 8), (32, 32), (24, 12), (24, 6), (12, 6), (20, 10), (8, 4), (20, 4)}
    assert {r[0][0][1] for r in strips} == {'strip16', 'stripk', 'stripk+small'}
    assert {r[0][0][0][3] for r in strips} == {'moving', 'batch', 'img'}
    assert {(r[0][0][0][2] + r[0][0][0][5]) // 16 for r in strips if r[0][0][1] == 'stripk'} == {2, 3}
    # (d) of the forced strip rows: on 1 024 .. 2 048 slots (4 .. 8 workgroups a compute unit x 256; the group kernels
    # are bounded for 4 and were found at 4) their wider grid runs another strip height in at least five of them --
    # placement invariance then holds ACROSS strip heights (on 512 slots in two of them)
    for slots in range(1024, 2056, 512):
        other = 0
        for r in strips:
            mcs, n, share = [r[0][0][0]], r[1], r[3]
            s2 = T.alt_share(mcs, n, 1, share)
            other += T.grid_rule(mcs, n, 1, s2, slots)[0]['rh'] != T.grid_rule(mcs, n, 1, share, slots)[0]['rh']
        assert other >= 5, (slots, other)
    bodies = {mb[1] for r in rows for mb in r[0]} | set(T.XCD_SMALL) | {r[0][0] for r in T.LISTED}
    assert bodies >= {'first', 'strip16', 'stripk', 'stripk+small', 'g16', 'g16+small', 'g8', 'g8+small', 'g4', 'wide8', 'wide4', 'ks8', 'ks4'}
    forced_upt = {r[5]['upt'] for r in rows if r[4] == 'forced' and 'upt' in r[5]}
    assert forced_upt >= {1, 2, 3, 4}
    assert {r[0][0][1] for r in rows if r[5].get('xcd')} == {'first', 'g16'}


@pytest.mark.parametrize('kind', list(T.XCD_SMALL))
def test_fitted_small_map_rows_run_eight_workgroups_on_any_device(kind):
    for per_cu in range(1, 9):
        probe, n, _ = T.xcd_small_member(kind, 1)
        assert R.bodies_of([probe], n, 1, 8) == [kind]
        assert T.grid_rule([probe], n, 1, 8, 8 * per_cu)[0]['gx'] == per_cu
        mc, n, rounds = T.xcd_small_member(kind, per_cu)
        assert R.bodies_of([mc], n, 1, 1) == [kind] and n <= 96
        r, = T.check_want(dict(gx=[8], xcd=True, rounds=rounds), [mc], n, 1, 1, 8 * per_cu, kind)
        assert r['per'] == [rounds] * 8 and rounds >= 3


@pytest.mark.parametrize('row', T.LISTED, ids=[r[0][0] for r in T.LISTED])
def test_listed_rows_keep_the_xcd_order_off(row):
    case, n, counts = row
    mc = tuple(case[1:]) + (None,)
    import test_conv_fwd_lists as L
    assert L.expected_body(case, n) == case[0]
    assert counts[0] == n and 0 < counts[1] < n and counts[2] == 0
    for slots in T.RESERVED_SLOTS:
        for c in counts:
            r, = T.grid_rule([mc], n, 1, 1, slots, counts=[c])
            assert r['body'] == case[0] and (c == 0 or not r['xcd'])
        assert T.grid_rule([mc], n, 1, 1, slots, counts=[n])[0]['busiest'] >= 1
