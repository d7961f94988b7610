"""The tile walks of the persistent forward conv launches (csrc/conv_fwd.hip: mpnn_msconv_fwd_group and
mpnn_msconv_fwd_group_rep; csrc/conv_first.hip, csrc/conv_strip.h, conv_body of csrc/conv_kernel.h) on grids of ONE TO
EIGHT workgroups per tile row, through the C ABI, on the GPU.

Every forward launch fits its grid to resident_slots() (csrc/common.h) and each workgroup -- in the first conv and the
strip bodies each WAVE -- then walks its tiles.  The other forward files run whatever ratio of tiles to grid the device
yields, mostly about one.  Here the ratio is controlled, with two handles of the public API:

  * `share` of mpnn_msconv_fwd_group_rep: the grid is resident_slots / share with a floor of 1.  share = 4096 exceeds any
    slot count of the header's residency model (8 four-wave workgroups x 256 compute units = 2048), so every member gets
    ONE workgroup per tile row on any device; the same share satisfies the evaluation thresholds (n * share >= 512 strips,
    >= 1024 32-channel tiles), which makes every body reachable at n = 1 .. 9;
  * mpnn_set_reserved_cus: resident_slots floors the free compute units at 8, so a reservation larger than the device
    leaves 8 x (workgroups per compute unit) slots: 8, 16, .. 64.  It also applies to mpnn_msconv_fwd_group (reps =
    share = 1), the only way onto the XCD-aware tile order, the sample-list bodies and the K-split body.

`grid_rule` restates the launchers' grid rule as a function of the slot count (next to body_of / bodies_of of
tests/test_conv_fwd_lists.py and tests/test_conv_fwd_rep.py, which restate the body selection): gx per member with
xcd_round, the (n_tiles + 3) / 4 cap and the split by work, the strip height rh, whether the XCD-aware order is taken,
the tiles (strips) of the busiest and the idlest workgroup (wave), and for the first conv nt per wave and the carries.
`first_walk` restates the first conv's incremental walk (origin / advance / image).  tests/test_fwd_tile_walks_cpu.py pins
both on hand-computed rows and asserts for every row of the tables below the property the row is listed for (`want`),
so the tables cannot silently stop reaching what they are there to reach.

How a row knows the grid it ran on (`how`):
  forced    share = 4096: gx == 1 for every member for every slot count up to 2048 (asserted without a GPU); on the GPU
            the members that carry out_sum (out_nslot = 16; slot = workgroup % 16) must have contributed to slot 0 only;
  readback  full reservation, share 8 .. 16: the out_sum slots that received a contribution are exactly the workgroups
            that had work, which gives gx; the slot counts 8 .. 64 that the restated rule maps to that gx give rh and the
            rounds, and the row's `want` is asserted at them;
  bounded   full reservation, share = 1: slots is one of 8, 16, .. 64 (mpnn_msconv_bwd_level_slots under the same
            reservation is asserted to be one of them too) and `want` holds at all eight (asserted without a GPU); the
            slots that out_sum shows must be min(gx, 16) of one of the eight.
  The XCD-aware order of the 8x8 and the 4x4 body cannot be held to three rounds at all eight slot counts -- at n <= 96
  it needs gx == 8 (4x4) or gx <= 16 (8x8) exactly, and gx is proportional to the slots.  test_xcd_order_of_the_small_maps
  therefore reads the workgroups per compute unit of the launch's kernel back first (the same kernel at share 8 under the
  reservation: gx = that number) and fits Cout = 16 x it, which makes gx == 8 on any device; out_sum then shows exactly
  eight workgroups.

Every launch is held to (tolerances of tests/test_conv_fwd_rep.py):
  a. buffers: guards intact, every out / pool_out element written (NaN-filled Guarded buffers), slots >= out_nslot of
     out_sum untouched;
  b. float64 (oracle/np_ops.py) on the activation as the kernel sees it: 2e-5 (identity / image) or 3e-5 (BatchNorm on
     load) x (1 + max |ref|); pool_out the exact 2x2 max of the launch's own out;
  c. out_sum over its slots against the float64 sums of the launch's own stored out: 1e-5 sum |term| + 1e-9;
  d. placement invariance -- the header's "speed only: any placement gives the same results": the same records on the
     widest grid that still selects the same bodies (no reservation; share = 1 where the row has it, else the smallest
     share with the row's bodies) write the same BITS of out and pool_out; for the strips that launch has another gx and,
     where the rule says so, another strip height (the heights of both launches are printed).  Every record through
     mpnn_msconv_fwd as well: the same bits, except the bodies that sum in another order than the single launch
     (multi-chunk strips, K-split: ORDER_DIFFERS of tests/test_conv_fwd_rep.py), held to 2e-5 x (1 + max) as (e) there.
     No body's per-element contraction order was found to depend on the placement: the tile decides WHICH elements a
     workgroup computes, the order over taps and chunks is fixed per tile;
  e. determinism: a second launch on fresh buffers gives the same bits, out_sum per slot to 1e-12 relative.

Mutants (libraries built aside, each run once against this file and, for contrast, against tests/test_conv_fwd_rep.py,
test_conv_fwd_lists.py, test_hip_conv.py, test_fwd_bodies_fuzz.py and test_conv_single_launches.py -- 274 cases, "the
existing files"; not kept).  Every mutant run keeps each access inside the launch's buffers: it changes which tile is
done, or what is zeroed, not where memory is touched.
  * `advance` whose row carry does not step the image (conv_first.hip): 'first, H 4 .. W 48', 'first REP, W 48 H 12' and
    'first, 1 .. 4 workgroups read back' fail; the existing files all pass.
  * `advance` whose column carry does not step the row: the same three rows fail; the existing files all pass.
  * the loop tail `if (i < nt)` dropped: all eight first-conv rows fail; of the existing files test_first_conv_kernel (4)
    and three fuzz cases fail.
  * the second half of the steady-state loop taking its operands from the wrong register set: 'first, 22 tiles', 'first
    REP, W 48 H 12' and the XCD row fail (it needs nt >= 5: at nt == 4 the set holds the re-issued last tile); of the
    existing files one fuzz case fails.
  * `image(ij)` of the first conv's XCD order with `ij & 1`: 'first, the XCD-aware order, 768 tiles' fails; of the
    existing files test_first_conv_kernel (2) and one fuzz case.
  * xcd_tile (conv_kernel.h) with `ij & 1`: both 'g16, the XCD-aware order' rows, 'ks8' and
    test_xcd_order_of_the_small_maps[g8] fail (the 4x4 form `8 j + x` does not use the expression); 11 existing cases.
  * gen_next stepping the tile by 1 instead of sqd (stays below sqn: in bounds): the two g16 XCD rows, 'ks8', 'ks4' and the
    listed g8 and g16+small fail; the one-workgroup rows pass, as they must (sqd == 1); 77 existing cases fail.
  * strip16_body zeroing the halo rows at the STRIP's ends instead of the image's (wrong only where rh < H): every
    strip16 row fails, the rh == H rows through (d) -- their wider grid runs rh 4 and 16; 31 existing cases fail.
  Argued from the code, not run: `next()` advancing past the end only changes what is LOADED two tiles ahead (the tiles past
  nt are never computed), i.e. nothing a test can see, and reads past the input; gen_next stepping by sqd after the
  first part instead of the last leaves the tile range (n_units stays my_tiles x upt), i.e. stores past the output; the
  strips' pooled row taken on the parity of the strip-relative row is the SAME program: rh is even by construction (the
  launcher only takes even divisors of H, or 4), so y0 = ys * rh is even.

Worst error / limit measured on the MI355X over the tables: out 0.055 ('g16+small, the image + four chunks of V'),
out_sum 0.008 ('wide8', on the grid of (d)), the bodies of another summation order against mpnn_msconv_fwd 0.053
('ks4').  The whole file runs in 2.7 s.  The group kernels were found at 4 workgroups per compute unit under the
reservation (32 slots), the K-split kernel at 2 (16 slots); (d) ran the forced strip rows at rh 8 -> 4, 32 -> 16,
12 -> 6, 6 -> 4 and 10 -> 4."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from lib import _hip
import test_conv_fwd_lists as L
import test_conv_fwd_rep as R
from test_conv_fwd_lists import Member, launch

pytestmark = pytest.mark.gpu

FORCE = 4096                                                   # > 2048 slots: one workgroup per tile row on any device
RESERVED_SLOTS = tuple(range(8, 72, 8))                        # 8 compute units x 1 .. 8 workgroups each
FORCED_SLOTS = tuple(range(8, 2056, 8))


def xcd_round(g):
    return g & ~7 if g >= 16 else g


def _count(c0, cn, cd):
    """Terms of c0, c0 + cd, .. < cn."""
    return (cn - 1 - c0) // cd + 1 if c0 < cn else 0


def grid_rule(mcs, n, reps, share, slots, counts=None):
    """The grids of one forward launch (fwd_group_launch in csrc/conv_fwd.hip, first_conv_launch in
    csrc/conv_first.hip) for `slots` = resident_slots() of its kernel; counts: the device counts of a listed launch.
    One dict per member: body, gx, gy, rh, xcd, upt (units per tile), per (the tiles of every workgroup -- for the
    wave-per-tile kernels the tiles / strips of every WAVE, workgroup-major), busiest, idlest; the first conv also
    nt (= per) and carries (d_img, d_ty, d_tx)."""
    if counts is None:
        bodies = R.bodies_of(mcs, n, reps, share)
    else:
        cases = [('',) + tuple(mc[:8]) for mc in mcs]
        bodies = [L.expected_body(c, n, cases) for c in cases]
    use_xcd = reps == 1 and share == 1
    units = [(mc[2] + 15) // 16 + (mc[5] + 15) // 16 for mc in mcs]

    def done(d, per):
        d.update(per=per, busiest=max(per), idlest=min(per))
        return d

    if bodies == ['first']:
        H, W = mcs[0][:2]
        tx_n, tpi = W // 16, (W // 16) * (H // 4)
        n_tiles = n * tpi
        gx = max(1, min(slots // share, (n_tiles + 3) // 4))  # a wave per tile: no more workgroups than a quarter of the tiles
        gx = xcd_round(gx) if use_xcd else gx
        xa = use_xcd and n % 32 == 0 and gx % 8 == 0
        nw, jn = (gx // 8 * 4, n_tiles // 8) if xa else (gx * 4, n_tiles)
        per = [_count((b // 8 if xa else b) * 4 + w, jn, nw) for b in range(gx) for w in range(4)]
        d_rem = nw % tpi
        d = dict(body='first', gx=gx, gy=1, rh=None, xcd=xa, upt=1, carries=(nw // tpi, d_rem // tx_n, d_rem % tx_n))
        return [done(d, per) | dict(nt=per)]
    if bodies[0] in ('ks8', 'ks4'):                            # one deep member alone: two chunks per unit, its own kernel
        H, W, Cout = mcs[0][0], mcs[0][1], mcs[0][6]
        n_tiles, gy = (n if H == 8 else (n + 3) // 4), Cout // 16
        gx = n_tiles if n_tiles * gy <= slots else max(slots // gy, 1)
        gx = xcd_round(gx)
        xa = n % 32 == 0 and gx % 8 == 0
        sqd, sqn = (gx // 8, n_tiles // 8) if xa else (gx, n_tiles)
        per = [_count(b // 8 if xa else b, sqn, sqd) for b in range(gx)]
        return [done(dict(body=bodies[0], gx=gx, gy=gy, rh=None, xcd=xa, upt=units[0] // 2), per)]
    slots = max(slots // share, 1)
    out, work, tiles, gys = [], [], [], []
    for mc, b in zip(mcs, bodies):
        H, W, Cout = mc[0], mc[1], mc[6]
        t = n * (W // 16) * (H // 4) if b.startswith(('g16', 'strip')) else n if b in ('g8', 'g8+small', 'wide8') else (n + 3) // 4
        gys.append(Cout // (32 if b.startswith('wide') else 16))
        tiles.append(t)
        work.append(t * gys[-1] * units[len(work)])
    for k, (mc, b) in enumerate(zip(mcs, bodies)):
        H, W = mc[:2]
        strip = b.startswith('strip')
        g = min(max(slots * work[k] // sum(work) // gys[k], 1), tiles[k])
        if strip:
            g = min(g, (tiles[k] + 3) // 4)
        gx = xcd_round(g) if use_xcd else g
        n_dev = n if counts is None else min(counts[k], n)
        d = dict(body=b, gx=gx, gy=gys[k], rh=None, upt=units[k])
        if strip:
            cols, rh, r = n * (W // 16), 4, H
            while r > 4:
                if r % 2 == 0 and H % r == 0 and cols * (H // r) >= 4 * gx:
                    rh = r
                    break
                r >>= 1
            xa = use_xcd and n % 32 == 0 and gx % 8 == 0 and counts is None
            tpi = (W // 16) * (H // rh)
            nw, jn = (gx // 8 * 4, n // 8 * tpi) if xa else (gx * 4, n_dev * tpi)
            per = [_count((bx // 8 if xa else bx) * 4 + w, jn, nw) for bx in range(gx) for w in range(4)]
            d.update(rh=rh, xcd=xa)
        else:
            t_dev = tiles[k] if counts is None else (n_dev * (W // 16) * (H // 4) if b.startswith('g16') else
                                                      n_dev if b.startswith(('g8', 'wide8')) else (n_dev + 3) // 4)
            xa = use_xcd and n_dev % 32 == 0 and gx % 8 == 0
            sqd, sqn = (gx // 8, t_dev // 8) if xa else (gx, t_dev)
            per = [_count(bx // 8 if xa else bx, sqn, sqd) for bx in range(gx)]
            d.update(xcd=xa)
        out.append(done(d, per))
    return out


def first_walk(n, H, W, gx, xa):
    """The first conv's walk (fwd_first_k): {(workgroup, wave): [(image, y0, x0), ..]} by `origin` for the first tile and
    `advance` (carries, no division) for the rest, and the set of carry events met: 'col', 'row', 'col+row' (one
    advance wraps a column and a row -- with it the image steps as well), 'img' (d_img > 0 or a row carry)."""
    tx_n, ty_n = W // 16, H // 4
    tpi, n_tiles = tx_n * ty_n, n * tx_n * ty_n
    nw, jn = (gx // 8 * 4, n_tiles // 8) if xa else (gx * 4, n_tiles)
    d_img, d_rem = nw // tpi, nw % tpi
    d_ty, d_tx = d_rem // tx_n, d_rem % tx_n
    walks, events = {}, set()
    for b in range(gx):
        image = (lambda ij: (ij >> 2 << 5) + 4 * (b & 7) + (ij & 3)) if xa else (lambda ij: ij)
        for w in range(4):
            c0 = (b // 8 if xa else b) * 4 + w
            nt = _count(c0, jn, nw)
            seq = []
            if nt:
                ij, rem = divmod(c0, tpi)
                ty, tx = divmod(rem, tx_n)
                seq.append((image(ij), ty * 4, tx * 16))
                for _ in range(nt - 1):
                    tx, ty, ij = tx + d_tx, ty + d_ty, ij + d_img
                    col = tx >= tx_n
                    if col:
                        tx, ty = tx - tx_n, ty + 1
                    row = ty >= ty_n
                    if row:
                        ty, ij = ty - ty_n, ij + 1
                    events |= {e for e, on in (('col', col), ('row', row), ('col+row', col and row), ('img', row or d_img > 0)) if on}
                    seq.append((image(ij), ty * 4, tx * 16))
            walks[(b, w)] = seq
    return walks, events


# member: (H, W, Ca, act mode, shift, Cv, Cout, pool, out_nslot or None: no out_sum)
# row: name -> (members: (member, body), n, reps, share, how, want); want: what the row is listed for, asserted of
# grid_rule / first_walk at every slot count of `how` in tests/test_fwd_tile_walks_cpu.py:
#   gx, rh: per member; xcd; nt: values some wave must have; nt_differ: waves of one launch with different nt;
#   carries; events: carry events of first_walk; rounds: the busiest workgroup (wave) walks at least that many tiles;
#   upt: units per tile; idle: some wave / workgroup walks nothing; ragged: the last 4x4 tile holds fewer than 4 images
def _first(H, W, C, pool, nslot):
    return (H, W, C, 'img', 0, 0, 16, pool, nslot)


ROWS = {
    # ---- the first conv on ONE workgroup (4 waves): the peeled pipeline and the carries
    'first, 6 tiles: nt 2 and 1 (the peeled head alone, the even tail)':
        ([(_first(8, 48, 3, True, 16), 'first')], 1, 1, FORCE, 'forced', dict(gx=[1], nt={1, 2}, nt_differ=True, carries=(0, 1, 1))),
    'first, W 16 (left and right edge in one tile), 14 tiles: nt 4 and 3':
        ([(_first(8, 16, 1, False, 16), 'first')], 7, 1, FORCE, 'forced', dict(gx=[1], nt={3, 4}, nt_differ=True, carries=(2, 0, 0))),
    'first, 22 tiles: nt 6 and 5 (two loop trips, odd and even tail), no out_sum':
        ([(_first(44, 32, 2, True, None), 'first')], 1, 1, FORCE, 'forced', dict(gx=[1], nt={5, 6}, nt_differ=True, carries=(0, 2, 0))),
    'first, H 4 (top and bottom in one tile) W 48: one advance wraps column, row and image':
        ([(_first(4, 48, 3, False, 16), 'first')], 5, 1, FORCE, 'forced', dict(gx=[1], nt={3, 4}, carries=(1, 0, 1), events={'col+row', 'img'})),
    'first REP, W 48 H 12: nw 4 against 3 tiles a row, 9 an image':
        ([(_first(12, 48, 3, True, 16), 'first')], 2, 2, FORCE, 'forced', dict(gx=[1], nt={4, 5}, carries=(0, 1, 1), events={'col', 'row', 'col+row'})),
    'first REP, H 4 W 16 (a tile an image), no pool, no out_sum':
        ([(_first(4, 16, 2, False, None), 'first')], 9, 2, FORCE, 'forced', dict(gx=[1], nt={2, 3}, carries=(4, 0, 0))),
    'first, 1 .. 4 workgroups read back':
        ([(_first(12, 48, 3, True, 16), 'first')], 3, 1, 16, 'readback', dict(rounds=2)),
    'first, the XCD-aware order, 768 tiles':
        ([(_first(32, 16, 3, True, 16), 'first')], 96, 1, 1, 'bounded', dict(xcd=True, rounds=3)),
    # ---- the strip bodies on one workgroup: every strip height
    'strip16, rh == H == 8':
        ([((8, 32, 16, 'moving', 0, 0, 16, True, 16), 'strip16')], 2, 1, FORCE, 'forced', dict(gx=[1], rh=[8])),
    'strip16, rh == H == 32, batch statistics, two tile rows':
        ([((32, 32, 16, 'batch', 0, 0, 32, True, 16), 'strip16')], 2, 1, FORCE, 'forced', dict(gx=[1], rh=[32])),
    'stripk two chunks, rh 12 of H 24':
        ([((24, 32, 16, 'moving', 0, 16, 16, True, 16), 'stripk')], 1, 1, FORCE, 'forced', dict(gx=[1], rh=[12])),
    'stripk three chunks, rh 6 of H 24, batch statistics':
        ([((24, 16, 32, 'batch', 0, 16, 16, True, 16), 'stripk')], 1, 1, FORCE, 'forced', dict(gx=[1], rh=[6])),
    'stripk+small, rh 6 of H 12':
        ([((12, 32, 3, 'img', 1, 16, 16, True, 16), 'stripk+small')], 1, 1, FORCE, 'forced', dict(gx=[1], rh=[6])),
    'strip16, rh 10 of H 20, batch statistics, waves with 2 and 1 strips':
        ([((20, 16, 16, 'batch', 0, 0, 16, True, 16), 'strip16')], 3, 1, FORCE, 'forced', dict(gx=[1], rh=[10], nt_differ=True)),
    'stripk two chunks, rh 10 of H 20, no out_sum':
        ([((20, 16, 16, 'moving', 0, 16, 32, True, None), 'stripk')], 2, 1, FORCE, 'forced', dict(gx=[1], rh=[10])),
    'strip16, rh 4, two waves idle':
        ([((8, 16, 16, 'moving', 0, 0, 16, True, 16), 'strip16')], 1, 1, FORCE, 'forced', dict(gx=[1], rh=[4], idle=True)),
    'stripk+small, rh 4 of H 20 (10 is too long for one column), no pool':
        ([((20, 16, 3, 'img', 2, 16, 16, False, 16), 'stripk+small')], 1, 1, FORCE, 'forced', dict(gx=[1], rh=[4], nt_differ=True)),
    'strip16 read back: every wave several strips of different images':
        ([((8, 16, 16, 'moving', 0, 0, 16, True, 16), 'strip16')], 64, 1, 8, 'readback', dict(rh=[8], rounds=2)),
    'stripk read back, batch statistics':
        ([((12, 16, 16, 'batch', 0, 16, 16, True, 16), 'stripk')], 64, 1, 8, 'readback', dict(rounds=2)),
    # ---- the general body on one workgroup per tile row: one, two, three and more units per tile, ragged n
    'g8, one unit a tile (weights staged once)':
        ([((8, 8, 16, 'id', 0, 0, 16, True, 16), 'g8')], 7, 1, FORCE, 'forced', dict(gx=[1], upt=1, rounds=7)),
    'g8, A + V: two units a tile, batch statistics':
        ([((8, 8, 16, 'batch', 0, 16, 16, True, 16), 'g8')], 9, 1, FORCE, 'forced', dict(gx=[1], upt=2, rounds=9)),
    'g4, three units a tile (two chunks of A, then V), ragged':
        ([((4, 4, 32, 'moving', 0, 16, 16, False, 16), 'g4')], 6, 1, FORCE, 'forced', dict(gx=[1], upt=3, rounds=2, ragged=True)),
    'g4, one unit a tile, ragged, no out_sum':
        ([((4, 4, 16, 'batch', 0, 0, 16, False, None), 'g4')], 9, 1, FORCE, 'forced', dict(gx=[1], upt=1, rounds=3, ragged=True)),
    'g16, four units a tile (two chunks a part)':
        ([((8, 16, 32, 'moving', 0, 32, 16, True, 16), 'g16')], 5, 1, FORCE, 'forced', dict(gx=[1], upt=4, rounds=10)),
    'g16+small, the image alone: one unit a tile':
        ([((8, 16, 3, 'img', 1, 0, 16, True, 16), 'g16+small')], 5, 1, FORCE, 'forced', dict(gx=[1], upt=1, rounds=10)),
    'g16+small, the image + four chunks of V':
        ([((8, 16, 1, 'img', 2, 64, 16, True, 16), 'g16+small')], 5, 1, FORCE, 'forced', dict(gx=[1], upt=5, rounds=10)),
    'g8+small':
        ([((8, 8, 3, 'img', 2, 16, 16, False, 16), 'g8+small')], 6, 1, FORCE, 'forced', dict(gx=[1], upt=2, rounds=6)),
    'wide8':
        ([((8, 8, 32, 'moving', 0, 32, 64, True, 16), 'wide8')], 5, 1, FORCE, 'forced', dict(gx=[1], upt=4, rounds=5)),
    'wide4, batch statistics, ragged':
        ([((4, 4, 64, 'batch', 0, 0, 128, False, 16), 'wide4')], 9, 1, FORCE, 'forced', dict(gx=[1], upt=4, rounds=3, ragged=True)),
    "the four members of tests/test_conv_fwd_rep.py's 'four bodies', a workgroup a tile row each":
        ([(R.B16W, 'stripk'), (R.B8, 'g8'), (R.B4, 'g4'), (R.B4V, 'g4')], 5, 1, FORCE, 'forced', dict(gx=[1, 1, 1, 1], rh=[8, None, None, None])),
    'the same four members, two nets':
        ([(R.B16W, 'stripk'), (R.B8, 'g8'), (R.B4, 'g4'), (R.B4V, 'g4')], 6, 2, FORCE, 'forced', dict(gx=[1, 1, 1, 1])),
    # ---- reps = share = 1 under the reservation: the XCD-aware order and the K-split body on 8 .. 64 slots
    'g16, the XCD-aware order, n 32':
        ([((32, 16, 16, 'moving', 0, 16, 16, True, 16), 'g16')], 32, 1, 1, 'bounded', dict(xcd=True, rounds=3, upt=2)),
    'g16, the XCD-aware order, n 64, one unit a tile':
        ([((16, 16, 16, 'id', 0, 0, 16, True, 16), 'g16')], 64, 1, 1, 'bounded', dict(xcd=True, rounds=3, upt=1)),
    'ks8: one deep 8x8 member, batch statistics':
        ([((8, 8, 64, 'batch', 0, 0, 64, True, 16), 'ks8')], 96, 1, 1, 'bounded', dict(rounds=3)),
    'ks4: one deep 4x4 member, A + V, batch statistics':
        ([((4, 4, 64, 'batch', 0, 64, 128, False, 16), 'ks4')], 96, 1, 1, 'bounded', dict(rounds=3)),
}

# The XCD-aware order of the 8x8 and the 4x4 body: (member with Cout = 16, n, the rounds); Cout is fitted to the device.
XCD_SMALL = {
    'g8': ((8, 8, 32, 'moving', 0, 16, 16, True, 16), 64, 8),
    'g4': ((4, 4, 64, 'moving', 0, 0, 16, False, 16), 96, 3),
}


def xcd_small_member(kind, per_cu):
    mc, n, rounds = XCD_SMALL[kind]
    return mc[:6] + (16 * per_cu,) + mc[7:], n, rounds


# The sample-list bodies under the reservation: (case of tests/test_conv_fwd_lists.py, capacity, counts)
LISTED = [
    (('g8', 8, 8, 32, 'moving', 0, 16, 64, True), 40, (40, 17, 0)),
    (('g4', 4, 4, 64, 'moving', 0, 0, 32, False), 42, (42, 9, 0)),
    (('g16+small', 16, 16, 3, 'img', 1, 16, 16, True), 40, (40, 17, 0)),
]


def slots_of(how):
    return FORCED_SLOTS if how == 'forced' else RESERVED_SLOTS


def alt_share(mcs, n, reps, share):
    """(d): the smallest share that selects the row's bodies -- the widest grid the same kernels can run on."""
    want = R.bodies_of(mcs, n, reps, share)
    return next(s for s in range(1, share + 1) if R.bodies_of(mcs, n, reps, s) == want)


def check_want(want, mcs, n, reps, share, slots, what):
    """The properties a row is listed for, of the restated rule at one slot count."""
    rule = grid_rule(mcs, n, reps, share, slots)
    what = '%s at %d slots: %s' % (what, slots, [(r['gx'], r['rh'], r['xcd'], r['per']) for r in rule])
    if 'gx' in want:
        assert [r['gx'] for r in rule] == want['gx'], what
    if 'rh' in want:
        assert [r['rh'] for r in rule] == want['rh'], what
    if 'xcd' in want:
        assert all(r['xcd'] == want['xcd'] for r in rule), what
    if 'nt' in want:
        assert want['nt'] <= set(rule[0]['per']), what
    if want.get('nt_differ'):
        assert len(set(rule[0]['per'][:4])) > 1, what
    if want.get('idle'):
        assert rule[0]['idlest'] == 0, what
    if 'rounds' in want:
        assert all(r['busiest'] >= want['rounds'] for r in rule), what
    if 'upt' in want:
        assert rule[0]['upt'] == want['upt'], what
    if want.get('ragged'):
        assert n % 4 and rule[0]['body'] in ('g4', 'wide4'), what
    if 'carries' in want or 'events' in want:
        r = rule[0]
        assert r['body'] == 'first' and r['carries'] == want.get('carries', r['carries']), what
        _, events = first_walk(n, mcs[0][0], mcs[0][1], r['gx'], r['xcd'])
        assert want.get('events', set()) <= events, (what, events)
    return rule


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _no_reservation_leaks():
    lib = _hip.load()
    assert lib.mpnn_set_reserved_cus(-1) == 0
    yield
    assert lib.mpnn_set_reserved_cus(-1) == 0


@contextlib.contextmanager
def reservation(full):
    """Every compute unit but the floor of 8 reserved (full) or none; nothing leaks."""
    lib = _hip.load()
    assert lib.mpnn_set_reserved_cus(-1) == 0
    try:
        if full:
            lib.mpnn_set_reserved_cus(1 << 20)
        yield
    finally:
        lib.mpnn_set_reserved_cus(0)
    assert lib.mpnn_set_reserved_cus(-1) == 0


def used_slots(m):
    """The out_sum slots that received a contribution (the sums of squares of random data are positive)."""
    return [int(s) for s in np.flatnonzero(np.abs(m.sums()).sum(1) > 0)]


def level_slots_reserved():
    arr = lambda *v: (C.c_int * len(v))(*v)
    return _hip.load().mpnn_msconv_bwd_level_slots(arr(32, 8), arr(32, 8), arr(16, 16), 2)


def check_members(nets, mcs, got, sums, what):
    """(a), (b), (c) of every member of every net."""
    for r, net in enumerate(nets):
        for k, m in enumerate(net.ms):
            w = '%s, net %d member %d' % (what, r, k)
            out, pool = got[r][k]
            assert np.isfinite(out).all(), w + ': out not written everywhere'
            if mcs[k][7]:
                import hiputil as U
                assert np.isfinite(pool).all(), w + ': pool_out not written everywhere'
                mine = U.pool2_np(out.reshape(m.n, m.H, m.W, m.Cout)).reshape(m.n, -1)
                assert np.array_equal(pool, mine), w + ': pool_out is not the 2x2 max of out'
            R._check_oracle(m, net.refs[k], out, w)
            if m.osum is not None:
                assert (sums[r][k][mcs[k][8]:] == 0).all(), w + ': a slot >= out_nslot of out_sum was written'
                R._check_stats(m, out, sums[r][k], w)


def joint(nets, reps, share):
    got = launch([net.ms for net in nets], entry='rep', reps=reps, share=share)
    return got, [[m.sums() if m.osum is not None else None for m in net.ms] for net in nets]


def same_bits(nets, a, b, what):
    for r, net in enumerate(nets):
        for k in range(len(net.ms)):
            assert R._bits(a[r][k][0], b[r][k][0]) and R._bits(a[r][k][1], b[r][k][1]), '%s, net %d member %d' % (what, r, k)


def established_gx(nets, mcs, n, reps, share, how, want, name):
    """The grid the launch just ran on, from out_sum; returns the slot counts consistent with it."""
    seen = [[used_slots(m) if m.osum is not None else None for m in net.ms] for net in nets]
    ok = []
    for slots in slots_of(how) if how != 'forced' else (8,):
        rule = grid_rule(mcs, n, reps, share, slots)
        if all(u is None or u == list(range(min(r['gx'], 16))) for net in seen for u, r in zip(net, rule)):
            ok.append(slots)
    assert ok, '%s: the workgroups that out_sum shows %s fit no slot count of %s' % (name, seen, how)
    if how == 'readback':                                      # gx is known exactly (<= 8): every consistent slot count gives it
        for slots in ok:
            rule = check_want(want, mcs, n, reps, share, slots, name)
            assert all(1 <= r['gx'] <= 8 for r in rule)
    print('%s: out_sum shows the workgroups %s; slot counts that give them: %s' % (name, seen[0], ok))
    return ok


@pytest.mark.parametrize('name', list(ROWS))
def test_tile_walk(name):
    members, n, reps, share, how, want = ROWS[name]
    mcs = [mb[0] for mb in members]
    assert R.bodies_of(mcs, n, reps, share) == [mb[1] for mb in members], 'the launcher selects other bodies than the row lists'
    nets = [R.Net(mcs, n, r) for r in range(reps)]
    with reservation(how != 'forced'):
        if how == 'bounded':
            assert level_slots_reserved() in RESERVED_SLOTS
        got, sums = joint(nets, reps, share)
        check_members(nets, mcs, got, sums, name)
        ok = established_gx(nets, mcs, n, reps, share, how, want, name)
        again, sums2 = joint(nets, reps, share)                # (e)
    same_bits(nets, again, got, name + ': the second run')
    for r, net in enumerate(nets):
        for k, m in enumerate(net.ms):
            if m.osum is not None:
                R._same_slots(sums2[r][k], sums[r][k], '%s: the second run, net %d member %d' % (name, r, k))
    # (d) the widest grid of the same bodies
    s2 = alt_share(mcs, n, reps, share)
    wide, wsums = joint(nets, reps, s2)
    same_bits(nets, wide, got, '%s: the grid of share %d without a reservation' % (name, s2))
    check_members(nets, mcs, wide, wsums, '%s at share %d' % (name, s2))
    if any(mb[1].startswith('strip') for mb in members):
        seen = [used_slots(m) if m.osum is not None else None for m in nets[0].ms]
        fits = [s for s in range(256, 2056, 8) if all(u is None or u == list(range(min(r['gx'], 16)))
                                                         for u, r in zip(seen, grid_rule(mcs, n, reps, s2, s)))]
        rhs = sorted({tuple(r['rh'] for r in grid_rule(mcs, n, reps, s2, s)) for s in fits})
        print('%s: strip heights %s at %d slots, %s on the grid of share %d (workgroups %s)' %
              (name, [r['rh'] for r in grid_rule(mcs, n, reps, share, ok[0])], ok[0], rhs, s2, seen))
    for r, net in enumerate(nets):                             # ... and the single launch of every record
        for k, m in enumerate(net.ms):
            what = '%s, net %d member %d: mpnn_msconv_fwd' % (name, r, k)
            one, = launch([m], entry='fwd')
            if members[k][1] in R.ORDER_DIFFERS:
                err = np.abs(one[0] - got[r][k][0]).max() / (2e-5 * (1.0 + np.abs(one[0]).max()))
                print('%s: worst difference / limit = %.3f' % (what, err))
                assert err <= 1.0, what
            else:
                assert R._bits(one[0], got[r][k][0]) and R._bits(one[1], got[r][k][1]), what


@pytest.mark.parametrize('kind', list(XCD_SMALL))
def test_xcd_order_of_the_small_maps(kind):
    """The XCD-aware order of the 8x8 / 4x4 body on exactly eight workgroups: 8 and 3 rounds."""
    probe, n, rounds = xcd_small_member(kind, 1)
    with reservation(True):
        pm = R.Net([probe], n, 7)
        launch([pm.ms], entry='rep', reps=1, share=8)          # the same kernel: gx = its workgroups per compute unit
        per_cu = len(used_slots(pm.ms[0]))
        assert 1 <= per_cu <= 8 and used_slots(pm.ms[0]) == list(range(per_cu))
        assert grid_rule([probe], n, 1, 8, 8 * per_cu)[0]['gx'] == per_cu
        mc, n, rounds = xcd_small_member(kind, per_cu)
        assert R.bodies_of([mc], n, 1, 1) == [kind]
        rule = check_want(dict(gx=[8], xcd=True, rounds=rounds), [mc], n, 1, 1, 8 * per_cu, kind)
        assert rule[0]['busiest'] == rule[0]['idlest'] == rounds
        net = R.Net([mc], n, 0)
        got, sums = joint([net], 1, 1)
        check_members([net], [mc], got, sums, kind)
        assert used_slots(net.ms[0]) == list(range(8)), 'not the eight workgroups the restated rule gives'
        again, sums2 = joint([net], 1, 1)
    same_bits([net], again, got, kind + ': the second run')
    R._same_slots(sums2[0][0], sums[0][0], kind + ': the second run')
    wide, wsums = joint([net], 1, 1)                           # (d) the default grid
    same_bits([net], wide, got, kind + ': the default grid')
    check_members([net], [mc], wide, wsums, kind + ' on the default grid')
    one, = launch([net.ms[0]], entry='fwd')
    assert R._bits(one[0], got[0][0][0]) and R._bits(one[1], got[0][0][1]), kind + ': mpnn_msconv_fwd'


@pytest.mark.parametrize('row', LISTED, ids=[r[0][0] for r in LISTED])
def test_listed_bodies_on_a_small_grid(row):
    """mpnn_msconv_fwd_group with idx / cnt under the reservation -- a full, a partial and an empty list: the listed rows
    carry the bits of the same launch on the default grid and of the dense launch, the oracle's values, and every other
    row is still NaN.  The XCD-aware order is off (count % 32 != 0; asserted of the restated rule at every slot count)."""
    import hiputil as U
    case, n, counts = row
    mc = tuple(case[1:]) + (None,)
    m = Member(case, n)
    dense, = launch([m])
    rng = np.random.default_rng(L._seed(row))
    for c in counts:
        for slots in RESERVED_SLOTS:
            r, = grid_rule([mc], n, 1, 1, slots, counts=[c])
            assert r['body'] == case[0] and (c == 0 or not r['xcd']) and (c > 0 or r['busiest'] == 0)
        perm = rng.permutation(n)
        m.set_list(*L._dev_list(perm, c))
        listed = perm[:c]
        with reservation(True):
            small, = launch([m])
            again, = launch([m])
        what = '%s, count %d' % (case[0], c)
        L._check(small, dense, listed, n, what)
        if c == 0:
            assert L._all_nan(small), what
        for a, b in zip(small, again):                         # (e); NaN rows included
            assert a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)), what + ': the second run'
        default, = launch([m])                                 # (d)
        for a, b in zip(small, default):
            assert a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)), what + ': the default grid'
        if c:
            ref = m.ref(listed)
            lim = (3e-5 if m.bn else 2e-5) * (1.0 + np.abs(ref).max())
            err = np.abs(small[0][listed].reshape(ref.shape) - ref).max()
            print('%s: out worst error / limit = %.3f' % (what, err / lim))
            assert err <= lim, what
            if small[1] is not None:
                mine = U.pool2_np(small[0][listed].reshape(len(listed), m.H, m.W, m.Cout))
                assert np.array_equal(small[1][listed], mine.reshape(len(listed), -1)), what + ': pool_out is not the 2x2 max of out'
        m.set_list(None, None)
