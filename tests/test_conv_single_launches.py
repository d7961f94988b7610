"""GPU parity: the SINGLE launches of the tuned 3x3 conv path -- mpnn_msconv_fwd, mpnn_msconv_dgrad_horz,
mpnn_msconv_dgrad_vert, mpnn_msconv_wgrad, and mpnn_conv_nhwc_* with supp == 3, which only fills their records --
through the C ABI against float64 (oracle/np_ops.py), on every kernel their dispatchers select.

The fused launches (tests/test_bwd_launches.py, tests/test_conv_fwd_lists.py, tests/test_conv_fwd_rep.py) only ever run
conv_body<GK,1,1,4,1,false,EPI_DGH_BN | EPI_DGV> and wgrad_body<GK, 1 | 4>.  The single launches are what the engine
emits under MPNN_STREAMS=1, what a single-scale `Conv` net runs, the fallback of the forward group and the anchor of the
suite's bit identities, and they instantiate other kernels: the 64-channel tile <0,2,2,2,2> of the 16-wide geometry under
all four epilogues, EPI_DGH_RAW with dy_extra / accumulate / g_ctx, wgrad_body<GK, 2> (the tap-slot form), operand widths
that are multiples of 4 but not of 16 (20, 24, 36), a 2- or 4-channel small operand, `prev` / `a` under MPNN_ACT_RELU and
MPNN_ACT_BN_MOVING.  `kernel_of` / `fwd_kernel_of` restate the two dispatchers (conv_launch, csrc/conv_kernel.h;
wgrad_launch, csrc/wgrad.hip); every row lists the kernels it is there for and asserts them, and a test without a GPU
asserts that the tables reach all 12 + 12 + 8 of them and every option the issue of this module lists (maps, widths,
modes, slots, operands, splits).

Rows are the smallest shapes at which a kernel can still go wrong: 4x16 (one tile per image), 12x16 (three tile rows),
8x32 (two tile columns); 8x8 at n = 3 and 5; 4x4 at n = 3 (less than one four-image tile), 5 and 9 (a ragged last tile).

Checks per row: tests/test_bwd_launches.py::check_oracle -- guards intact, every plain-store element written (NaN
pre-fill), out / dz_g_fine within 2e-5 (3e-5 with a BatchNorm on g or dz) x (1 + max|ref|), dW / db within 1e-4 x
(1 + max|ref|), red_out within 1e-5 x sum|term| per channel.  A raw dgrad-horz record carries a red_out between guards
that must come back untouched.  Forward rows: checks (a)-(c) of tests/test_conv_fwd_rep.py.

Cross-launch identities, as the code gives them.  mpnn_msconv_bwd_scale runs conv_body<GK,1,1,4,1> and
wgrad_body<GK, 4 | 1>; one workgroup computes a dgrad tile whole, in a fixed contraction order, so on the 16-channel tile
the single launch writes the same bits as the fused one; the 64-channel tile is held to the oracle's tolerance against
it.  Weight gradients are bit-identical where OT and SMALLC match at the same split and tile order; the single launch
never takes the XCD-aware tile order (its record leaves ConvP.xcd at 0; mpnn_msconv_bwd_scale sets it), so the row at
n = 32 with a split of 8 is held to fp32 rounding, as are OT 2 against OT 1 and the general body against SMALLC.
red_out: another workgroup partition, the oracle's bound.

Max-pool ties.  The header routes each window's gradient "to the FIRST maximum" (row-major window order, as
oracle/np_ops.pool2_bwd, held by tests/test_oracle_vs_torch.py).  The tie rows draw the finer map from multiples of 1/2 in
[-1, 1] (hiputil.grid_map), and run the same case through the single launches, mpnn_msconv_bwd_scale,
mpnn_msconv_dgrad_pair and a one-member mpnn_msconv_bwd_level.  Precondition, asserted on the host (and without a GPU in
test_tie_maps_hold_ties): at least a quarter of the 2x2 windows hold a tied maximum; positions 0, 1 and 2 each occur as
the first maximum of a tied window and positions 1, 2 and 3 each hold a later, losing copy -- position 3, the last in
window order, cannot be the FIRST of two equal maxima, so it is required as a loser and as an untied maximum instead.  A
wrong choice moves a whole value of order 1 against a limit of 3e-5.

Worst error / limit observed over the tables of this module, per output type, one run on an MI355X (WORST below;
MPNN_SINGLE_WORST=path writes it; check_oracle's own collection of relative errors goes where MPNN_BWD_WORST says):
  out 0.019   dz_g_fine 0.034   red_out 0.015   dWa 0.003   dWv 0.004   db 0.143 (rows with g_ctx, whose db sums
  a gradient the BatchNorm backward has centred; 0.002 without)
  forward out 0.030 (out_sum 0.003)   Conv supp 3: dx 0.022, dW 0.002, db 0.002
"""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from lib import _hip
from test_bwd_launches import M, check_oracle, close, same_dgrad, same_wgrad

S = _hip.BN_SLOTS
gpu = pytest.mark.gpu
WORST = {}          # worst error / LIMIT per output type over this module (MPNN_SINGLE_WORST=path: written there as JSON)
REL = {}            # check_oracle's own collection (worst relative error; MPNN_BWD_WORST=path writes it)
LIMIT = {'out': 2e-5, 'dz_g_fine': 3e-5, 'red_out': 1e-5, 'dWa': 1e-4, 'dWv': 1e-4, 'db': 1e-4}


def note(ratios):
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    if os.environ.get('MPNN_SINGLE_WORST'):
        with open(os.environ['MPNN_SINGLE_WORST'], 'w') as f:
            json.dump(WORST, f, indent=1)


def oracle(cs, r, what):
    """check_oracle of tests/test_bwd_launches.py, and its errors over their limits into WORST."""
    errs = check_oracle(cs, r, REL)
    lim = dict(LIMIT, out=3e-5 if cs.g_ctx is not None else 2e-5)
    ratios = {k: v / lim[k] for k, v in errs.items()}
    print(what, {k: '%.3f' % v for k, v in ratios.items()})
    note(ratios)


def hz(Cp, extra=False, acc=False, nslot=8, **kw):
    return dict(Cp=Cp, extra=extra, acc=acc, nslot=nslot, **kw)


def vt(Cf, has_dz=True, nslot=8, **kw):
    return dict(Cf=Cf, has_dz=has_dz, nslot=nslot, **kw)


RAW = dict(prev=None)


# ---------------------------------------------------------------------------------------------------- the dispatchers
def geom_of(H, W):
    """conv_launch / mpnn_wgrad_tiles: the geometry of a map, or None (MPNN_E_SHAPE)."""
    if W >= 16 and W % 16 == 0 and H % 4 == 0:
        return 'g16'
    return {(8, 8): 'g8', (4, 4): 'g4'}.get((H, W))


def is_raw(h):
    return 'prev' in h and h['prev'] is None


def kernel_of(spec, fused=False):
    """The kernels of a row: dgrad as (geometry, channel tile, epilogue) -- conv_launch_geom: the 64-channel tile on the
    16-wide geometry where Cout % 64 == 0, the 16-channel tile elsewhere -- and wgrad as (geometry, OT, SMALLC) --
    wgrad_launch: OT 4 / 2 / 1 by Cout % 64 / 32 / 16, SMALLC at OT 1 with a.C <= 3.
    fused: what mpnn_msconv_bwd_scale runs for the same member (bwd_scale_launch: 16-channel dgrad tiles; OT 4 or 1)."""
    g = geom_of(spec['H'], spec['W'])

    def dgrad(Cout, epi):
        return (g, 64 if g == 'g16' and Cout % 64 == 0 and not fused else 16, epi)

    k = {}
    if spec.get('horz'):
        k['horz'] = dgrad(spec['horz']['Cp'], 'DGH_RAW' if is_raw(spec['horz']) else 'DGH_BN')
    if spec.get('vert'):
        k['vert'] = dgrad(spec['vert']['Cf'], 'DGV')
    if spec.get('wgrad', True):
        Co, Ca = spec['Cg'], spec.get('a', ('bn', 16, S))[1]
        ot = 4 if Co % 64 == 0 else 2 if Co % 32 == 0 and not fused else 1
        k['wgrad'] = (g, ot, ot == 1 and Ca <= 3)
    return k


def fwd_kernel_of(mc):
    """conv_launch<EPI_FWD>: (geometry, channel tile, SMALL_A = a.C <= 4) of a forward member (H, W, Ca, ..., Cout, ...)."""
    H, W, Ca, Cout = mc[0], mc[1], mc[2], mc[6]
    g = geom_of(H, W)
    return (g, 64 if g == 'g16' and Cout % 64 == 0 else 16, Ca <= 4)


# ---------------------------------------------------------------------------------------------------- backward rows
# name -> (spec, the kernels the row is there for).  Tiles: 16-wide n * (W / 16) * (H / 4); 8x8 n; 4x4 ceil(n / 4).
ROWS = {
    # 4x16, one tile per image.  Raw horz (bare) and vert on the 64-channel tile, one row of it; OT 1, split 1
    'g16_4x16_raw64_dgv64_ot1': (
        M(3, 4, 16, 16, horz=hz(64, **RAW), vert=vt(64, has_dz=True, nslot=8), a=('bn', 16, 8), Cv=16, split=1),
        dict(horz=('g16', 64, 'DGH_RAW'), vert=('g16', 64, 'DGV'), wgrad=('g16', 1, False))),
    # 12x16, three tile rows; Cg 128 (eight chunks); two rows of the 64-channel tile; BN prev with extra + acc; OT 4, odd split
    'g16_12x16_bn128_dgv128_ot4': (
        M(2, 12, 16, 128, gctx=8, horz=hz(128, extra=True, acc=True, nslot=S), vert=vt(128, has_dz=False, nslot=1),
          a=('bn', 128, S), Cv=128, split=3),
        dict(horz=('g16', 64, 'DGH_BN'), vert=('g16', 64, 'DGV'), wgrad=('g16', 4, False))),
    # 8x32, two tile columns; output width 48 = three rows of the 16-channel tile; OT 2 on a 3-channel image (the general
    # body), Cv 36, split == tiles
    'g16_8x32_bn48_dgv48_ot2_img3': (
        M(2, 8, 32, 32, gctx=S, horz=hz(48, nslot=8), vert=vt(48, has_dz=True, nslot=S), a=('img', 3, 1), Cv=36,
          split=8),
        dict(horz=('g16', 16, 'DGH_BN'), vert=('g16', 16, 'DGV'), wgrad=('g16', 2, False))),
    # dgrad only: Cg 24 (a chunk of two channel quads) under g_ctx; raw horz with extra + acc
    'g16_4x16_cg24_dgrad_only': (
        M(5, 4, 16, 24, gctx=1, horz=hz(16, extra=True, acc=True, **RAW), vert=vt(16, has_dz=False, nslot=8),
          wgrad=False),
        dict(horz=('g16', 16, 'DGH_RAW'), vert=('g16', 16, 'DGV'))),
    # prev in RELU mode (what mpnn_conv_nhwc_dgrad builds) on the 64-channel tile; SMALLC on a 1-channel image, split > tiles
    'g16_4x16_relu64_smallc_img1': (
        M(2, 4, 16, 16, horz=hz(64, extra=True, nslot=1, prev_mode='relu'), a=('img', 1, 0), Cv=0, split=100),
        dict(horz=('g16', 64, 'DGH_BN'), wgrad=('g16', 1, True))),
    # raw horz with extra under g_ctx; OT 4 on a 2-channel image (the general body), shift 2
    'g16_4x16_raw16_gctx_ot4_img2': (
        M(2, 4, 16, 64, gctx=8, horz=hz(16, extra=True, **RAW), a=('img', 2, 2), Cv=16, split=2),
        dict(horz=('g16', 16, 'DGH_RAW'), wgrad=('g16', 4, False))),
    # the XCD-aware tile order of the fused launch (n % 32 == 0, split % 8 == 0): the single launch keeps the plain order
    'g16_4x16_n32_split8': (
        M(32, 4, 16, 16, a=('bn', 16, 8), Cv=0, split=8),
        dict(wgrad=('g16', 1, False))),
    # 8x8, n = 3: raw horz with acc; a of 20 channels, Cv 36
    'g8_n3_raw_acc_dgv_ot1_a20': (
        M(3, 8, 8, 16, horz=hz(32, acc=True, **RAW), vert=vt(16, has_dz=True, nslot=1), a=('bn', 20, 8), Cv=36,
          split=1),
        dict(horz=('g8', 16, 'DGH_RAW'), vert=('g8', 16, 'DGV'), wgrad=('g8', 1, False))),
    # 8x8, n = 5: prev under moving averages; a in RELU mode with 36 channels; OT 2, odd split
    'g8_n5_moving_dgv_ot2_relu36': (
        M(5, 8, 8, 32, gctx=8, horz=hz(16, extra=True, nslot=8, prev_mode='moving'), vert=vt(32, has_dz=False, nslot=S),
          a=('relu', 36), Cv=16, split=3),
        dict(horz=('g8', 16, 'DGH_BN'), vert=('g8', 16, 'DGV'), wgrad=('g8', 2, False))),
    # 8x8: SMALLC on a 3-channel image at shift 3, Cout 48, split == tiles; BN prev with acc
    'g8_n5_bn_acc_smallc_img3': (
        M(5, 8, 8, 48, horz=hz(16, acc=True, nslot=S), a=('img', 3, 3), Cv=0, split=5),
        dict(horz=('g8', 16, 'DGH_BN'), wgrad=('g8', 1, True))),
    # 8x8: OT 4 on a 1-channel image (the general body), Cv 128, g_ctx over all slots
    'g8_n3_ot4_img1_cv128': (
        M(3, 8, 8, 64, gctx=S, a=('img', 1, 2), Cv=128, split=2),
        dict(wgrad=('g8', 4, False))),
    # 4x4, n = 3 (less than one tile): bare raw horz; a under moving averages
    'g4_n3_raw_dgv_ot1_moving': (
        M(3, 4, 4, 16, horz=hz(16, **RAW), vert=vt(32, has_dz=True, nslot=8), a=('moving', 16, 8), Cv=0, split=1),
        dict(horz=('g4', 16, 'DGH_RAW'), vert=('g4', 16, 'DGV'), wgrad=('g4', 1, False))),
    # 4x4, n = 5 (ragged): prev in RELU mode with extra + acc, four tile rows; OT 2 on a 4-channel image
    'g4_n5_relu_dgv_ot2_img4': (
        M(5, 4, 4, 32, gctx=1, horz=hz(64, extra=True, acc=True, nslot=1, prev_mode='relu'),
          vert=vt(16, has_dz=False, nslot=S), a=('img', 4, 1), Cv=16, split=2),
        dict(horz=('g4', 16, 'DGH_BN'), vert=('g4', 16, 'DGV'), wgrad=('g4', 2, False))),
    # 4x4, n = 9 (ragged, three tiles): OT 4, a of 36 channels, Cv 36, split > tiles
    'g4_n9_dgv_ot4_a36': (
        M(9, 4, 4, 128, vert=vt(16, has_dz=True, nslot=8), a=('bn', 36, 1), Cv=36, split=7),
        dict(vert=('g4', 16, 'DGV'), wgrad=('g4', 4, False))),
    # 4x4: SMALLC on a 2-channel image, Cv 16, an odd split > tiles
    'g4_n5_smallc_img2': (
        M(5, 4, 4, 16, a=('img', 2, 0), Cv=16, split=3),
        dict(wgrad=('g4', 1, True))),
}

GEOMS = ('g16', 'g8', 'g4')
DGRAD_KERNELS = {(g, t, e) for g, t in (('g16', 16), ('g16', 64), ('g8', 16), ('g4', 16)) for e in ('DGH_RAW', 'DGH_BN', 'DGV')}
WGRAD_KERNELS = {(g, ot, sc) for g in GEOMS for ot, sc in ((4, False), (2, False), (1, False), (1, True))}
FWD_KERNELS = {(g, t, sm) for g, t in (('g16', 16), ('g16', 64), ('g8', 16), ('g4', 16)) for sm in (True, False)}

# ---------------------------------------------------------------------------------------------------- forward rows
# name -> ((H, W, Ca, act mode, shift, Cv, Cout, pool, out_nslot), n, the kernel)
FWD = {
    # (pool_out on a map less than 8 high is refused by the launcher, MPNN_E_SHAPE: tests/test_host_cpu.py)
    'g16x64_img3_4x16': ((4, 16, 3, 'img', 1, 16, 64, False, 8), 3, ('g16', 64, True)),
    'g16x64_img1_8x32': ((8, 32, 1, 'img', 0, 36, 64, True, S), 2, ('g16', 64, True)),
    'g16_img2_12x16': ((12, 16, 2, 'img', 0, 0, 48, True, 8), 2, ('g16', 16, True)),
    'g16_img4_4x16': ((4, 16, 4, 'img', 0, 16, 16, False, 5), 3, ('g16', 16, True)),
    'g8_img4_shift1': ((8, 8, 4, 'img', 1, 16, 32, True, 8), 3, ('g8', 16, True)),
    'g4_img2_shift1_n5': ((4, 4, 2, 'img', 1, 0, 16, False, 1), 5, ('g4', 16, True)),
    'g16x64_batch_a20_v36': ((8, 16, 20, 'batch', 0, 36, 64, True, 8), 3, ('g16', 64, False)),
    'g16_moving_a20_v36': ((8, 32, 20, 'moving', 0, 36, 16, True, S), 2, ('g16', 16, False)),
    'g8_relu_a20_v36': ((8, 8, 20, 'relu', 0, 36, 32, True, 8), 5, ('g8', 16, False)),
    'g4_batch_a20_v36_n5': ((4, 4, 20, 'batch', 0, 36, 16, False, 1), 5, ('g4', 16, False)),
}


# ---------------------------------------------------------------------------------------------------- coverage (CPU)
def _tiles(sp):
    g = geom_of(sp['H'], sp['W'])
    return {'g16': sp['n'] * (sp['W'] // 16) * (sp['H'] // 4), 'g8': sp['n'], 'g4': (sp['n'] + 3) // 4}[g]


def test_tables_reach_every_single_launch_kernel():
    """The 12 single dgrad kernels, the 12 wgrad kernels and the 8 forward kernels, and every option the module
    promises to cover, from the tables alone (nothing launches)."""
    dk, wk = set(), set()
    for name, (sp, want) in ROWS.items():
        assert kernel_of(sp) == want, name
        dk |= {want[k] for k in ('horz', 'vert') if k in want}
        wk |= {want[k] for k in ('wgrad',) if k in want}
    assert dk == DGRAD_KERNELS and wk == WGRAD_KERNELS
    assert {k for mc, _, k in FWD.values()} == FWD_KERNELS
    assert all(fwd_kernel_of(mc) == k for mc, _, k in FWD.values())
    specs = [sp for sp, _ in ROWS.values()]
    hs = [sp['horz'] for sp in specs if sp.get('horz')]
    vs = [sp['vert'] for sp in specs if sp.get('vert')]
    ws = [sp for sp in specs if sp.get('wgrad', True)]
    # maps
    assert {(sp['H'], sp['W']) for sp in specs} >= {(4, 16), (12, 16), (8, 32), (8, 8), (4, 4)}
    assert {sp['n'] for sp in specs if geom_of(sp['H'], sp['W']) == 'g8'} >= {3, 5}
    assert {sp['n'] for sp in specs if geom_of(sp['H'], sp['W']) == 'g4'} >= {3, 5, 9}
    # dgrad: output widths on the 16-wide geometry, K, options
    wide = [sp for sp in specs if geom_of(sp['H'], sp['W']) == 'g16']
    assert {sp[k][c] for sp in wide for k, c in (('horz', 'Cp'), ('vert', 'Cf')) if sp.get(k)} >= {16, 48, 64, 128}
    assert {sp['Cg'] for sp in specs if sp.get('horz') or sp.get('vert')} >= {16, 24, 128}
    for raw in (True, False):
        mine = [h for h in hs if is_raw(h) == raw]
        assert {(h['extra'], h['acc']) for h in mine} >= {(False, False), (True, True)}
        assert {h['extra'] for h in mine} == {False, True} and {h['acc'] for h in mine} == {False, True}
    assert any(is_raw(sp['horz']) and sp.get('gctx') for sp in specs if sp.get('horz'))
    assert {h.get('prev_mode', 'batch') for h in hs if not is_raw(h)} == {'batch', 'relu', 'moving'}
    assert {sp.get('gctx') for sp in specs} >= {None, 1, 8, S}
    assert {h['nslot'] for h in hs if not is_raw(h)} >= {1, 8, S} and {v['nslot'] for v in vs} >= {1, 8, S}
    assert {v['has_dz'] for v in vs} == {False, True}
    # wgrad: operand A, operand V, splits
    for g in GEOMS:
        assert {kernel_of(sp)['wgrad'][1] for sp in ws if geom_of(sp['H'], sp['W']) == g} == {1, 2, 4}
    assert {sp['a'][1] for sp in ws if sp['a'][0] == 'bn'} >= {16, 20, 36, 128}
    img = [sp for sp in ws if sp['a'][0] == 'img']
    assert {sp['a'][1] for sp in img if kernel_of(sp)['wgrad'][2]} == {1, 2, 3}                 # SMALLC
    assert {kernel_of(sp)['wgrad'][1] for sp in img if sp['a'][1] <= 3 and not kernel_of(sp)['wgrad'][2]} == {2, 4}
    assert 4 in {sp['a'][1] for sp in img} and {sp['a'][2] for sp in img} == {0, 1, 2, 3}
    assert {sp['a'][0] for sp in ws} >= {'relu', 'moving'}
    assert {sp.get('Cv', 0) for sp in ws} >= {0, 16, 36, 128}
    kinds = set()
    for sp in ws:
        t, s = _tiles(sp), sp.get('split', 1)
        kinds.add('1' if s == 1 else '>tiles' if s > t else '==tiles' if s == t else 'odd' if s % 2 else 'even')
    assert kinds >= {'1', 'odd', '==tiles', '>tiles'}
    assert any(sp['n'] == 32 and sp['split'] == 8 for sp in ws)
    # forward
    fw = [mc for mc, _, _ in FWD.values()]
    assert {(mc[0], mc[1]) for mc in fw if mc[2] <= 4 and mc[6] == 64 and mc[5] and mc[8]} >= {(4, 16), (8, 32)}
    assert all(mc[7] for mc in fw if mc[6] == 64 and mc[0] >= 8)          # pool_out on the 64-channel tile wherever it is admitted
    assert {(mc[2], mc[4]) for mc in fw} >= {(2, 0), (2, 1), (4, 0), (4, 1)}
    assert {mc[3] for mc in fw if mc[2] == 20 and mc[5] == 36} == {'batch', 'moving', 'relu'}
    assert any((mc[0], mc[1], mc[8]) == (4, 4, 1) and n == 5 for mc, n, _ in FWD.values())


# ---------------------------------------------------------------------------------------------------- backward rows
def _tol(cs, key):
    return 3e-5 if key == 'dzg' or cs.g_ctx is not None else 2e-5


def same_inputs_grads(cs, single, fused, kernels, keys, what):
    """Input gradients of the single launches against a fused launch of the same member: the same bits on the
    16-channel tile (the same body template, one workgroup per tile); the 64-channel tile within the oracle's
    tolerance of it.  red_out (another workgroup partition): 1e-5 * sum|term|."""
    for key, part in (('out', 'horz'), ('dzg', 'vert')):
        if key not in keys:
            continue
        a, b = single[key], fused[key]
        if kernels[part][1] == 16:
            assert np.array_equal(a, b), (what, key, np.abs(a - b).max())
        else:
            assert np.isfinite(a).all() and np.isfinite(b).all(), (what, key)
            assert np.abs(a - b).max() <= _tol(cs, key) * (1.0 + np.abs(b).max()), (what, key, np.abs(a - b).max())
    if 'out' in keys:
        ra, rb = single['red'].sum(0), fused['red'].sum(0)
        assert (np.abs(ra - rb) <= 1e-5 * cs.red_abs).all(), (what, 'red_out', np.abs(ra - rb).max())


@gpu
@pytest.mark.parametrize('name', list(ROWS))
def test_single_launches_vs_oracle(name):
    """Every output of the row's single launches against float64, then against mpnn_msconv_bwd_scale on the same
    records wherever that launch takes the member (it needs weight gradients and refuses a raw dgrad-horz)."""
    import hiputil as U
    spec, want = ROWS[name]
    k1 = kernel_of(spec)
    assert k1 == want, 'the dispatchers select other kernels for this row than it is listed for'
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cs = U.BwdCase(rng, spec)
    single = U.run_single(cs)
    oracle(cs, single, name)
    raw = cs.h is not None and cs.raw
    if raw:
        assert (single['red'] == U.RED_RAW).all(), 'a raw dgrad-horz launch wrote red_out'
    if cs.w is None:
        return
    fused = U.run_scale(cs, horz=not raw)
    assert cs.guards_ok(), 'a write outside the outputs'
    if not raw:
        check_oracle(cs, fused, None)
    keys = ([] if raw or cs.h is None else ['out']) + (['dzg'] if cs.v is not None else [])
    same_inputs_grads(cs, single, fused, k1, keys, name)
    k2 = kernel_of(spec, fused=True)
    xcd = cs.n % 32 == 0 and cs.split % 8 == 0           # (the fused launch alone takes the XCD-aware tile order)
    same_wgrad(single, fused, name, exact=k1['wgrad'] == k2['wgrad'] and not xcd)


# ---------------------------------------------------------------------------------------------------- max-pool ties
TIE_MAPS = {'4x16': (3, 4, 16), '8x8': (3, 8, 8), '4x4': (5, 4, 4)}          # (n, coarse H, coarse W); Cf = 16
TIE_SEED = 0


def tie_spec(geo, has_dz):
    n, H, W = TIE_MAPS[geo]
    return M(n, H, W, 16, horz=hz(16), vert=vt(16, has_dz=has_dz, nslot=8, ties=True, seed=TIE_SEED), a=('bn', 16, 8),
             Cv=16, split=1)


def assert_ties(s):
    """The precondition of a tie row (see the module docstring) on the finer map s."""
    import hiputil as U
    share, first, later, untied = U.tie_stats(s)
    assert share >= 0.25, share
    assert first == {0, 1, 2} and later == {1, 2, 3} and 3 in untied, (first, later, untied)


@pytest.mark.parametrize('geo', list(TIE_MAPS))
def test_tie_maps_hold_ties(geo):
    """The reference draw of every tie row satisfies the precondition (no GPU: the draw is pure numpy)."""
    import hiputil as U
    n, H, W = TIE_MAPS[geo]
    assert_ties(U.grid_map(np.random.default_rng(TIE_SEED), (n, 2 * H, 2 * W, 16)))


@gpu
@pytest.mark.parametrize('has_dz', [False, True])
@pytest.mark.parametrize('geo', list(TIE_MAPS))
def test_dgrad_vert_routes_ties_to_the_first_maximum(geo, has_dz):
    """The same case, four launches: single, mpnn_msconv_bwd_scale, mpnn_msconv_dgrad_pair, a one-member level."""
    import hiputil as U
    spec = tie_spec(geo, has_dz)
    n, H, W = TIE_MAPS[geo]
    cs = U.BwdCase(np.random.default_rng(zlib.crc32(('ties' + geo).encode()) + has_dz), spec)
    assert np.array_equal(cs.fine.s, U.grid_map(np.random.default_rng(TIE_SEED), (n, 2 * H, 2 * W, 16)))
    assert_ties(cs.fine.s)                                         # (before anything launches)
    single = U.run_single(cs)
    oracle(cs, single, 'ties %s has_dz %d' % (geo, has_dz))
    for what, run in (('bwd_scale', U.run_scale), ('bwd_level', lambda c: U.run_level([c])[0])):
        r = run(cs)
        check_oracle(cs, r, None)
        same_dgrad(single, r, what, cs.red_abs)
    r = U.run_pair(cs)
    assert cs.guards_ok(), 'a write outside the outputs'
    close(r['out'].reshape(cs.out_ref.shape), cs.out_ref, 2e-5, 'out (dgrad_pair)')
    close(r['dzg'].reshape(cs.dzg_ref.shape), cs.dzg_ref, 3e-5, 'dz_g_fine (dgrad_pair)')
    same_dgrad(single, r, 'dgrad_pair', cs.red_abs)


# ---------------------------------------------------------------------------------------------------- forward rows
@gpu
@pytest.mark.parametrize('name', list(FWD))
def test_single_forward_launch_vs_oracle(name):
    """mpnn_msconv_fwd on one record: checks (a)-(c) of tests/test_conv_fwd_rep.py."""
    import test_conv_fwd_rep as R
    mc, n, want = FWD[name]
    assert fwd_kernel_of(mc) == want, 'the dispatcher selects another kernel for this row than it is listed for'
    m = R.Member((name,) + mc[:8], n, out_nslot=mc[8])
    got, = R.launch([m], entry='fwd')
    sums = m.sums()
    R._check_buffers(m, mc, got, sums, name)
    ref = m.ref(np.arange(n))
    R._check_oracle(m, ref, got[0], name)
    R._check_stats(m, got[0], sums, name)
    lim = (3e-5 if m.bn else 2e-5) * (1.0 + np.abs(ref).max())
    note({'fwd out': np.abs(got[0].reshape(ref.shape) - ref).max() / lim})


# ---------------------------------------------------------------------------------------------------- Conv, supp == 3
@gpu
@pytest.mark.parametrize('n,H,W,ci,co', [(2, 12, 16, 64, 32), (5, 4, 4, 32, 16)], ids=['12x16', '4x4_n5'])
def test_conv_nhwc_dgrad_with_relu_src_between_guards(n, H, W, ci, co):
    """mpnn_conv_nhwc_dgrad, supp 3, with the producer's Rect: dx (NaN pre-filled) and a `scratch` of exactly the
    2 * Cin doubles the header promises, both between guards."""
    import torch
    import hiputil as U
    from oracle import np_ops as O
    lib = _hip.load()
    rng = np.random.default_rng(n * 100 + ci)
    x, x64 = U.f32(rng.standard_normal((n, H, W, ci)))
    w, w64 = U.f32(rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * ci))
    g, g64 = U.f32(rng.standard_normal((n, H, W, co)))
    xd, gd = U.dev(x), U.dev(g)
    bw = U.pack_weights([w])[1][0]
    dx, scratch = U.Guarded(x.size), U.Guarded(2 * ci, torch.float64)
    dx.fill(np.nan)
    scratch.fill(0.0)
    d = _hip.ConvNhwcDgradArgs()
    d.g, d.Cg, d.w = gd.data_ptr(), co, bw.data_ptr()
    d.relu_src, d.scratch, d.dx = xd.data_ptr(), scratch.ptr(), dx.ptr()
    d.n, d.H, d.W, d.Cin, d.supp = n, H, W, ci, 3
    _hip.check(lib.mpnn_conv_nhwc_dgrad(C.byref(d), U.stream()), 'conv_nhwc_dgrad')
    torch.cuda.synchronize()
    assert dx.guards_ok() and scratch.guards_ok(), 'a write outside dx or scratch'
    want = O.conv_same_bwd(np.maximum(x64, 0.0), w64, g64)[0] * (x64 > 0)
    note({'nhwc dx': close(dx.get().reshape(want.shape), want, 2e-5, 'dx') / 2e-5})


@gpu
def test_conv_nhwc_wgrad_split_3_into_a_slab():
    """mpnn_conv_nhwc_wgrad, supp 3, n_split = 3: partial sums into a slab, then mpnn_slab_reduce."""
    import torch
    import hiputil as U
    from oracle import np_ops as O
    lib = _hip.load()
    n, H, W, ci, co, split = 2, 12, 16, 16, 32, 3
    rng = np.random.default_rng(7)
    x, x64 = U.f32(rng.standard_normal((n, H, W, ci)))
    g, g64 = U.f32(rng.standard_normal((n, H, W, co)))
    xd, gd = U.dev(x), U.dev(g)
    sizes = [9 * ci * co, co]
    total = sum(sizes)
    stride = (total + 3) // 4 * 4
    slab, grads = U.Guarded(split * stride), U.Guarded(total)
    slab.fill(np.nan)
    grads.fill(np.nan)
    a = _hip.ConvNhwcWgradArgs()
    a.a = _hip.act(xd, ci, _hip.ACT_RELU)
    a.g, a.dw, a.db = gd.data_ptr(), slab.ptr(), slab.ptr(sizes[0])
    a.split_stride, a.n_split = stride, split
    a.n, a.H, a.W, a.Cout, a.supp = n, H, W, co, 3
    _hip.check(lib.mpnn_conv_nhwc_wgrad(C.byref(a), U.stream()), 'conv_nhwc_wgrad')
    item, tab = _hip.slab_item_size(split), []
    for o, sz in zip([0, sizes[0]], sizes):
        for k in range(0, sz, item):
            tab += [o + k, o + k, min(item, sz - k), split, stride, 0]
    t = U.dev(np.array(tab, np.int32), torch.int32)
    _hip.check(lib.mpnn_slab_reduce(slab.ptr(), grads.ptr(), t.data_ptr(), len(tab) // 6, U.stream()), 'slab_reduce')
    torch.cuda.synchronize()
    assert slab.guards_ok() and grads.guards_ok(), 'a write outside the slab or the gradients'
    got = grads.get()
    dw_ref = O.conv_same_bwd(np.maximum(x64, 0.0), np.zeros((3, 3, ci, co)), g64)[1]
    assert np.isfinite(got).all(), 'not every element written'
    db_ref = g64.sum((0, 1, 2))
    e1 = np.abs(got[:sizes[0]] - dw_ref.reshape(-1)).max() / (1e-4 * np.abs(dw_ref).max())      # (tests/test_conv_layer.py's limits)
    e2 = np.abs(got[sizes[0]:] - db_ref).max() / (1e-4 * np.abs(db_ref).max() + 1e-5)
    note({'nhwc dW': e1, 'nhwc db': e2})
    assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)
