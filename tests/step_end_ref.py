"""Float64 restatements (numpy, no GPU) of the launches that end a training step, and the shared case tables of
tests/test_step_end_kernels.py.  tests/test_step_end_ref_cpu.py holds every function here to an independent answer.

  bn_finalize_ref / spread_slots   mpnn_bn_finalize: moving averages, dgamma / dbeta, the [slot][2*C] sums it reads
  talr_ref                         mpnn_talr_momentum_step: TALR + L2 + momentum over a list of work items
  pack_ref                         mpnn_pack_weights: the forward / backward pack layout of include/mpnn_hip.h
  seg_path                         which of opt_seg's three pack-emission paths (csrc/opt_body.h) a work item takes
  route_lds_floats / route_rb      the host formula of mpnn_route (csrc/route.hip) that picks samples per workgroup
"""
import numpy as np

from oracle import np_ops as O

BN_SLOTS, SEG_INTS = 16, 12            # MPNN_BN_SLOTS, MPNN_SEG_INTS (lib/_hip.py carries the same; asserted on the CPU)


# ---------------------------------------------------------------------------------------------------- BatchNorm
def bn_finalize_ref(x, dz, gamma, state_m, state_v, decay, eps=1e-6):
    """x, dz: [n, H, W, C] pre-BN activations and the gradient at the BatchNorm's output.
    Moving averages after the step (layer_types.py:233-234: biased batch variance) and dbeta = sum dz,
    dgamma = sum dz * xhat; with them the fp64 mean / variance and xhat (for spread_slots)."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    _, m, v = O.bn_train(x, gamma, 0.0, eps)
    m_avg, v_avg = O.bn_moving(np.asarray(state_m, np.float64), np.asarray(state_v, np.float64), m, v, decay)
    _, dgamma, dbeta = O.bn_train_bwd(x, gamma, m, v, dz, eps)
    return dict(mean=m, var=v, m_avg=m_avg, v_avg=v_avg, dgamma=dgamma, dbeta=dbeta, xhat=(x - m) / np.sqrt(v + eps))


def spread_slots(x, dz, xhat, nslot, rng):
    """(sums, reds), each [nslot][2*C] float64 in the library's layout: row s holds, over the pixels dealt to slot s,
    [sum x | sum x^2] and [sum dz | sum dz * xhat].  Pixels go to slots at random (a slot may stay empty)."""
    c = x.shape[-1]
    x2, d2, h2 = (np.asarray(a, np.float64).reshape(-1, c) for a in (x, dz, xhat))
    slot = rng.integers(0, nslot, x2.shape[0])
    sums, reds = np.zeros((nslot, 2 * c)), np.zeros((nslot, 2 * c))
    for s in range(nslot):
        on = slot == s
        sums[s, :c], sums[s, c:] = x2[on].sum(0), (x2[on] ** 2).sum(0)
        reds[s, :c], reds[s, c:] = d2[on].sum(0), (d2[on] * h2[on]).sum(0)
    return sums, reds


# ---------------------------------------------------------------------------------------------------- optimizer
def talr_ref(P, A, G, items, stat, lr, mu, artr, talr, inv_n, grad_scale, w_eq=None):
    """net_types.py:24-37 + layer_types.py:52 over work items (offset, count, node, is_router, l2, w_eq offset | -1):
      g = grad_scale * G + 2 * l2 * pbar(node) * (w - w_eq);  g *= lr_scale(node) [* alpha_rtr for a router];
      accum = mu * accum + g;  w -= lr * accum
    pbar = mean p_tr, lr_scale = 1 / sqrt(mean p_tr^2) with TALR and 1 without (stat: [n_nodes][2] sums, inv_n = 1 /
    samples behind them); a router's alpha_rtr applies either way.  Returns float64 (params, accum)."""
    P64, A64, G64 = (np.array(a, np.float64) for a in (P, A, G))
    stat = np.asarray(stat, np.float64)
    for off, cnt, node, is_router, l2, eq_off in items:
        sl = slice(off, off + cnt)
        pbar = stat[node, 0] * inv_n
        sc = (1.0 / np.sqrt(stat[node, 1] * inv_n) if talr else 1.0) * (artr if is_router else 1.0)
        eq = np.asarray(w_eq[eq_off:eq_off + cnt], np.float64) if eq_off >= 0 else 0.0
        g = (np.asarray(G[sl], np.float64) * grad_scale + 2 * np.float64(np.float32(l2)) * pbar * (np.asarray(P[sl], np.float64) - eq)) * sc
        A64[sl] = mu * np.asarray(A[sl], np.float64) + g
        P64[sl] = np.asarray(P[sl], np.float64) - lr * A64[sl]
    return P64, A64


# ---------------------------------------------------------------------------------------------------- weight packs
def pack_sizes(cin, cout):
    return 9 * ((cin + 15) // 16) * 16 * cout, 9 * ((cout + 15) // 16) * 16 * cin


def pack_ref(w):
    """w: HWIO [3][3][Cin][Cout] float32.  (forward pack [9][nchF][4][Cout][4], backward pack [9][nchB][4][Cin][4]):
    fwd (tap, ch, gb, co, j) <- W[tap][ch*16+4gb+j][co]; bwd (tap, ch, gb, ci, j) <- W[8-tap][ci][ch*16+4gb+j]; the
    lanes of channels that do not exist are 0."""
    _, _, ci, co = w.shape
    wf = np.asarray(w, np.float32).reshape(9, ci, co)
    ref = np.zeros((9, (ci + 15) // 16, 4, co, 4), np.float32)
    for c in range(ci):
        ref[:, c // 16, (c % 16) // 4, :, c % 4] = wf[:, c, :]
    refb = np.zeros((9, (co + 15) // 16, 4, ci, 4), np.float32)
    for o in range(co):
        refb[:, o // 16, (o % 16) // 4, :, o % 4] = wf[::-1, :, o]
    return ref, refb


def seg_path(row):
    """The pack-emission path of opt_seg (csrc/opt_body.h) for one MPNN_SEG_INTS row, packs given:
    None (no pack: Cin = 0), 'tap' (fast, whole 4-row groups inside one tap), 'taps' (fast, whole taps), 'slow'."""
    off, cnt, tbase, cin, cout = row[0], row[1], row[6], row[7], row[8]
    if cin <= 0:
        return None
    R, row0 = cnt // cout, (off - tbase) // cout
    if not (cnt <= 2048 and cin % 4 == 0 and row0 % 4 == 0 and R % 4 == 0 and R * cout == cnt):
        return 'slow'
    if R <= cin and row0 % cin + R <= cin:
        return 'tap'
    if R % cin == 0 and row0 % cin == 0:
        return 'taps'
    return 'slow'


# The optimizer case: conv tensors [3][3][Cin][Cout] (the planner's pack rule: a forward pack each, a backward pack only
# with Cin % 16 == 0) with other tensors between them.  (name, Cin, Cout | size, node, is_router, l2, has w_eq)
OPT_TENSORS = [('r0', 0, 37, 1, 1, 1e-4, False), ('c3x16', 3, 16, 0, 0, 0.0, False), ('b0', 0, 16, 2, 0, 0.0, False),
               ('c4x16', 4, 16, 0, 0, 1e-4, False), ('c16x16', 16, 16, 3, 0, 1e-4, True), ('b1', 0, 201, 3, 0, 1e-4, False),
               ('c16x128', 16, 128, 2, 0, 0.0, False), ('b2', 0, 3, 1, 0, 0.0, False), ('c20x32', 20, 32, 1, 0, 1e-4, False),
               ('c32x16', 32, 16, 2, 0, 0.0, False), ('r1', 0, 2049, 3, 1, 0.0, False), ('c64x64', 64, 64, 3, 0, 1e-4, False),
               ('c128x128', 128, 128, 0, 0, 0.0, False)]
OPT_LISTS = {'chunks': 2048, 'p64': 64, 'p256': 256, 'p1024': 1024}      # work-item size (lib/_eng_alloc.py; slab items)
OPT_GAP = 8                            # sentinel floats between two tensors
EQ_OFF = 7                             # where the one w_eq tensor starts in the w_eq buffer


def l2_bits(l2):
    return int(np.float32(l2).view(np.int32))


def opt_layout(tensors=OPT_TENSORS, start=OPT_GAP):
    """Offsets of the tensors in params and of their packs.  Returns (list of dicts, params size, packs size)."""
    out, off, poff = [], start, 0
    for name, cin, co, node, rt, l2, has_eq in tensors:
        size = 9 * cin * co if cin else co
        t = dict(name=name, cin=cin, cout=co if cin else 0, size=size, off=off, node=node, rt=rt, l2=l2,
                 eq=EQ_OFF if has_eq else -1, fwd=-1, bwd=-1)
        if cin:
            fs, bs = pack_sizes(cin, co)
            t['fwd'] = poff
            poff += fs
            if cin % 16 == 0:
                t['bwd'] = poff
                poff += bs
        out.append(t)
        off += size + OPT_GAP
    return out, off, poff


def seg_rows(t, piece, off0=0, size=None):
    """MPNN_SEG_INTS rows of tensor t cut into `piece`-element work items (the last one ragged)."""
    rows = []
    size = t['size'] if size is None else size
    for s in range(0, size, piece):
        rows.append([t['off'] + s, min(piece, size - s), t['node'], t['rt'], l2_bits(t['l2']),
                     t['eq'] + s if t['eq'] >= 0 else -1, t['off'] if t['cin'] else 0, t['cin'], t['cout'], t['fwd'], t['bwd'], 0])
    return rows


def opt_rows(piece, tensors=None):
    tensors = opt_layout()[0] if tensors is None else tensors
    return [r for t in tensors for r in seg_rows(t, piece)]


def path_counts(rows):
    c = {'tap': 0, 'taps': 0, 'slow': 0}
    for r in rows:
        p = seg_path(r)
        if p is not None:
            c[p] += 1
    return c


def items_of(rows):
    """talr_ref's work items of MPNN_SEG_INTS rows."""
    return [(r[0], r[1], r[2], r[3], float(np.int32(r[4]).view(np.float32)), r[5]) for r in rows]


# ---------------------------------------------------------------------------------------------------- route
def route_lds_floats(n_nodes, n_switches, n_leaves, max_sinks):
    """(floats per sample, fixed floats) of mpnn_route's tables in LDS (the host formula of csrc/route.hip)."""
    return (4 * n_nodes + 2 * n_switches * max_sinks + n_switches + 2 * n_leaves,
            n_nodes * 5 + 8 + n_switches)


def route_rb(n_nodes, n_switches, n_leaves, max_sinks, cap=160 * 1024):
    """Samples per workgroup mpnn_route picks: the first of 64, 32, 16 whose tables fit `cap` bytes (None: refused)."""
    per, fix = route_lds_floats(n_nodes, n_switches, n_leaves, max_sinks)
    for rb in (64, 32, 16):
        if (per * rb + fix) * 4 <= cap:
            return rb
    return None
