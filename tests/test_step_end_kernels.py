"""GPU: the launches that end a training step, each alone through the C ABI against the float64 references of
tests/step_end_ref.py (held to independent answers in tests/test_step_end_ref_cpu.py):

  mpnn_bn_finalize                      five BatchNorm records in one launch: C up to 256 (the block has 128 threads),
                                        1 to 16 slots, a record nobody consumes (gamma_goff = -1), constant channels
                                        whose variance cancels to rounding noise; sums_keep on / off, reds on / off
  mpnn_backward_finish                  == mpnn_slab_reduce, then mpnn_bn_finalize, bit for bit
  mpnn_talr_momentum_step(..., packs)   the three pack-emission paths of opt_seg (csrc/opt_body.h) over 2048-element
                                        chunks and slab-item sized pieces; packs == mpnn_pack_weights(new parameters)
  mpnn_backward_finish_opt / _multi     == mpnn_slab_reduce, mpnn_bn_finalize, mpnn_talr_momentum_step, bit for bit;
                                        three nets in one launch == three launches

Every buffer a launch may write is a hiputil.Guarded one whose gaps -- between records, between tensors, the slots a
record does not use -- hold the sentinel too; "bit for bit" compares whole buffers, guards included, as integers.

Tolerances:
  moving averages       the project's close(..., 1e-6): |err| <= 1e-6 * (1 + max|ref|) per record (an fp64 mean cast
                        once and one fp32 update: three roundings)
  dgamma, dbeta         1 ulp of fp32, 2^-23 * |ref| (one cast of an fp64 sum; half an ulp if the sum is exact), plus
                        2^-48 * sum|terms| for the float64 sums themselves -- the reference's pairwise sum over up to
                        5120 pixels and the kernel's sum over the slots (1e-6 of an ulp where nothing cancels)
  parameters, accum     close(..., 1e-6) against talr_ref, as tests/test_exit_kernels.py::test_talr_momentum_step
  slab sums             2e-6 * sqrt(split) * (1 + max|ref|), as tests/test_hip_conv.py::test_slab_reduce_items_and_groups
Fused against composed, multi against single and packs against mpnn_pack_weights are exact.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lib import _hip
from hiputil import DEV, SENTINEL, Guarded, dev, stream
import step_end_ref as R
from test_exit_gen_kernels import close as lim_close

DECAY, EPS, N_IMG = float(np.float32(0.9)), 1e-6, 5
ULP = 2.0 ** -23
SENT32 = np.float32(SENTINEL)
LR, MU, ARTR, N_STAT, N_NODES = 0.05, 0.9, 1.7, 128, 4


def up(a, dtype=torch.float32):
    g = Guarded(a.size, dtype)
    g.fill(a)
    return g


def itab(rows):
    a = np.array(rows, np.int32).reshape(-1)
    return dev(a if a.size else np.zeros(1, np.int32), torch.int32)


def bits(g):
    a = g.buf.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b, what):
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        assert np.array_equal(x, y), '%s: %s differs in %d of %d elements' % (what, k, int((x != y).sum()), x.size)


def unchanged(g, host, what):
    """The buffer still holds `host` (its initial contents), bit for bit, between intact guards."""
    assert g.guards_ok(), what + ': written outside the buffer'
    want = torch.as_tensor(np.ascontiguousarray(host).reshape(-1)).to(g.t.dtype).numpy()
    kind = np.uint32 if want.dtype == np.float32 else np.uint64
    assert np.array_equal(g.get().view(kind), want.view(kind)), what + ': changed'


def proj_close(got, ref, tol, what):
    ref = np.asarray(ref, np.float64)
    lim_close(got, ref, tol * (1 + np.abs(ref).max()), what)


def sync_ok(bufs):
    torch.cuda.synchronize()
    for k, g in bufs.items():
        assert g.guards_ok(), k + ': written outside the buffer'


# ---------------------------------------------------------------------------------------------------- BatchNorm side
BN_RECS = [(16, 1, 1, 1), (64, 3, 4, 4), (200, 8, 8, 8), (256, 16, 32, 32), (32, 8, 4, 4)]       # C, nslot, H, W
BN_SKIP = 4                                            # the record with gamma_goff = -1
# constant channels of record 2 (beyond the block's 128 threads) and their large values: sum x^2 / N - mean^2 cancels
# to rounding noise, zero or NEGATIVE (about -1e-10; bn_data asserts that negative values occur).  Their moving variance
# starts at exactly 0.0, so that decay * 0 + (1 - decay) * (float)var is negative unless the kernel clamps var at 0.
BN_CONST = (2, list(range(136, 144)), np.float32([1000.1, 999.7, 1234.5, 1000.0, 873.3, 1500.9, 1023.99, 1111.1]))
_bn = None


def bn_data():
    """The five BatchNorms: activations, upstream gradients, state, the float64 reference and the slot sums.  Once."""
    global _bn
    if _bn is None:
        rng = np.random.default_rng(77)
        _bn = []
        for k, (Cc, ns, H, W) in enumerate(BN_RECS):
            x = (rng.standard_normal((N_IMG, H, W, Cc)) * rng.uniform(0.5, 2, Cc) + rng.standard_normal(Cc)).astype(np.float32)
            if k == BN_CONST[0]:
                x[..., BN_CONST[1]] = BN_CONST[2]
            dz = rng.standard_normal(x.shape).astype(np.float32)
            gamma, beta = rng.uniform(0.5, 1.5, Cc).astype(np.float32), (rng.standard_normal(Cc) * 0.3).astype(np.float32)
            m0, v0 = rng.standard_normal(Cc).astype(np.float32), rng.uniform(0.5, 2, Cc).astype(np.float32)
            if k == BN_CONST[0]:
                v0[BN_CONST[1]] = 0.0
            ref = R.bn_finalize_ref(x, dz, gamma.astype(np.float64), m0, v0, DECAY, EPS)
            sums, reds = R.spread_slots(x, dz, ref['xhat'], ns, rng)
            d64 = dz.astype(np.float64).reshape(-1, Cc)
            _bn.append(dict(C=Cc, nslot=ns, px=H * W, gamma=gamma, beta=beta, m0=m0, v0=v0, ref=ref, sums=sums, reds=reds,
                            abs_b=np.abs(d64).sum(0), abs_g=np.abs(d64 * ref['xhat'].reshape(-1, Cc)).sum(0)))
        # the constant channels: the two terms of sum x^2 / N - mean^2 agree to rounding; the exact variance is 0
        r = _bn[BN_CONST[0]]
        assert (r['ref']['var'][BN_CONST[1]] < 1e-20).all()
        # ... and the kernel's own fp64 arithmetic (slots ascending from 0.0, times 1 / N) goes below zero on some of them,
        # whether or not the compiler contracts s2 * inv - mean * mean into an fma: without the clamp those fail
        from fractions import Fraction
        inv, raw, raw_fma = 1.0 / (N_IMG * r['px']), [], []
        for c in BN_CONST[1]:
            s1 = s2 = 0.0
            for s in range(r['nslot']):
                s1, s2 = s1 + r['sums'][s, c], s2 + r['sums'][s, r['C'] + c]
            mean = s1 * inv
            raw.append(s2 * inv - mean * mean)
            raw_fma.append(float(Fraction(s2 * inv) - Fraction(mean) * Fraction(mean)))
        r['raw_var'] = np.array(raw)
        assert ((r['raw_var'] < 0) & (np.array(raw_fma) < 0)).any(), (raw, raw_fma)
    return _bn


class BnSide:
    """The records' places in sums / reds / sums_keep (doubles), state and grads (floats): non-zero, non-adjacent
    offsets, the sentinel between them and in the slots a record does not use."""

    def __init__(self, gstart):
        self.recs = bn_data()
        soff, stoff, goff = 6, 5, gstart
        self.rows, self.table = [], []
        for k, r in enumerate(self.recs):
            Cc = r['C']
            row = dict(sum=soff, m=stoff, v=stoff + Cc + 3, g=goff, b=goff + Cc + 2)
            self.rows.append(row)
            self.table += [row['sum'], row['m'], row['v'], Cc, r['px'], -1 if k == BN_SKIP else row['g'], row['b'], r['nslot']]
            soff += R.BN_SLOTS * 2 * Cc + 10
            stoff += 2 * Cc + 3 + 7
            goff += 2 * Cc + 2 + 5
        self.n_sum, self.n_state, self.gend = soff, stoff, goff
        self.sums = np.full(self.n_sum, SENTINEL)
        self.reds = np.full(self.n_sum, SENTINEL)
        self.used = np.zeros(self.n_sum, bool)
        self.state = np.full(self.n_state, SENT32)
        for r, row in zip(self.recs, self.rows):
            n = r['nslot'] * 2 * r['C']
            self.sums[row['sum']:row['sum'] + n] = r['sums'].reshape(-1)
            self.reds[row['sum']:row['sum'] + n] = r['reds'].reshape(-1)
            self.used[row['sum']:row['sum'] + n] = True
            self.state[row['m']:row['m'] + r['C']] = r['m0']
            self.state[row['v']:row['v'] + r['C']] = r['v0']
        self.tab_d = itab(self.table)

    def upload(self):
        return dict(sums=up(self.sums, torch.float64), reds=up(self.reds, torch.float64),
                    keep=up(np.full(self.n_sum, SENTINEL), torch.float64), state=up(self.state))

    def check(self, b, grads, ran=True, reds_on=True, keep=False, tag=''):
        """State, gradients and the slot arenas after a launch (ran = False: the launch had no BatchNorm)."""
        state = b['state'].get()
        if not ran:
            unchanged(b['state'], self.state, tag + 'state')
        acc = {k: ([], [], []) for k in ('moving mean', 'moving variance', 'dbeta', 'dgamma')}

        def add(key, got, ref, lim):
            for lst, v in zip(acc[key], (got, ref, lim)):
                lst.append(np.broadcast_to(np.asarray(v, np.float64), np.shape(ref)))
        touched = np.zeros(self.n_state, bool)
        for k, (r, row) in enumerate(zip(self.recs, self.rows)):
            Cc, ref = r['C'], r['ref']
            m, v = state[row['m']:row['m'] + Cc], state[row['v']:row['v'] + Cc]
            gb, gg = grads[row['b']:row['b'] + Cc], grads[row['g']:row['g'] + Cc]
            touched[row['m']:row['m'] + Cc] = touched[row['v']:row['v'] + Cc] = True
            if k == BN_SKIP or not ran:              # nobody consumes its output: averages and gradients keep their bits
                assert np.array_equal(m.view(np.uint32), r['m0'].view(np.uint32)), tag + 'moving mean of a skipped record'
                assert np.array_equal(v.view(np.uint32), r['v0'].view(np.uint32)), tag + 'moving variance of a skipped record'
                assert (gb == SENT32).all() and (gg == SENT32).all(), tag + 'gradients of a skipped record'
                continue
            add('moving mean', m, ref['m_avg'], 1e-6 * (1 + np.abs(ref['m_avg']).max()))
            add('moving variance', v, ref['v_avg'], 1e-6 * (1 + np.abs(ref['v_avg']).max()))
            if reds_on:
                tiny = np.finfo(np.float64).tiny         # (a constant channel: xhat, dgamma and its limit are exactly 0)
                add('dbeta', gb, ref['dbeta'], ULP * np.abs(ref['dbeta']) + 2.0 ** -48 * r['abs_b'] + tiny)
                add('dgamma', gg, ref['dgamma'], ULP * np.abs(ref['dgamma']) + 2.0 ** -48 * r['abs_g'] + tiny)
            else:
                assert (gb == SENT32).all() and (gg == SENT32).all(), tag + 'gradients without reductions'
            if k == BN_CONST[0]:                     # the variance clamp
                vc = v[BN_CONST[1]]                  # from 0.0: (1 - decay) * max(var, 0), i.e. +0.0 or a positive 1e-11
                assert np.isfinite(vc).all() and (vc >= 0.0).all() and not np.signbit(vc).any() and (vc <= 1e-6).all(), (tag, vc)
        if ran:
            assert np.isfinite(state[touched]).all(), tag + 'a moving average that is not finite'
            for k, (r, row) in enumerate(zip(self.recs, self.rows)):
                assert (state[row['v']:row['v'] + r['C']] >= 0).all(), tag + 'a negative moving variance'
            for key, (g, f, l) in acc.items():
                if g:
                    lim_close(np.concatenate(g), np.concatenate(f), np.concatenate(l), tag + key)
        assert (state[~touched] == SENT32).all(), tag + 'state between the records'
        # the slot arenas
        if keep and ran:
            unchanged(b['keep'], np.where(self.used, self.sums, SENTINEL), tag + 'sums_keep (the old sums in the used slots)')
            unchanged(b['sums'], np.where(self.used, 0.0, SENTINEL), tag + 'sums (cleared in the used slots)')
            unchanged(b['reds'], np.where(self.used, 0.0, SENTINEL) if reds_on else self.reds, tag + 'reds')
        else:
            unchanged(b['keep'], np.full(self.n_sum, SENTINEL), tag + 'sums_keep')
            unchanged(b['sums'], self.sums, tag + 'sums')
            unchanged(b['reds'], self.reds, tag + 'reds')


def bn_grads_gaps_ok(side, grads, lo):
    """grads[lo:] outside the records' gamma / beta ranges still holds the sentinel."""
    inside = np.zeros(side.gend, bool)
    for r, row in zip(side.recs, side.rows):
        inside[row['g']:row['g'] + r['C']] = inside[row['b']:row['b'] + r['C']] = True
    assert (grads[lo:][~inside[lo:]] == SENT32).all(), 'grads between the records'


@pytest.mark.parametrize('form', ['plain', 'keep', 'no_reds', 'no_reds_keep'])
def test_bn_finalize_alone(form):
    lib = _hip.load()
    side = BnSide(gstart=9)
    b = side.upload()
    b['grads'] = up(np.full(side.gend, SENT32))
    keep, reds_on = form.endswith('keep'), not form.startswith('no_reds')
    _hip.check(lib.mpnn_bn_finalize(b['sums'].ptr(), b['reds'].ptr() if reds_on else None, b['state'].ptr(), b['grads'].ptr(),
                                    side.tab_d.data_ptr(), len(BN_RECS), DECAY, N_IMG, b['keep'].ptr() if keep else None,
                                    stream()), 'bn_finalize')
    sync_ok(b)
    grads = b['grads'].get()
    side.check(b, grads, reds_on=reds_on, keep=keep, tag=form + ': ')
    bn_grads_gaps_ok(side, grads, 0)


# ---------------------------------------------------------------------------------------------------- slabs
class SlabSide:
    """Tensors summed over `split` slabs, as tests/test_hip_conv.py::test_slab_reduce_items_and_groups: item sizes of
    _hip.slab_item_size, ragged last items, one tensor off the 16-byte grid (the scalar path), one cut into 64s."""

    def __init__(self, split, seed):
        rng = np.random.default_rng(seed)
        sizes = [1024 * 3 + 20, 433, 7, 64]
        self.split, self.stride = split, (sum(sizes) + 5 + 3) // 4 * 4
        self.slab = rng.standard_normal(split * self.stride).astype(np.float32)
        tab, off, self.want = [], 4, []
        for ti, sz in enumerate(sizes):
            if ti == 2:
                off += 1
            item = _hip.slab_item_size(split) if ti != 3 else 64
            for k in range(0, sz, item):
                tab += [off + k, off + k, min(item, sz - k), split, self.stride, 0]
            self.want.append((off, sz))
            off += sz
        assert off <= self.stride
        self.n_items = len(tab) // 6
        self.tab_d, self.slab_d = itab(tab), dev(self.slab)
        self.ref = self.slab.astype(np.float64).reshape(split, self.stride).sum(0)

    def check(self, grads, ran=True):
        mask = np.zeros(self.stride, bool)
        for o, sz in self.want:
            mask[o:o + sz] = True
            if ran:
                proj_close(grads[o:o + sz], self.ref[o:o + sz], 2e-6 * np.sqrt(self.split), 'slab sums at %d' % o)
        assert (grads[:self.stride][~mask if ran else slice(None)] == SENT32).all(), 'grads outside the summed tensors'


@pytest.mark.parametrize('what', ['both', 'bn_only', 'slabs_only'])
@pytest.mark.parametrize('split', [3, 17])
def test_backward_finish_is_its_two_launches(split, what):
    lib = _hip.load()
    slabs = SlabSide(split, seed=split)
    side = BnSide(gstart=slabs.stride + 8)
    n_items, n_bn = (0 if what == 'bn_only' else slabs.n_items), (0 if what == 'slabs_only' else len(BN_RECS))
    keep = what == 'both'
    runs = []
    for fused in (True, False):
        b = side.upload()
        b['grads'] = up(np.full(side.gend, SENT32))
        kp = b['keep'].ptr() if keep else None
        bn_args = (b['sums'].ptr(), b['reds'].ptr(), b['state'].ptr())
        if fused:
            _hip.check(lib.mpnn_backward_finish(slabs.slab_d.data_ptr(), b['grads'].ptr(), slabs.tab_d.data_ptr(), n_items,
                                                *bn_args, side.tab_d.data_ptr(), n_bn, DECAY, N_IMG, kp, stream()), 'backward_finish')
        else:
            _hip.check(lib.mpnn_slab_reduce(slabs.slab_d.data_ptr(), b['grads'].ptr(), slabs.tab_d.data_ptr(), n_items, stream()), 'slab_reduce')
            _hip.check(lib.mpnn_bn_finalize(*bn_args, b['grads'].ptr(), side.tab_d.data_ptr(), n_bn, DECAY, N_IMG, kp, stream()), 'bn_finalize')
        sync_ok(b)
        runs.append(b)
    same_bits(runs[0], runs[1], 'mpnn_backward_finish against mpnn_slab_reduce + mpnn_bn_finalize')
    grads = runs[0]['grads'].get()
    slabs.check(grads, ran=n_items > 0)
    side.check(runs[0], grads, ran=n_bn > 0, keep=keep, tag='%s, split %d: ' % (what, split))
    bn_grads_gaps_ok(side, grads, slabs.stride)


# ---------------------------------------------------------------------------------------------------- optimizer + packs
def opt_common(rng):
    p = rng.random((N_NODES, N_STAT)) * 0.9 + 0.01
    stat = np.stack([p.sum(1), (p ** 2).sum(1)], 1).astype(np.float32)
    hyp = np.zeros(_hip.HYP_N, np.float32)
    hyp[_hip.HYP_LR], hyp[_hip.HYP_MU], hyp[_hip.HYP_ARTR] = LR, MU, ARTR
    eq = rng.standard_normal(R.EQ_OFF + 2304 + 5).astype(np.float32)
    return stat, hyp, eq


def fill_tensors(rng, tensors, size):
    """(params, accum, grads, mask of the tensors' elements): random inside the tensors, the sentinel between them."""
    arrs = [np.full(size, SENT32) for _ in range(3)]
    mask = np.zeros(size, bool)
    for t in tensors:
        sl = slice(t['off'], t['off'] + t['size'])
        mask[sl] = True
        for a, scale in zip(arrs, (0.2, 0.1, 1.0)):
            a[sl] = (rng.standard_normal(t['size']) * scale).astype(np.float32)
    return arrs + [mask]


def pack_desc(tensors):
    return [v for t in tensors if t['cin'] for v in (t['off'], t['fwd'], t['bwd'], t['cin'], t['cout'], 0)]


def pack_into(params_g, ksize, desc_d, n):
    """mpnn_pack_weights of the parameters in a Guarded buffer, into a fresh Guarded buffer."""
    packs = Guarded(max(ksize, 1))
    if n:
        _hip.check(_hip.load().mpnn_pack_weights(params_g.ptr(), packs.ptr(), desc_d.data_ptr(), n, stream()), 'pack_weights')
    torch.cuda.synchronize()
    return packs


def check_packs(packs, params_g, tensors, ksize, desc_d, what):
    """packs == mpnn_pack_weights(the updated parameters), whole buffer; and == the documented layout (pad lanes +0.0)."""
    assert packs.guards_ok(), what + ': written outside the packs'
    fresh = pack_into(params_g, ksize, desc_d, len(pack_desc(tensors)) // 6)
    assert torch.equal(packs.buf, fresh.buf) and np.array_equal(bits(packs), bits(fresh)), what + ': packs != mpnn_pack_weights(params)'
    P, K = params_g.get(), packs.get()
    for t in tensors:
        if not t['cin']:
            continue
        fw, bw = R.pack_ref(P[t['off']:t['off'] + t['size']].reshape(3, 3, t['cin'], t['cout']))
        assert np.array_equal(K[t['fwd']:t['fwd'] + fw.size].view(np.uint32), fw.reshape(-1).view(np.uint32)), (what, t['name'], 'forward pack')
        if t['bwd'] >= 0:
            assert np.array_equal(K[t['bwd']:t['bwd'] + bw.size].view(np.uint32), bw.reshape(-1).view(np.uint32)), (what, t['name'], 'backward pack')


_opt = None


def opt_data():
    global _opt
    if _opt is None:
        rng = np.random.default_rng(31)
        tensors, psize, ksize = R.opt_layout()
        P, A, G, mask = fill_tensors(rng, tensors, psize)
        stat, hyp, eq = opt_common(rng)
        _opt = dict(tensors=tensors, psize=psize, ksize=ksize, P=P, A=A, G=G, mask=mask, stat=stat, hyp=hyp, eq=eq,
                    rows={k: R.opt_rows(v, tensors) for k, v in R.OPT_LISTS.items()},
                    dev=dict(stat=dev(stat), hyp=dev(hyp), eq=dev(eq), desc=itab(pack_desc(tensors)), G=dev(G)))
    return _opt


@pytest.mark.parametrize('talr', [0, 1])
@pytest.mark.parametrize('lst', list(R.OPT_LISTS))
def test_optimizer_emits_the_packs(lst, talr):
    lib = _hip.load()
    d = opt_data()
    # a condition on the inputs, not a measurement: every emission path is taken by at least 10 work items of the lists
    total = {k: sum(R.path_counts(rows)[k] for rows in d['rows'].values()) for k in ('tap', 'taps', 'slow')}
    assert min(total.values()) >= 10, total
    rows, dd = d['rows'][lst], d['dev']
    inv_n, gs = 1.0 / (2 * N_STAT), 0.5                        # (sums over two replicas' batches, as after an all-reduce)
    b = dict(params=up(d['P']), accum=up(d['A']))
    b['packs'] = pack_into(b['params'], d['ksize'], dd['desc'], len(pack_desc(d['tensors'])) // 6)
    seg = itab(rows)
    _hip.check(lib.mpnn_talr_momentum_step(b['params'].ptr(), b['accum'].ptr(), dd['G'].data_ptr(), seg.data_ptr(), len(rows),
                                           dd['stat'].data_ptr(), dd['hyp'].data_ptr(), talr, inv_n, gs, dd['eq'].data_ptr(),
                                           b['packs'].ptr(), stream()), 'talr_momentum_step')
    sync_ok(b)
    want_P, want_A = R.talr_ref(d['P'], d['A'], d['G'], R.items_of(rows), d['stat'], LR, MU, ARTR, talr, inv_n, gs, d['eq'])
    P, A, m = b['params'].get(), b['accum'].get(), d['mask']
    proj_close(A[m], want_A[m], 1e-6, '%s talr %d: accumulators' % (lst, talr))
    proj_close(P[m], want_P[m], 1e-6, '%s talr %d: parameters' % (lst, talr))
    assert (P[~m] == SENT32).all() and (A[~m] == SENT32).all(), 'written between the tensors'
    check_packs(b['packs'], b['params'], d['tensors'], d['ksize'], dd['desc'], '%s talr %d' % (lst, talr))


# ---------------------------------------------------------------------------------------------------- the fused step end
FIN_TENSORS = [t for t in R.OPT_TENSORS if t[0] not in ('c16x128', 'c128x128')]


class StepEnd:
    """One net's end of step: conv tensors summed from slabs (items = True) or with final gradients, the five BatchNorms
    with gamma / beta in the parameter arena (bn = True), and the other tensors as plain optimizer items."""

    def __init__(self, seed, splits, items=True, bn=True, plain=True):
        rng = np.random.default_rng(seed)
        self.tensors, tend, self.ksize = R.opt_layout(FIN_TENSORS)
        self.side = BnSide(gstart=tend)
        self.psize = self.side.gend
        self.stride = (self.psize + 3) // 4 * 4
        self.P, self.A, self.G, self.mask = fill_tensors(rng, self.tensors, self.psize)
        self.stat, self.hyp, self.eq = opt_common(rng)
        slab_tab, self.item_rows, self.plain_rows, self.summed = [], [], [], []
        k = 0
        for t in self.tensors:
            if t['cin'] and items:
                split = splits[k % len(splits)]
                k += 1
                item = _hip.slab_item_size(split)
                self.item_rows += R.seg_rows(t, item)
                for s in range(0, t['size'], item):
                    slab_tab += [t['off'] + s, t['off'] + s, min(item, t['size'] - s), split, self.stride, 0]
                self.summed.append((t, split))
                self.G[t['off']:t['off'] + t['size']] = SENT32          # written by the reduction
            elif t['cin'] or plain:
                self.plain_rows += R.seg_rows(t, 2048)
            else:
                self.mask[t['off']:t['off'] + t['size']] = False         # (no work item: stays as it is)
        self.n_items, self.n_plain = len(self.item_rows), len(self.plain_rows)
        assert items or not self.n_items
        self.slab = rng.standard_normal(max(splits) * self.stride).astype(np.float32) if items else np.zeros(4, np.float32)
        # BatchNorms: gamma / beta are parameters like any other; a record's node and L2 factors in bn_opt
        self.n_bn = len(BN_RECS) if bn else 0
        self.bn_opt, self.bn_rows = [], []
        for kk, (r, row) in enumerate(zip(self.side.recs, self.side.rows)):
            Cc, node = r['C'], kk % N_NODES
            l2g, l2b = (1e-4 if kk == 1 else 0.0), (2e-4 if kk == 2 else 0.0)
            self.bn_opt += [node, R.l2_bits(l2g), R.l2_bits(l2b), 0]
            for off, v in ((row['g'], r['gamma']), (row['b'], r['beta'])):
                self.P[off:off + Cc] = v
                self.A[off:off + Cc] = (rng.standard_normal(Cc) * 0.1).astype(np.float32)
            if kk != BN_SKIP and bn:
                self.bn_rows.append([row['b'], Cc, node, 0, R.l2_bits(l2b), -1, 0, 0, 0, -1, -1, 0])
                self.bn_rows.append([row['g'], Cc, node, 0, R.l2_bits(l2g), -1, 0, 0, 0, -1, -1, 0])
                self.mask[row['g']:row['g'] + Cc] = self.mask[row['b']:row['b'] + Cc] = True
        self.ro = dict(slab=dev(self.slab), slab_tab=itab(slab_tab), item_seg=itab(self.item_rows), plain_seg=itab(self.plain_rows),
                       bn_opt=itab(self.bn_opt), stat=dev(self.stat), hyp=dev(self.hyp), eq=dev(self.eq),
                       desc=itab(pack_desc(self.tensors)), all_seg=itab(self.item_rows + self.bn_rows + self.plain_rows))
        self.n_desc = len(pack_desc(self.tensors)) // 6
        self.inv_n = 1.0 / N_STAT

    def upload(self):
        b = self.side.upload()
        b.update(params=up(self.P), accum=up(self.A), grads=up(self.G))
        b['packs'] = pack_into(b['params'], self.ksize, self.ro['desc'], self.n_desc)
        return b

    def record(self, b, talr, gs):
        ro, f = self.ro, _hip.FinishNet()
        f.slabs, f.slab_table, f.n_items, f.item_seg = ro['slab'].data_ptr(), ro['slab_tab'].data_ptr(), self.n_items, ro['item_seg'].data_ptr()
        f.sums, f.reds, f.state, f.bn_table = b['sums'].ptr(), b['reds'].ptr(), b['state'].ptr(), self.side.tab_d.data_ptr()
        f.n_bn, f.bn_opt, f.n_img, f.sums_keep = self.n_bn, ro['bn_opt'].data_ptr(), N_IMG, b['keep'].ptr()
        f.params, f.accum, f.grads = b['params'].ptr(), b['accum'].ptr(), b['grads'].ptr()
        f.node_stat, f.hyp, f.talr, f.inv_n, f.grad_scale = ro['stat'].data_ptr(), ro['hyp'].data_ptr(), talr, self.inv_n, gs
        f.w_eq, f.packs, f.plain_seg, f.n_plain = ro['eq'].data_ptr(), b['packs'].ptr(), ro['plain_seg'].data_ptr(), self.n_plain
        return f

    def fused(self, b, talr, gs):
        f = self.record(b, talr, gs)
        _hip.check(_hip.load().mpnn_backward_finish_opt(
            f.slabs, f.slab_table, f.n_items, f.item_seg, f.sums, f.reds, f.state, f.bn_table, f.n_bn, f.bn_opt, DECAY, f.n_img,
            f.sums_keep, f.params, f.accum, f.grads, f.node_stat, f.hyp, f.talr, f.inv_n, f.grad_scale, f.w_eq, f.packs,
            f.plain_seg, f.n_plain, stream()), 'backward_finish_opt')

    def composed(self, b, talr, gs):
        lib, ro = _hip.load(), self.ro
        _hip.check(lib.mpnn_slab_reduce(ro['slab'].data_ptr(), b['grads'].ptr(), ro['slab_tab'].data_ptr(), self.n_items, stream()), 'slab_reduce')
        _hip.check(lib.mpnn_bn_finalize(b['sums'].ptr(), b['reds'].ptr(), b['state'].ptr(), b['grads'].ptr(), self.side.tab_d.data_ptr(),
                                        self.n_bn, DECAY, N_IMG, b['keep'].ptr(), stream()), 'bn_finalize')
        n_seg = self.n_items + len(self.bn_rows) + self.n_plain
        _hip.check(lib.mpnn_talr_momentum_step(b['params'].ptr(), b['accum'].ptr(), b['grads'].ptr(), ro['all_seg'].data_ptr(), n_seg,
                                               ro['stat'].data_ptr(), ro['hyp'].data_ptr(), talr, self.inv_n, gs, ro['eq'].data_ptr(),
                                               b['packs'].ptr(), stream()), 'talr_momentum_step')

    def check(self, b, talr, gs, tag):
        """The result against float64: the gradients (slab sums; dgamma / dbeta), then the update of exactly those."""
        grads = b['grads'].get()
        for t, split in self.summed:
            ref = self.slab.reshape(-1, self.stride)[:split, t['off']:t['off'] + t['size']].astype(np.float64).sum(0)
            proj_close(grads[t['off']:t['off'] + t['size']], ref, 2e-6 * np.sqrt(split), tag + 'slab sums of ' + t['name'])
        self.side.check(b, grads, ran=self.n_bn > 0, keep=True, tag=tag)
        rows = self.item_rows + self.bn_rows + self.plain_rows
        want_P, want_A = R.talr_ref(self.P, self.A, grads, R.items_of(rows), self.stat, LR, MU, ARTR, talr, self.inv_n, gs, self.eq)
        P, A, m = b['params'].get(), b['accum'].get(), self.mask
        proj_close(A[m], want_A[m], 1e-6, tag + 'accumulators')
        proj_close(P[m], want_P[m], 1e-6, tag + 'parameters')
        for name, got, host in (('params', P, self.P), ('accum', A, self.A)):
            assert np.array_equal(got[~m].view(np.uint32), host[~m].view(np.uint32)), tag + name + ' without a work item changed'
        check_packs(b['packs'], b['params'], self.tensors, self.ksize, self.ro['desc'], tag)


_fin = {}


def step_end(key, *a, **kw):
    if key not in _fin:
        _fin[key] = StepEnd(*a, **kw)
    return _fin[key]


@pytest.mark.parametrize('gs', [1.0, 0.5])
@pytest.mark.parametrize('talr', [0, 1])
def test_backward_finish_opt_is_its_three_launches(talr, gs):
    net = step_end('one', 5, [3, 17, 40, 256])
    assert net.n_items and net.n_bn and net.n_plain and any(r[3] for r in net.plain_rows)       # (a router item among the plain ones)
    assert {R.seg_path(r) for r in net.item_rows} == {'tap', 'taps', 'slow'}
    runs = []
    for run in (net.fused, net.composed):
        b = net.upload()
        run(b, talr, gs)
        sync_ok(b)
        runs.append(b)
    same_bits(runs[0], runs[1], 'mpnn_backward_finish_opt against its three launches')
    net.check(runs[0], talr, gs, 'fused, talr %d, grad_scale %g: ' % (talr, gs))


def test_backward_finish_opt_multi_is_three_single_launches():
    lib = _hip.load()
    nets = [step_end('m0', 11, [3, 17]), step_end('m1', 12, [3], items=False), step_end('m2', 13, [17, 3], bn=False, plain=False)]
    shapes = [(n.n_items, n.n_bn, n.n_plain) for n in nets]
    assert nets[1].n_items == 0 and nets[2].n_bn == 0 and len({sum(s) for s in shapes}) == 3, shapes
    cfg = [(1, 0.5), (0, 1.0), (1, 1.0)]                        # (talr, grad_scale) per net
    single = []
    for net, (talr, gs) in zip(nets, cfg):
        b = net.upload()
        net.fused(b, talr, gs)
        sync_ok(b)
        single.append(b)
    multi = [net.upload() for net in nets]
    recs = [net.record(b, talr, gs) for net, b, (talr, gs) in zip(nets, multi, cfg)]
    host = (_hip.FinishNet * len(recs))(*recs)
    tab = _hip.to_device_table(recs, DEV)
    _hip.check(lib.mpnn_backward_finish_opt_multi(host, tab.data_ptr(), len(recs), DECAY, stream()), 'backward_finish_opt_multi')
    for k, (net, b, (talr, gs)) in enumerate(zip(nets, multi, cfg)):
        sync_ok(b)
        same_bits(b, single[k], 'net %d of mpnn_backward_finish_opt_multi against its own launch' % k)
        net.check(b, talr, gs, 'multi, net %d: ' % k)
