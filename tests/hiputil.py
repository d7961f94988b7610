"""Thin numpy-in / numpy-out drivers of the C-ABI entry points, for the parity tests."""
import ctypes as C

import numpy as np
import torch

from lib import _hip
from oracle import np_ops as O

DEV = 'cuda:0'


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack_sizes(cin, cout):
    return 9 * ((cin + 15) // 16) * 16 * cout, 9 * ((cout + 15) // 16) * 16 * cin


def pack_weights(ws, want_bwd=True):
    """ws: list of HWIO float arrays.  Returns (list of fwd packs, list of bwd packs) as device tensors."""
    lib = _hip.load()
    flat = np.concatenate([w.reshape(-1) for w in ws]).astype(np.float32)
    desc, off, poff = [], 0, 0
    spans = []
    for w in ws:
        _, _, ci, co = w.shape
        fs, bs = pack_sizes(ci, co)
        has_b = want_bwd and ci % 16 == 0
        desc += [off, poff, poff + fs if has_b else -1, ci, co, 0]
        spans.append((poff, fs, poff + fs, bs if has_b else 0))
        off += w.size
        poff += fs + (bs if has_b else 0)
    params, packs = dev(flat), torch.zeros(poff, device=DEV)
    d = dev(np.array(desc, np.int32), torch.int32)
    _hip.check(lib.mpnn_pack_weights(params.data_ptr(), packs.data_ptr(), d.data_ptr(), len(ws), stream()), 'pack')
    torch.cuda.synchronize()
    return ([packs[a:a + n] for a, n, _, _ in spans], [packs[b:b + m] if m else None for _, _, b, m in spans])


def slots(v):
    """A statistics vector [2C] spread (unevenly, on purpose) over the [SLOTS][2C] layout."""
    v = np.asarray(v, np.float64)
    out = np.zeros((_hip.BN_SLOTS, v.size))
    w = np.random.default_rng(7).random(_hip.BN_SLOTS); w /= w.sum()
    out[:] = w[:, None] * v[None, :]
    out[0] += v - out.sum(0)
    return out


def unslot(t, c2):
    return t.cpu().numpy().reshape(_hip.BN_SLOTS, c2).sum(0)


def bn_dict(x, gamma, beta, m_avg=None, v_avg=None, eps=1e-6):
    """Device BatchNorm context for pre-BN array x (statistics over all leading dims)."""
    c = x.shape[-1]
    x64 = np.asarray(x, np.float64).reshape(-1, c)
    sums = slots(np.concatenate([x64.sum(0), (x64 ** 2).sum(0)]))
    d = dict(sum=dev(sums, torch.float64), gamma=dev(gamma), beta=dev(beta),
             m_avg=dev(np.zeros(c) if m_avg is None else m_avg),
             v_avg=dev(np.ones(c) if v_avg is None else v_avg), eps=eps)
    return d, x64.shape[0]


def pool2_np(v):
    n, h, w, c = v.shape
    return np.ascontiguousarray(v.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4)))


def conv_fwd(x, wh, b, v=None, wv=None, bn=None, mode=_hip.ACT_IDENTITY, shift=0, bn_cnt=1, want_pool=False, group=False):
    """x: [n, H<<shift, W<<shift, Ca]; v: the UNPOOLED finer map [n, 2H, 2W, Cv] (pooled here, as its
    producer would).  Returns (out, out_sum[, pooled out])."""
    if v is not None:
        v = pool2_np(np.asarray(v, np.float32))
    lib = _hip.load()
    n = x.shape[0]
    H, W = x.shape[1] >> shift, x.shape[2] >> shift
    co = wh.shape[3]
    fw, _ = pack_weights([wh] + ([wv] if wv is not None else []), want_bwd=False)
    xd, vd, bd = dev(x), dev(v), dev(b)
    out = torch.empty((n, H, W, co), device=DEV)
    osum = torch.zeros(_hip.BN_SLOTS * 2 * co, device=DEV, dtype=torch.float64)
    a = _hip.ConvFwdArgs()
    a.a = _hip.act(xd, x.shape[3], mode, shift, bn, bn_cnt)
    a.v = _hip.ptr(vd); a.Cv = v.shape[3] if v is not None else 0
    a.wa_pack = fw[0].data_ptr(); a.wv_pack = fw[1].data_ptr() if wv is not None else None
    a.bias = bd.data_ptr(); a.out = out.data_ptr(); a.out_sum = osum.data_ptr(); a.out_nslot = _hip.BN_SLOTS
    pool = torch.full((n, H // 2, W // 2, co), 9.0, device=DEV) if want_pool else None
    a.pool_out = _hip.ptr(pool)
    a.n, a.H, a.W, a.Cout = n, H, W, co
    if group:            # the same conv as a one-member wavefront group (device table; K-split body on deep small maps)
        arr = (_hip.ConvFwdArgs * 1)(a)
        tab = _hip.to_device_table([a], DEV)
        _hip.check(lib.mpnn_msconv_fwd_group(arr, tab.data_ptr(), 1, stream()), 'msconv_fwd_group')
    else:
        _hip.check(lib.mpnn_msconv_fwd(C.byref(a), stream()), 'msconv_fwd')
    torch.cuda.synchronize()
    if want_pool:
        return out.cpu().numpy(), unslot(osum, 2 * co), pool.cpu().numpy()
    return out.cpu().numpy(), unslot(osum, 2 * co)


def bn_ctx(s_dev, C_, bn, cnt, mode=_hip.ACT_BN_BATCH, red=None):
    ctx = _hip.BnCtx()
    ctx.s = s_dev.data_ptr()
    ctx.bn = _hip.act(None, C_, mode, 0, bn, cnt)
    ctx.red = _hip.ptr(red)
    ctx.red_nslot = _hip.BN_SLOTS
    return ctx


def dgrad_horz(g, w, s_prev=None, bn=None, cnt=1, extra=None):
    """g: [n,H,W,Cout_fwd]; w: HWIO [3,3,Cin,Cout_fwd].  Returns (out, red) ; red None if raw."""
    lib = _hip.load()
    n, H, W, cg = g.shape
    ci = w.shape[2]
    _, bw = pack_weights([w])
    gd, ed = dev(g), dev(extra)
    out = torch.empty((n, H, W, ci), device=DEV)
    a = _hip.DgradHorzArgs()
    a.g = gd.data_ptr(); a.Cg = cg; a.w_pack = bw[0].data_ptr(); a.dy_extra = _hip.ptr(ed)
    a.out = out.data_ptr(); a.n, a.H, a.W, a.Cout = n, H, W, ci
    red = None
    keep = []
    if s_prev is not None:
        sd = dev(s_prev)
        red = torch.zeros(_hip.BN_SLOTS * 2 * ci, device=DEV, dtype=torch.float64)
        ctx = bn_ctx(sd, ci, bn, cnt)
        keep += [sd, ctx]
        a.prev = C.pointer(ctx); a.red_out = red.data_ptr()
    _hip.check(lib.mpnn_msconv_dgrad_horz(C.byref(a), stream()), 'dgrad_horz')
    torch.cuda.synchronize()
    return out.cpu().numpy(), (None if red is None else unslot(red, 2 * ci))


def dgrad_vert(g, w, s_fine, bn, cnt, dz_fine=None, red=None):
    """g: coarse grad [n,H,W,Cg]; w: HWIO [3,3,Cf,Cg]; s_fine/dz_fine: [n,2H,2W,Cf]."""
    lib = _hip.load()
    n, H, W, cg = g.shape
    cf = w.shape[2]
    _, bw = pack_weights([w])
    gd, sd = dev(g), dev(s_fine)
    buf = dev(dz_fine) if dz_fine is not None else torch.full((n, 2 * H, 2 * W, cf), 7.0, device=DEV)
    redd = dev(slots(red), torch.float64) if red is not None else None
    ctx = bn_ctx(sd, cf, bn, cnt, red=redd)
    a = _hip.DgradVertArgs()
    a.g = gd.data_ptr(); a.Cg = cg; a.w_pack = bw[0].data_ptr(); a.fine = C.pointer(ctx)
    a.fine_has_dz = 1 if dz_fine is not None else 0
    a.dz_g_fine = buf.data_ptr(); a.n, a.H, a.W, a.Cout = n, H, W, cf
    _hip.check(lib.mpnn_msconv_dgrad_vert(C.byref(a), stream()), 'dgrad_vert')
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def wgrad(x, g, v=None, bn=None, mode=_hip.ACT_IDENTITY, shift=0, bn_cnt=1, n_split=7):
    """Partial sums into a slab + mpnn_slab_reduce (n_split > 1) or straight into the gradients."""
    lib = _hip.load()
    if v is not None:
        v = pool2_np(np.asarray(v, np.float32))          # the producer's pooled map
    n = x.shape[0]
    H, W = x.shape[1] >> shift, x.shape[2] >> shift
    ca, co = x.shape[3], g.shape[3]
    cv = v.shape[3] if v is not None else 0
    xd, gd, vd = dev(x), dev(g), dev(v)
    sizes = [9 * ca * co, 9 * cv * co, co]
    offs = [0, sizes[0], sizes[0] + sizes[1]]
    total = sum(sizes)
    stride = (total + 3) // 4 * 4
    n_split = max(1, min(n_split, lib.mpnn_wgrad_tiles(n, H, W)))
    grads = torch.full((total,), 3.0, device=DEV)          # poison: every element must be written
    slab = grads if n_split == 1 else torch.full((n_split * stride,), 5.0, device=DEV)
    a = _hip.WgradArgs()
    a.a = _hip.act(xd, ca, mode, shift, bn, bn_cnt)
    a.v = _hip.ptr(vd); a.Cv = cv
    a.g = gd.data_ptr()
    a.dwa = slab[offs[0]:].data_ptr(); a.dwv = slab[offs[1]:].data_ptr() if cv else None
    a.db = slab[offs[2]:].data_ptr()
    a.split_stride = stride if n_split > 1 else 0
    a.n, a.H, a.W, a.Cout, a.n_split = n, H, W, co, n_split
    _hip.check(lib.mpnn_msconv_wgrad(C.byref(a), stream()), 'wgrad')
    if n_split > 1:
        tab = []
        for o, sz in zip(offs, sizes):
            item = _hip.slab_item_size(n_split)
            for k in range(0, sz, item):
                tab += [o + k, o + k, min(item, sz - k), n_split, stride, 0]
        t = dev(np.array(tab, np.int32), torch.int32)
        _hip.check(lib.mpnn_slab_reduce(slab.data_ptr(), grads.data_ptr(), t.data_ptr(), len(tab) // 6, stream()),
                   'slab_reduce')
    torch.cuda.synchronize()
    out = grads.cpu().numpy()
    dwa = out[:sizes[0]].reshape(3, 3, ca, co)
    dwv = out[offs[1]:offs[2]].reshape(3, 3, cv, co) if cv else None
    return dwa, dwv, out[offs[2]:]


def bn_bwd_reduce(dy, s, bn, cnt):
    lib = _hip.load()
    c = s.shape[-1]
    dyd, sd = dev(dy), dev(s)
    dz = torch.empty_like(dyd)
    red = torch.zeros(_hip.BN_SLOTS * 2 * c, device=DEV, dtype=torch.float64)
    ctx = bn_ctx(sd, c, bn, cnt)
    _hip.check(lib.mpnn_bn_bwd_reduce(dyd.data_ptr(), C.byref(ctx), dz.data_ptr(), red.data_ptr(),
                                      dy.size // c, stream()), 'bn_bwd_reduce')
    torch.cuda.synchronize()
    return dz.cpu().numpy(), unslot(red, 2 * c)


def bn_bwd_apply(dz, s, bn, cnt, red):
    lib = _hip.load()
    c = s.shape[-1]
    dzd, sd, redd = dev(dz), dev(s), dev(slots(red), torch.float64)
    ctx = bn_ctx(sd, c, bn, cnt, red=redd)
    _hip.check(lib.mpnn_bn_bwd_apply(dzd.data_ptr(), C.byref(ctx), dz.size // c, stream()), 'bn_bwd_apply')
    torch.cuda.synchronize()
    return dzd.cpu().numpy()


# ---- backward launches (mpnn_msconv_bwd_level / _rep / _bwd_scale / dgrad_pair) ------------------------------------
# A BwdCase holds the inputs of ONE backward member -- dgrad-horz (optional), dgrad-vert (optional) and the weight
# gradients of one g -- with every output in a Guarded buffer, the C-ABI argument records, and its float64 reference.

RED_RAW = 7.5                      # fill of the red_out that a raw dgrad-horz record carries and must not touch
GUARD = 256                        # elements of each guard region (keeps the 16-byte alignment of the kernels' stores)
SENTINEL = -1.2345678e25


class Guarded:
    """A device buffer of `size` elements between two sentinel guard regions: a kernel that writes outside its
    output changes a guard."""

    def __init__(self, size, dtype=torch.float32):
        self.size = size
        self.buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + size]

    def fill(self, v):
        if np.isscalar(v):
            self.t.fill_(v)
        else:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(v).reshape(-1)).to(DEV, self.t.dtype))

    def ptr(self, off=0):
        return self.t[off:].data_ptr()

    def get(self):
        return self.t.cpu().numpy()

    def guards_ok(self):
        s = torch.tensor(SENTINEL, dtype=self.buf.dtype)
        return bool((self.buf[:GUARD].cpu() == s).all() and (self.buf[GUARD + self.size:].cpu() == s).all())


def f32(a):
    """fp32 values, and the same values exactly in float64 for the oracle."""
    a = np.asarray(a, np.float32)
    return a, a.astype(np.float64)


def slot_spread(v, nslot, rng):
    """[nslot][len(v)] float64 rows (uneven weights) that sum to v."""
    v = np.asarray(v, np.float64)
    w = rng.random(nslot) + 0.1
    out = w[:, None] / w.sum() * v[None, :]
    out[0] += v - out.sum(0)
    return out


def grid_map(rng, shape, grid=2):
    """A map of multiples of 1 / grid in [-1, 1] (exact in fp32): equal values, hence tied 2x2 maxima, are common (five
    values: a good third of the windows; the nine values of a grid of 1/4 give a fifth)."""
    return (rng.integers(-grid, grid + 1, shape) / float(grid)).astype(np.float32)


def tie_stats(s):
    """Of the 2x2 windows of s [n, 2H, 2W, C] (positions 0..3 in row-major window order): the share whose maximum is
    tied, the positions that occur as the FIRST maximum of a tied window, the positions that hold a later, losing copy
    of a tied maximum, and the positions that occur as an untied maximum."""
    n, h, w, c = s.shape
    win = s.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)
    mx = win.max(3, keepdims=True)
    eq = win == mx
    tied = eq.sum(3) > 1
    first = eq.argmax(3)
    later = eq & (np.arange(4)[None, None, None, :, None] != first[:, :, :, None, :])
    return (float(tied.mean()), set(np.unique(first[tied]).tolist()),
            set(np.flatnonzero(later.any((0, 1, 2, 4))).tolist()), set(np.unique(first[~tied]).tolist()))


class BnMap:
    """A pre-BN map s (fp32) with its BatchNorm (batch statistics over nslot slots).  Entries whose fp64 BatchNorm
    output lies within `margin` of zero are drawn again, so that a ReLU mask or a max-pool decision cannot differ
    between the kernel's fp32 arithmetic and the oracle.

    s: the map itself, taken as it is -- NO margin redraw (a grid_map for the max-pool ties of dgrad-vert, which uses
    no ReLU decision of the map).
    mode: 'batch', or the two modes whose coefficients do not come from the batch (bn_coef / the non-batch branches
    beside bn_bwd_row in csrc/common.h and csrc/conv_kernel.h):
      'relu'    MPNN_ACT_RELU: m = 0, rstd = 1, gamma = 1, beta = 0 (gamma / beta / sum are not read): y = s, xhat = s;
      'moving'  MPNN_ACT_BN_MOVING: m = m_avg, rstd = 1 / sqrt(v_avg + eps), the record's gamma and beta (sum is not read).
    In both the backward coefficients of a producer are (m, rstd, gamma * rstd, beta, 0), as under batch statistics, so
    dz = [y > 0] * dy and red_out = [sum dz, sum dz * xhat] with the mode's own y and xhat."""

    def __init__(self, rng, shape, nslot, margin=1e-3, eps=1e-6, mode='batch', s=None):
        c = shape[-1]
        self.gamma, self.gamma64 = f32(rng.uniform(0.5, 1.5, c))
        self.beta, self.beta64 = f32(rng.standard_normal(c) * 0.3)
        self.mode = mode
        m_avg, v_avg = np.zeros(c), np.ones(c)
        if mode == 'relu':
            self.gamma, self.gamma64 = f32(np.ones(c))
            self.beta, self.beta64 = f32(np.zeros(c))
        elif mode == 'moving':
            (m_avg, m64), (v_avg, v64) = f32(rng.standard_normal(c) * 0.2), f32(rng.uniform(0.5, 2.0, c))

        def bn(s64):
            if mode == 'batch':
                return O.bn_train(s64, self.gamma64, self.beta64, eps)
            if mode == 'relu':
                return s64.copy(), np.zeros(c), np.ones(c) - eps
            return self.gamma64 * (s64 - m64) / np.sqrt(v64 + eps) + self.beta64, m64, v64

        fixed = s is not None
        if not fixed:
            s = rng.standard_normal(shape).astype(np.float32)
        while True:
            s64 = s.astype(np.float64)
            y, m, var = bn(s64)
            bad = np.abs(y) < margin
            if fixed or not bad.any():
                break
            s[bad] = rng.standard_normal(int(bad.sum())).astype(np.float32)
        self.s, self.s64, self.y, self.m, self.var = s, s64, y, m, var
        self.xh = (s64 - m) / np.sqrt(var + eps)
        self.rstd = 1.0 / np.sqrt(var + eps)
        self.cnt, self.C, self.nslot, self.eps = s.size // c, c, nslot, eps
        self.act_mode = {'batch': _hip.ACT_BN_BATCH, 'relu': _hip.ACT_RELU, 'moving': _hip.ACT_BN_MOVING}[mode]
        sums = None
        if mode == 'batch':
            x2 = s64.reshape(-1, c)
            sums = dev(slot_spread(np.concatenate([x2.sum(0), (x2 ** 2).sum(0)]), nslot, rng), torch.float64)
        self.dev = dict(sum=sums, gamma=dev(self.gamma), beta=dev(self.beta),
                        m_avg=dev(m_avg), v_avg=dev(v_avg), eps=eps, nslot=nslot)
        self.sd = dev(s)

    def ctx(self, red=None, red_nslot=None):
        """mpnn_bn_ctx; red: float64 [2C] (spread over red_nslot slots) or None."""
        c = _hip.BnCtx()
        c.s = self.sd.data_ptr()
        c.bn = _hip.act(None, self.C, self.act_mode, 0, self.dev, self.cnt)
        self.red_d = None
        if red is not None:
            self.red_d = dev(slot_spread(red, red_nslot, np.random.default_rng(3)), torch.float64)
            c.red = self.red_d.data_ptr()
        c.red_nslot = red_nslot if red_nslot is not None else self.nslot
        return c

    def apply(self, dz, red):
        """mpnn_bn_bwd_apply: gamma * rstd * (dz - red0 / cnt - xhat * red1 / cnt), float64."""
        C_ = self.C
        return self.gamma64 * self.rstd * (dz - red[:C_] / self.cnt - self.xh * red[C_:] / self.cnt)


def red_of(dz, xh):
    c = dz.shape[-1]
    return np.concatenate([dz.reshape(-1, c).sum(0), (dz * xh).reshape(-1, c).sum(0)])


class BwdCase:
    """One backward member.  spec keys:
      n, H, W, Cg           g: [n, H, W, Cg]
      gctx                  None (raw g) or the red_nslot of the BatchNorm context applied while loading g
      horz                  None or dict(Cp=, extra=bool, acc=bool, nslot=)    (with `prev`, batch statistics), and
                            prev_mode='relu' | 'moving': `prev` in that mode (BnMap: the coefficients it implies);
                            prev=None: the RAW form -- `out` is dy = conv^T(geff) [+ extra] [+ old], no mask; the
                            record still carries a red_out (filled with RED_RAW) that the launch must not touch
      vert                  None or dict(Cf=, has_dz=bool, nslot=), and ties=True: the finer map is a grid_map (seed
                            `seed`, default 0) taken as it is -- tied 2x2 maxima; the reference (O.pool2_bwd) routes to the
                            FIRST maximum in row-major window order
      a                     ('bn', Ca, nslot) or ('img', Ca, shift)            operand A of the weight gradients;
                            ('relu', Ca) / ('moving', Ca, nslot): a map under MPNN_ACT_RELU / MPNN_ACT_BN_MOVING
      wgrad                 False: a member without weight gradients (single launches only; Cg need not be 16k)
      Cv                    channels of the pooled finer map v (0: none)
      split                 n_split of the weight gradients
      wg_horz, wg_vert      level budgets
    Outputs live in Guarded buffers; reset() restores their initial contents before every launch."""

    def __init__(self, rng, spec):
        self.spec = sp = dict(gctx=None, horz=None, vert=None, a=('bn', 16, _hip.BN_SLOTS), Cv=0, split=1,
                              wg_horz=1, wg_vert=1, wgrad=True)
        sp.update(spec)
        n, H, W, Cg = sp['n'], sp['H'], sp['W'], sp['Cg']
        self.n, self.H, self.W, self.Cg = n, H, W, Cg
        lib = _hip.load()
        self.keep = []
        # g, or dz with the BatchNorm backward of the coarsest map applied on load
        g, g64 = f32(rng.standard_normal((n, H, W, Cg)))
        self.gd = dev(g)
        self.g_ctx = None
        if sp['gctx'] is not None:
            bm = BnMap(rng, (n, H, W, Cg), sp['gctx'])
            red = red_of(g64, bm.xh)
            self.g_ctx = bm.ctx(red, sp['gctx'])
            self.keep.append(bm)
            self.geff = bm.apply(g64, red)
        else:
            self.geff = g64
        # dgrad-horz
        self.h = None
        if sp['horz'] is not None:
            hz = sp['horz']
            Cp = hz['Cp']
            wh, wh64 = f32(rng.standard_normal((3, 3, Cp, Cg)) / 3 / np.sqrt(Cg))
            self.wh_pack = pack_weights([wh])[1][0]
            self.raw = 'prev' in hz and hz['prev'] is None
            self.prev = BnMap(rng, (n, H, W, Cp), hz['nslot'], mode=hz.get('prev_mode', 'batch'))
            self.prev_ctx = self.prev.ctx(None, hz['nslot'])
            ex64 = None
            self.exd = None
            if hz['extra']:
                ex, ex64 = f32(rng.standard_normal((n, H, W, Cp)))
                self.exd = dev(ex)
            dy = O.conv_same_bwd(np.zeros((n, H, W, Cp)), wh64, self.geff)[0]
            if ex64 is not None:
                dy = dy + ex64
            new = dy if self.raw else np.where(self.prev.y > 0, dy, 0.0)
            self.out = Guarded(n * H * W * Cp)
            self.red = Guarded(hz['nslot'] * 2 * Cp, torch.float64)
            terms = [new, new * self.prev.xh]
            self.red_ref = np.concatenate([t.reshape(-1, Cp).sum(0) for t in terms])
            self.red_abs = np.concatenate([np.abs(t).reshape(-1, Cp).sum(0) for t in terms])
            if hz['acc']:
                old, old64 = f32(rng.standard_normal((n, H, W, Cp)))
                self.out_init = old
                self.out_ref = old64 + new
                red0 = rng.standard_normal((hz['nslot'], 2 * Cp)) * 10.0
                self.red_init = red0
                self.red_ref = self.red_ref + red0.sum(0)
                self.red_abs = self.red_abs + np.abs(red0).sum(0)
            else:
                self.out_init, self.out_ref = np.nan, new
                self.red_init = 0.0
            if self.raw:                          # red_out must come back as it went in: an exact reference, no slack
                self.red_init = RED_RAW
                self.red_ref = np.full(2 * Cp, hz['nslot'] * RED_RAW)
                self.red_abs = np.zeros(2 * Cp)
            a = _hip.DgradHorzArgs()
            a.g, a.Cg = self.gd.data_ptr(), Cg
            a.g_ctx = C.pointer(self.g_ctx) if self.g_ctx is not None else None
            a.w_pack = self.wh_pack.data_ptr()
            a.dy_extra = ptr_or_none(self.exd)
            a.prev = None if self.raw else C.pointer(self.prev_ctx)
            a.out, a.red_out = self.out.ptr(), self.red.ptr()
            a.n, a.H, a.W, a.Cout = n, H, W, Cp
            a.accumulate = 1 if hz['acc'] else 0
            self.h = a
        # dgrad-vert
        self.v = None
        if sp['vert'] is not None:
            vt = sp['vert']
            Cf = vt['Cf']
            wv, wv64 = f32(rng.standard_normal((3, 3, Cf, Cg)) / 3 / np.sqrt(Cg))
            self.wv_pack = pack_weights([wv])[1][0]
            fs = None
            if vt.get('ties'):
                fs = grid_map(np.random.default_rng(vt.get('seed', 0)), (n, 2 * H, 2 * W, Cf))
            self.fine = BnMap(rng, (n, 2 * H, 2 * W, Cf), vt['nslot'], s=fs)
            dz, dz64 = f32(rng.standard_normal((n, 2 * H, 2 * W, Cf)))
            fred = red_of(dz64, self.fine.xh)
            self.fine_ctx = self.fine.ctx(fred, vt['nslot'])
            dp = O.conv_same_bwd(np.zeros((n, H, W, Cf)), wv64, self.geff)[0]
            self.dzg_ref = O.pool2_bwd(self.fine.s64, dp)
            if vt['has_dz']:
                self.dzg_ref = self.dzg_ref + self.fine.apply(dz64, fred)
                self.dzg_init = dz
            else:
                self.dzg_init = np.nan            # not read: every element is written
            self.dzg = Guarded(dz.size)
            a = _hip.DgradVertArgs()
            a.g, a.Cg = self.gd.data_ptr(), Cg
            a.g_ctx = C.pointer(self.g_ctx) if self.g_ctx is not None else None
            a.w_pack = self.wv_pack.data_ptr()
            a.fine = C.pointer(self.fine_ctx)
            a.fine_has_dz = 1 if vt['has_dz'] else 0
            a.dz_g_fine = self.dzg.ptr()
            a.n, a.H, a.W, a.Cout = n, H, W, Cf
            self.v = a
        # weight gradients
        self.w = self.slab = self.grads = self.dwv_ref = None
        if not sp['wgrad']:
            return
        kind = sp['a']
        Ca = kind[1]
        w = _hip.WgradArgs()
        if kind[0] == 'bn':
            self.abn = BnMap(rng, (n, H, W, Ca), kind[2])
            w.a = _hip.act(self.abn.sd, Ca, _hip.ACT_BN_BATCH, 0, self.abn.dev, self.abn.cnt)
            act64 = np.maximum(self.abn.y, 0.0)
        elif kind[0] in ('relu', 'moving'):
            self.abn = BnMap(rng, (n, H, W, Ca), kind[2] if len(kind) > 2 else 1, mode=kind[0])
            w.a = _hip.act(self.abn.sd, Ca, self.abn.act_mode, 0, self.abn.dev, self.abn.cnt)
            act64 = np.maximum(self.abn.y, 0.0)
        else:
            sh = kind[2]
            x, x64 = f32(rng.standard_normal((n, H << sh, W << sh, Ca)))
            self.xd = dev(x)
            w.a = _hip.act(self.xd, Ca, _hip.ACT_IDENTITY, sh)
            act64 = x64[:, ::1 << sh, ::1 << sh, :]
        Cv = sp['Cv']
        zeros = lambda ci: np.zeros((3, 3, ci, Cg))
        self.dwa_ref = O.conv_same_bwd(act64, zeros(Ca), self.geff)[1]
        self.db_ref = self.geff.sum((0, 1, 2))
        self.dwv_ref = None
        if Cv:
            vf, vf64 = f32(rng.standard_normal((n, 2 * H, 2 * W, Cv)))
            vp64 = O.pool2(vf64)
            self.vd = dev(vp64.astype(np.float32))          # the producer's pooled map (exact: a max of fp32 values)
            w.v, w.Cv = self.vd.data_ptr(), Cv
            self.dwv_ref = O.conv_same_bwd(vp64, zeros(Cv), self.geff)[1]
        w.g = self.gd.data_ptr()
        w.g_ctx = C.pointer(self.g_ctx) if self.g_ctx is not None else None
        self.sizes = [9 * Ca * Cg, 9 * Cv * Cg, Cg]
        self.offs = [0, self.sizes[0], self.sizes[0] + self.sizes[1]]
        total = sum(self.sizes)
        self.grads = Guarded(total)
        tiles = lib.mpnn_wgrad_tiles(n, H, W)
        self.tiles = tiles
        self.split = max(1, min(sp['split'], tiles))     # (the launchers clamp n_split the same way)
        self.slab = None
        if self.split > 1:
            stride = (total + 3) // 4 * 4
            self.slab = Guarded(self.split * stride)
            dst = self.slab
            w.split_stride = stride
            tab = []
            item = _hip.slab_item_size(self.split)
            for o, sz in zip(self.offs, self.sizes):
                for k in range(0, sz, item):
                    tab += [o + k, o + k, min(item, sz - k), self.split, stride, 0]
            self.tab = dev(np.array(tab, np.int32), torch.int32)
            self.n_items = len(tab) // 6
        else:
            dst = self.grads
            w.split_stride = 0
        w.dwa = dst.ptr(self.offs[0])
        w.dwv = dst.ptr(self.offs[1]) if Cv else None
        w.db = dst.ptr(self.offs[2])
        w.n, w.H, w.W, w.Cout, w.n_split = n, H, W, Cg, sp['split']
        self.w = w

    # -- launches ---------------------------------------------------------------------------------------------------
    def reset(self):
        if self.h is not None:
            self.out.fill(self.out_init)
            self.red.fill(self.red_init)
        if self.v is not None:
            self.dzg.fill(self.dzg_init)
        if self.grads is not None:
            self.grads.fill(np.nan)
        if self.slab is not None:
            self.slab.fill(np.nan)

    def member(self, m, wg_horz=None, wg_vert=None):
        m.horz = C.pointer(self.h) if self.h is not None else None
        m.vert = C.pointer(self.v) if self.v is not None else None
        m.wgrad = C.pointer(self.w)
        m.wg_horz = self.spec['wg_horz'] if wg_horz is None else wg_horz
        m.wg_vert = self.spec['wg_vert'] if wg_vert is None else wg_vert

    def finish(self):
        """mpnn_slab_reduce of the weight-gradient slabs (n_split > 1)."""
        if self.slab is not None:
            _hip.check(_hip.load().mpnn_slab_reduce(self.slab.ptr(), self.grads.ptr(), self.tab.data_ptr(), self.n_items,
                                                    stream()), 'slab_reduce')

    def results(self):
        torch.cuda.synchronize()
        r = {}
        if self.h is not None:
            r['out'] = self.out.get()
            r['red'] = self.red.get().reshape(-1, self.red.size // self.spec['horz']['nslot'])
        if self.v is not None:
            r['dzg'] = self.dzg.get()
        if self.grads is None:
            return r
        gr = self.grads.get()
        r['dwa'] = gr[:self.sizes[0]]
        r['dwv'] = gr[self.offs[1]:self.offs[2]]
        r['db'] = gr[self.offs[2]:]
        return r

    def guards_ok(self):
        bufs = ([self.grads] if self.grads is not None else []) + ([self.slab] if self.slab is not None else []) + \
               ([self.out, self.red] if self.h is not None else []) + ([self.dzg] if self.v is not None else [])
        return all(b.guards_ok() for b in bufs)


def ptr_or_none(t):
    return None if t is None else t.data_ptr()


def level_records(cases, budgets=None, reps=None):
    """(BwdMember array, device records) of a level; budgets: [(wg_horz, wg_vert)] per case (None: the spec's).
    reps: the _rep form (cases = reps * count, net r's at [r * count, ...))."""
    lib = _hip.load()
    k = len(cases)
    mem = (_hip.BwdMember * k)()
    for j, cs in enumerate(cases):
        b = budgets[j] if budgets is not None else (None, None)
        cs.member(mem[j], *b)
    size = lib.mpnn_msconv_bwd_level_record_size()
    host = (C.c_char * (size * k))()
    if reps is None:
        rc = lib.mpnn_msconv_bwd_level_prepare(mem, k, host)
    else:
        rc = lib.mpnn_msconv_bwd_level_prepare_rep(mem, k // reps, reps, host)
    _hip.check(rc, 'bwd_level_prepare')
    recs = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    return mem, recs


def run_level(cases, budgets=None):
    """mpnn_msconv_bwd_level over `cases` (then the slab reductions); returns every case's results."""
    lib = _hip.load()
    for cs in cases:
        cs.reset()
    mem, recs = level_records(cases, budgets)
    _hip.check(lib.mpnn_msconv_bwd_level(mem, len(cases), recs.data_ptr(), stream()), 'bwd_level')
    for cs in cases:
        cs.finish()
    return [cs.results() for cs in cases]


def run_level_rep(cases, reps):
    lib = _hip.load()
    for cs in cases:
        cs.reset()
    mem, recs = level_records(cases, reps=reps)
    _hip.check(lib.mpnn_msconv_bwd_level_rep(mem, len(cases) // reps, reps, recs.data_ptr(), stream()), 'bwd_level_rep')
    for cs in cases:
        cs.finish()
    return [cs.results() for cs in cases]


def run_single(cs):
    """The member as the three single launches mpnn_msconv_dgrad_horz, mpnn_msconv_dgrad_vert and mpnn_msconv_wgrad on
    its own records, each where present (what the engine emits under MPNN_STREAMS=1)."""
    lib = _hip.load()
    cs.reset()
    if cs.h is not None:
        _hip.check(lib.mpnn_msconv_dgrad_horz(C.byref(cs.h), stream()), 'dgrad_horz')
    if cs.v is not None:
        _hip.check(lib.mpnn_msconv_dgrad_vert(C.byref(cs.v), stream()), 'dgrad_vert')
    if cs.w is not None:
        _hip.check(lib.mpnn_msconv_wgrad(C.byref(cs.w), stream()), 'wgrad')
    cs.finish()
    return cs.results()


def run_scale(cs, horz=True):
    """The same member as one mpnn_msconv_bwd_scale launch (it sizes its own dgrad grids).  horz=False: without the
    member's dgrad-horz (the launch refuses a raw one); `out` / `red` then hold their initial contents."""
    cs.reset()
    _hip.check(_hip.load().mpnn_msconv_bwd_scale(C.byref(cs.h) if cs.h is not None and horz else None,
                                                  C.byref(cs.v) if cs.v is not None else None, C.byref(cs.w), stream()),
               'bwd_scale')
    cs.finish()
    return cs.results()


def run_pair(cs):
    """The member's two input gradients as one mpnn_msconv_dgrad_pair launch."""
    cs.reset()
    _hip.check(_hip.load().mpnn_msconv_dgrad_pair(C.byref(cs.h), C.byref(cs.v), stream()), 'dgrad_pair')
    return cs.results()
