"""Float64 restatements, input builders and case tables of the small launches around the conv path: the three BatchNorm
launches of csrc/misc.hip (mpnn_bn_relu_fwd, mpnn_bn_bwd_reduce, mpnn_bn_bwd_apply) and the 1x1 kernels of
csrc/conv_nhwc.hip (mpnn_conv_nhwc_fwd / _dgrad / _wgrad with supp = 1).  Pure numpy: the GPU tests
(tests/test_bn_launches.py, tests/test_conv1x1_kernels.py) launch what is built here, tests/test_small_launch_ref_cpu.py
checks the builders, the references and the limits themselves.

Every input is a float32 value carried exactly into float64 (hiputil.f32).  A map that feeds a ReLU decision is drawn
again until no float64 pre-ReLU value lies within MARGIN of zero, in every mode, so the kernel's fp32 arithmetic and the
reference cannot disagree on a mask and NO element is left out of a comparison.  Plain-ReLU maps then get exact 0.0f and
-0.0f in about 1 % of their elements: their mask is 0 ([x > 0]), and the kernel's y equals s there exactly.

Limits (tests/test_conv_hw.py): |got - ref| <= rel * bound + 1e-6 per element, bound = the float64 sum of the absolute
values of the element's terms, rel = 2e-6 (forward values, input gradients, elementwise BatchNorm outputs) or 4e-6 (1x1
weight and bias gradients); 1e-5 * bound + 1e-9 for the fp64 reductions, with the bounds of
tests/test_conv_ch.py::test_bn_launches_any_c_vs_float64.
"""
import zlib

import numpy as np

from hiputil import f32, slot_spread

SLOTS = 16                         # MPNN_BN_SLOTS: every statistics buffer holds this many slots
MARGIN = 1e-3
EPS = np.float32(1e-6)             # mpnn_act.eps is a float
REL, REL_W = 2e-6, 4e-6
MODES = ('id', 'relu', 'batch', 'moving')


def seed(case):
    return zlib.crc32(repr(case).encode())


def case_id(case):
    return '-'.join(str(f) for f in case)


def lim(bound, rel=REL):
    return rel * bound + 1e-6


def sum_lim(bound):
    return 1e-5 * bound + 1e-9


# ------------------------------------------------------------------ which kernel a launch selects (csrc/misc.hip)
def quad_bwd(C):
    """bn_shape_ok: mpnn_bn_bwd_reduce / _apply take the quad kernels."""
    return C % 4 == 0 and C <= 256 and 256 % (C // 4) == 0


def quad_fwd(C):
    """mpnn_bn_relu_fwd takes the quad kernel for EVERY C % 4 == 0 up to 256."""
    return C % 4 == 0 and C <= 256


# C: (mpnn_bn_relu_fwd, mpnn_bn_bwd_reduce / _apply); any4 / any1: the any-C kernels with and without 16-byte accesses
KERNELS = {
    1: ('any1', 'any1'), 3: ('any1', 'any1'), 4: ('quad', 'quad'), 8: ('quad', 'quad'), 12: ('quad', 'any4'),
    16: ('quad', 'quad'), 48: ('quad', 'any4'), 100: ('quad', 'any4'), 200: ('quad', 'any4'), 255: ('any1', 'any1'),
    256: ('quad', 'quad'), 257: ('any1', 'any1'), 260: ('any4', 'any4'), 300: ('any4', 'any4'), 511: ('any1', 'any1'),
    512: ('any4', 'any4'),
}


def selected(C):
    any_ = 'any4' if C % 4 == 0 else 'any1'
    return ('quad' if quad_fwd(C) else any_, 'quad' if quad_bwd(C) else any_)


def side(C):
    """Pixels a reduction workgroup takes side by side."""
    if quad_bwd(C):
        return 256 // (C // 4)
    return 256 // C if C <= 256 else 1


def reduce_blocks(C, n_pix):
    """Workgroups of mpnn_bn_bwd_reduce: 16 rounds each, at most 512."""
    return min(512, max(1, -(-n_pix // (16 * side(C)))))


# ------------------------------------------------------------------ an activation operand
class ActMap:
    """A map s [n_pix, C] (fp32) with its activation on load.  mode: 'id', 'relu', 'batch' (statistics of s itself, spread
    unevenly over nslot of the SLOTS slots; the others hold NaN) or 'moving' (m_avg / v_avg).  Float64 fields: pre (the
    pre-ReLU value; None for 'id'), y (the activation as a consumer sees it), on (pre > 0), xh, m, rstd, and gamma, beta
    (1, 0 for 'id' and 'relu').  margin None: the map is left as drawn."""

    def __init__(self, rng, n_pix, C, mode, nslot=8, margin=MARGIN, zeros=None):
        assert mode in MODES
        self.n_pix, self.C, self.mode, self.nslot, self.cnt = n_pix, C, mode, nslot, n_pix
        bn = mode in ('batch', 'moving')
        self.gamma = self.beta = self.m_avg = self.v_avg = self.sums = None
        self.gamma64, self.beta64 = np.ones(C), np.zeros(C)
        if bn:
            self.gamma, self.gamma64 = f32(rng.uniform(0.5, 1.5, C))
            beta = rng.standard_normal(C) * 0.3
            # (one pixel: batch statistics give y = beta whatever s is, so beta itself keeps the margin)
            self.beta, self.beta64 = f32(np.where(np.abs(beta) < 0.01, np.copysign(0.01, beta), beta))
        if mode == 'moving':
            self.m_avg, self.m64 = f32(rng.standard_normal(C) * 0.2)
            self.v_avg, self.v64 = f32(rng.uniform(0.5, 2.0, C))
        s = rng.standard_normal((n_pix, C)).astype(np.float32)
        for _ in range(1000):
            self.s, self.s64 = s, s.astype(np.float64)
            self._coef()
            if mode == 'id' or margin is None:
                break
            bad = np.abs(self.pre) < margin
            if not bad.any():
                break
            s[bad] = rng.standard_normal(int(bad.sum())).astype(np.float32)
        else:
            raise AssertionError('no draw keeps the margin')
        self.planted = np.zeros((n_pix, C), bool)
        if (mode == 'relu') if zeros is None else zeros:
            assert mode == 'relu'
            pick = rng.random((n_pix, C)) < 0.01
            pick.reshape(-1)[rng.integers(0, pick.size, 2)] = True            # (a small map gets its zeros too)
            idx = np.flatnonzero(pick.reshape(-1))
            s.reshape(-1)[idx] = np.where(np.arange(idx.size) % 2 == 0, 0.0, -0.0).astype(np.float32)
            self.planted = pick
            self.s, self.s64 = s, s.astype(np.float64)
            self._coef()
        if mode == 'batch':
            tot = np.concatenate([self.s64.sum(0), (self.s64 ** 2).sum(0)])
            self.sums = np.full((SLOTS, 2 * C), np.nan)
            self.sums[:nslot] = slot_spread(tot, nslot, rng)

    def _coef(self):
        s, C = self.s64, self.C
        if self.mode == 'batch':
            self.m = s.mean(0)
            self.var = ((s - self.m) ** 2).mean(0)
        elif self.mode == 'moving':
            self.m, self.var = self.m64, self.v64
        else:
            self.m, self.var = np.zeros(C), None
        self.rstd = np.ones(C) if self.var is None else 1.0 / np.sqrt(self.var + np.float64(EPS))
        self.xh = (s - self.m) * self.rstd
        if self.mode == 'id':
            self.pre, self.y, self.on = None, s, None
        else:
            self.pre = self.gamma64 * self.xh + self.beta64
            self.y, self.on = np.maximum(self.pre, 0.0), self.pre > 0

    # -- float64 references with their absolute-term bounds
    def fwd(self):
        """mpnn_bn_relu_fwd: (y, bound)."""
        if self.mode == 'id':
            return self.y, np.abs(self.y)
        return self.y, np.abs(self.gamma64 * self.rstd) * (np.abs(self.s64) + np.abs(self.m)) + np.abs(self.beta64)

    def reduce(self, dy64):
        """mpnn_bn_bwd_reduce: (dz, red [2C], terms [2C])."""
        dz = dy64 * self.on
        red = np.concatenate([dz.sum(0), (dz * self.xh).sum(0)])
        terms = np.concatenate([np.abs(dz).sum(0), np.abs(dz * self.xh).sum(0)])
        return dz, red, terms

    def apply(self, dz64, red64):
        """mpnn_bn_bwd_apply: (g, bound); red64 None: ctx->red == NULL, zero reductions."""
        C = self.C
        red = np.zeros(2 * C) if red64 is None else red64
        k = self.gamma64 * self.rstd
        g = k * (dz64 - red[:C] / self.cnt - self.xh * red[C:] / self.cnt)
        return g, np.abs(k) * (np.abs(dz64) + np.abs(red[:C]) / self.cnt + np.abs(self.xh * red[C:]) / self.cnt)

    # -- the same operations in float32, as a correct kernel may evaluate them
    def coef32(self):
        """(m, rstd, gamma * rstd, beta) as bn_coef gives them."""
        C, one = self.C, np.ones(self.C, np.float32)
        if self.mode in ('id', 'relu'):
            return 0 * one, one, one, 0 * one
        if self.mode == 'batch':
            tot = np.zeros(2 * C)
            for r in range(self.nslot):
                tot = tot + self.sums[r]
            mean = tot[:C] * (1.0 / self.cnt)
            var = np.maximum(tot[C:] * (1.0 / self.cnt) - mean * mean, 0.0)
            m, v = mean.astype(np.float32), var.astype(np.float32)
        else:
            m, v = self.m_avg, self.v_avg
        rstd = (1.0 / np.sqrt((v + EPS).astype(np.float64))).astype(np.float32)
        return m, rstd, self.gamma * rstd, self.beta

    def fwd32(self):
        if self.mode == 'id':
            return self.s
        m, _, k, b = self.coef32()
        return np.maximum((self.s - m) * k + b, np.float32(0))

    def reduce32(self, dy):
        m, rstd, k, b = self.coef32()
        d = self.s - m
        dz = np.where(d * k + b > 0, dy, np.float32(0))
        return dz, np.concatenate([dz.sum(0, dtype=np.float64), (dz * (d * rstd)).sum(0, dtype=np.float64)])

    def apply32(self, dz, red64):
        m, rstd, k, _ = self.coef32()
        C = self.C
        red = np.zeros(2 * C) if red64 is None else red64
        e4, e5 = (red[:C] / self.cnt).astype(np.float32), (red[C:] / self.cnt).astype(np.float32)
        return k * (dz - e4 - (self.s - m) * rstd * e5)


# ------------------------------------------------------------------ BatchNorm launch cases
# (C, n_pix, mode, nslot, red_nslot); red_nslot 0 means 1
def _pixel_counts(C):
    return sorted({1, side(C) - 1, 3 * 16 * side(C) + 5} - {0})


BN_C = [1, 3, 4, 8, 12, 16, 100, 200, 255, 256, 257, 260, 511, 512]
BN_C_MODES = [3, 8, 48, 200, 260, 512]                     # every kernel of both selections sees every mode
BN_SLOT_PAIRS = [(1, 0), (3, 1), (16, 3), (8, 16)]
BN_CASES = [(C, p, 'batch', 8, 8) for C in BN_C for p in _pixel_counts(C)]
BN_CASES += [(C, _pixel_counts(C)[-1], 'batch', ns, rn) for C in BN_C_MODES for ns, rn in BN_SLOT_PAIRS]
BN_CASES += [(C, _pixel_counts(C)[-1], mode, 1, rn) for C in BN_C_MODES for mode, rn in (('moving', 3), ('relu', 1), ('id', 1))]
# mpnn_bn_relu_fwd against mpnn_bn_bwd_reduce on maps WITHOUT the margin: (C, n_pix, mode)
CONTRACT_CASES = [(C, 301, mode) for C in (12, 48, 256, 300) for mode in ('batch', 'moving', 'relu')]


def bn_inputs(case):
    C, n_pix, mode, nslot, red_nslot = case
    rng = np.random.default_rng(seed(case))
    d = dict(a=ActMap(rng, n_pix, C, mode, nslot), rn=max(red_nslot, 1))
    d['dy'], d['dy64'] = f32(rng.standard_normal((n_pix, C)))
    d['dz'], d['dz64'] = f32(rng.standard_normal((n_pix, C)))              # (mpnn_bn_bwd_apply takes any dz)
    d['red64'] = rng.standard_normal(2 * C) * 10
    d['red'] = np.full((SLOTS, 2 * C), np.nan)
    d['red'][:d['rn']] = slot_spread(d['red64'], d['rn'], rng)
    d['prior'] = rng.standard_normal((SLOTS, 2 * C)) * 10                  # red_out before the launch, every slot
    return d


def contract_inputs(case):
    C, n_pix, mode = case
    rng = np.random.default_rng(seed(case))
    a = ActMap(rng, n_pix, C, mode, 8, margin=None)
    dy = rng.standard_normal((n_pix, C)).astype(np.float32)
    dy[dy == 0] = 1.0
    return a, dy


# ------------------------------------------------------------------ 1x1 conv cases
PAIRS = [(1, 1), (3, 16), (4, 17), (15, 1), (16, 16), (17, 15), (18, 20), (20, 18), (100, 10), (255, 256), (256, 255), (256, 256)]
ACTS = ['id', 'relu', 'batch1', 'batch3', 'batch8', 'moving']
M_SHAPES = [(1, 1, 1), (5, 3, 1), (2, 1, 8), (1, 17, 1), (3, 3, 7), (2, 4, 8), (5, 1, 13), (3, 11, 31), (4, 8, 32), (5, 5, 41)]
M_PAIRS = [(17, 15), (20, 18), (4, 17)]
assert [n * h * w for n, h, w in M_SHAPES] == [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]

# forward and weight gradient: (n, H, W, Cin, Cout, act on load)
CONV_CASES = [(5, 3, 7, ci, co, ACTS[(i + j) % 6]) for i, (ci, co) in enumerate(PAIRS) for j in (0, 3)]
CONV_CASES += [(n, h, w, ci, co, ACTS[(i + j) % 6]) for i, (n, h, w) in enumerate(M_SHAPES) for j, (ci, co) in enumerate(M_PAIRS)]
CONV_BIG_W = (5, 32, 410, 4, 5, 'batch3')                  # M = 65 600: beyond the weight gradient's 64 pixel splits
CONV_BIG_G = (5, 64, 410, 3, 2, 'relu')                    # M = 131 200: beyond the GEMM's 2048 workgroups
CONV_CASES += [CONV_BIG_W, CONV_BIG_G]
# input gradient: (n, H, W, Cg, Cin, relu_src)
DGRAD_CASES = [(5, 3, 7, co, ci, m) for ci, co in PAIRS for m in (False, True)]
DGRAD_CASES += [(n, h, w, co, ci, (i + j) % 2 == 0) for i, (n, h, w) in enumerate(M_SHAPES) for j, (ci, co) in enumerate(M_PAIRS)]
DGRAD_CASES += [(5, 64, 410, 2, 3, True)]
# forward with the identity matrix against mpnn_bn_relu_fwd: (n, H, W, C, act)
IDENT_CASES = [(5, 3, 7, C, act) for C in (12, 48, 256) for act in ('id', 'relu', 'batch3', 'moving')]


def act_of(rng, M, C, act):
    return ActMap(rng, M, C, act.rstrip('0123456789'), int(act[5:]) if act.startswith('batch') else 1)


def conv_inputs(case):
    n, H, W, ci, co, act = case
    M = n * H * W
    rng = np.random.default_rng(seed(case))
    d = dict(M=M, a=act_of(rng, M, ci, act))
    d['w'], d['w64'] = f32(rng.standard_normal((ci, co)) * 0.2)
    d['b'], d['b64'] = f32(rng.standard_normal(co) * 0.1)
    d['g'], d['g64'] = f32(rng.standard_normal((M, co)))
    d['dw0'], d['dw064'] = f32(rng.standard_normal((ci, co)))             # known priors of the accumulated outputs
    d['db0'], d['db064'] = f32(rng.standard_normal(co))
    return d


def conv_fwd_ref(d):
    y = d['a'].y
    return y @ d['w64'] + d['b64'], np.abs(y) @ np.abs(d['w64']) + np.abs(d['b64'])


def conv_wgrad_ref(d):
    """(dw, its bound, db, its bound) from zero."""
    y, g = d['a'].y, d['g64']
    return y.T @ g, np.abs(y).T @ np.abs(g), g.sum(0), np.abs(g).sum(0)


def dgrad_inputs(case):
    n, H, W, cg, ci, masked = case
    M = n * H * W
    rng = np.random.default_rng(seed(case))
    d = dict(M=M, src=ActMap(rng, M, ci, 'relu') if masked else None)
    d['g'], d['g64'] = f32(rng.standard_normal((M, cg)))
    d['w'], d['w64'] = f32(rng.standard_normal((ci, cg)) * 0.2)           # the forward weight [Cin][Cout = Cg]
    return d


def conv_dgrad_ref(d):
    dx, bound = d['g64'] @ d['w64'].T, np.abs(d['g64']) @ np.abs(d['w64']).T
    if d['src'] is not None:
        dx, bound = dx * d['src'].on, bound * d['src'].on
    return dx, bound


def matmul32(a, b, block=1024):
    """a.T @ b over the rows in float32, block by block (the two large-M cases)."""
    out = np.zeros((a.shape[1], b.shape[1]), np.float32)
    for r in range(0, a.shape[0], block):
        out += a[r:r + block].T @ b[r:r + block]
    return out
