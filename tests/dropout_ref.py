"""Reference of Dropout in front of an exit's classifier (csrc/dropout.hip), written out in numpy.

TEST INFRASTRUCTURE: nothing here is on the product path.

The reference's line (scripts/lib/layer_types.py:212-217) is ``self.x = tf.nn.dropout(x, self.hypers.λ)``, in TF 0.12
``x / keep_prob * floor(keep_prob + u)`` with u ~ U[0, 1): an element is kept iff u >= 1 - λ and scaled by 1/λ.  Here
u = r / 2^32 of a 32-bit Philox4x32-10 word r, so kept iff r >= thresh(λ) = ceil((1 - λ) 2^32) -- exact, so the mask of the
kernels can be restated bit for bit:

  key      (seed & 0xffffffff, seed >> 32) of the layer's 64-bit seed
  counter  (k >> 2, s, leaf, t): k the feature index of the NHWC-flattened map, s the sample's row, leaf the exit's leaf
           index, t the engine's training-step counter; word k & 3 of the four output words decides element k

  philox / philox_int      the generator, vectorised over numpy arrays / on plain Python ints (two independent restatements)
  thresh, words, mask      ceil((1 - λ) 2^32) as a uint32; the words and the keep mask [n, K] of one launch
  layer / layer_bwd        x m / λ and dx = (acc ? dx : 0) + m dxd / λ in float64; with ``dt=np.float32`` the kernels'
                           own arithmetic: times inv_keep = float32(1 / λ), dropped elements exact
  KERNEL_CASES             the records of tests/test_dropout_kernel.py
  RefNetDropout            oracle.ref_net.RefNet with the layer, on RefNetActivity (mixed heads keep working): the mask in
                           'tr', the identity in 'ev'
"""
import math

import numpy as np

try:
    import activity_error_ref as AR
except ImportError:                 # (the --emit child of tests/golden/dropout_ref_graph.py runs beside the REFERENCE's lib, without
    AR = None                       # the oracle: it uses the generator alone)

F64 = np.float64
M0, M1 = 0xD2511F53, 0xCD9E8D57          # the published multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the Weyl increments of the key
ROUNDS = 10
MASK32 = 0xFFFFFFFF
RANK_STRIDE = 0x9E3779B97F4A7C15        # data parallel: rank r draws with seed + r * RANK_STRIDE mod 2^64


def philox(counter, key):
    """Philox4x32-10 of counters [..., 4] under keys [..., 2] (uint32, broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (c[..., j] for j in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    m32 = np.uint64(MASK32)
    for _ in range(ROUNDS):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # (32 x 32 bits: no overflow in 64)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def philox_int(counter, key):
    """The same generator on plain Python ints: (c0, c1, c2, c3), (k0, k1) -> four ints."""
    c0, c1, c2, c3 = (int(v) for v in counter)
    k0, k1 = (int(v) for v in key)
    for _ in range(ROUNDS):
        hi0, lo0 = divmod(M0 * c0, 1 << 32)
        hi1, lo1 = divmod(M1 * c2, 1 << 32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) % (1 << 32), (k1 + W1) % (1 << 32)
    return c0, c1, c2, c3


def thresh(λ):
    """ceil((1 - λ) 2^32) in float64 as a uint32: a word r keeps its element iff r >= thresh.  (1 - λ) 2^32 rounds to 2^32
    for λ below 2^-53: the largest word still keeps.)"""
    return min(int(math.ceil((1.0 - float(λ)) * 4294967296.0)), MASK32)


def rank_seed(seed, rank):
    return (int(seed) + int(rank) * RANK_STRIDE) % (1 << 64)


def words(seed, t, leaf, n, K):
    """The word that decides every element of an [n, K] map: uint32 [n, K]."""
    Q = (K + 3) // 4
    ctr = np.zeros((n, Q, 4), np.uint32)
    ctr[..., 0] = np.arange(Q, dtype=np.uint32)[None, :]
    ctr[..., 1] = np.arange(n, dtype=np.uint32)[:, None]
    ctr[..., 2] = np.uint32(int(leaf) & MASK32)
    ctr[..., 3] = np.uint32(int(t) & MASK32)
    key = np.array([int(seed) & MASK32, (int(seed) >> 32) & MASK32], np.uint32)
    return philox(ctr, key).reshape(n, Q * 4)[:, :K]


def mask(seed, t, leaf, n, K, λ):
    """The keep mask [n, K] (bool) of the layer with keep probability λ."""
    return words(seed, t, leaf, n, K) >= np.uint32(thresh(λ))


def inv_keep(λ):
    return np.float32(1.0 / float(λ))


def layer(x, m, λ, dt=F64):
    """The layer on x [n, K] under the keep mask m: x m / λ (float64), or the kernels' x * inv_keep and +0 (float32)."""
    x = np.asarray(x, dt)
    if dt is F64:
        return x * m / dt(λ)
    return np.where(m, x * inv_keep(λ), dt(0))


def layer_bwd(dxd, m, λ, dx=None, dt=F64):
    """(dx, bound) = (dx given ? dx : 0) + m dxd / λ; bound = |dx| + |dxd| / λ.  float32: dx + dxd * inv_keep where kept, dx's
    own bits where dropped."""
    dxd = np.asarray(dxd, dt)
    base = np.zeros_like(dxd) if dx is None else np.asarray(dx, dt)
    bound = np.abs(np.asarray(base, F64)) + np.abs(np.asarray(dxd, F64)) / float(λ)
    if dt is F64:
        return base + m * dxd / dt(λ), bound
    return np.where(m, base + dxd * inv_keep(λ), base), bound


# ---- the cases of tests/test_dropout_kernel.py: (name, n, HW, C, act mode, λ, seed, leaf) -- a dozen, not the product of
# rows 1 / 5 / 128 / 130, maps 16x16 / 16x128 / 4x6 (K = 24) / 1x5 (K = 5: a quad tail) / 3x2 (K = 6) / 6x10 (K = 60) and
# λ 1 / 0.9 / 0.5 / 1e-3, both activation modes
KERNEL_CASES = [
    ('one-row',      1, 16, 16, 'batch', 0.5, 0, 0),
    ('ship',       128, 16, 16, 'batch', 0.5, 1, 3),
    ('ragged-rows', 130, 16, 16, 'batch', 0.9, 2 ** 40 + 7, 1),
    ('wide',         5, 16, 128, 'batch', 0.5, 3, 2),
    ('wide-128',   128, 16, 128, 'identity', 0.9, 4, 5),
    ('k24',          5, 4, 6, 'batch', 0.5, 5, 0),
    ('k5-tail',    130, 1, 5, 'batch', 0.5, 6, 7),
    ('k5-one',       1, 1, 5, 'identity', 0.9, 7, 0),
    ('k6',         128, 3, 2, 'batch', 1e-3, 8, 4),
    ('k60',          5, 6, 10, 'identity', 0.5, 2 ** 64 - 1, 46),
    ('keep-all',   130, 6, 10, 'batch', 1.0, 9, 2),
    ('rare',       128, 16, 16, 'identity', 1e-3, 10, 1),
]
KERNEL_TABLES = [('one-row',), ('ship', 'k5-tail'), ('ragged-rows', 'k24', 'wide'), ('wide-128', 'k5-one', 'k60'), ('k6', 'keep-all', 'rare')]
CASE = {c[0]: c for c in KERNEL_CASES}


def kernel_inputs(name):
    """fp32 inputs of one record: the pre-activation map x [n, HW, C] with the BatchNorm's parameters (as tests/exit_ref.py
    draws an affine map's), the head's gradient dxd and a dx to accumulate into, both [n, K]."""
    _, n, HW, C_, mode, λ, seed, leaf = CASE[name]
    rng = np.random.default_rng(sum(ord(ch) for ch in name))
    f = np.float32
    K = HW * C_
    d = dict(name=name, n=n, HW=HW, C=C_, K=K, mode=mode, λ=λ, seed=seed, leaf=leaf)
    d['x'] = rng.standard_normal((n, HW, C_)).astype(f)
    d['gamma'], d['beta'] = (rng.random(C_) + 0.5).astype(f), (rng.standard_normal(C_) * 0.2).astype(f)
    d['dxd'] = rng.standard_normal((n, K)).astype(f)
    d['dx'] = rng.standard_normal((n, K)).astype(f)
    d['dx'][0, 0] = -0.0                                    # (a dropped element of an accumulating dx keeps even this)
    return d


def activated(d, dt=F64):
    """(act(x) [n, K], bound): relu(bn(x)) with batch statistics, or x; bound = |γ / σ| (|x| + |mean|) + |β|, the sum of the
    absolute values of the element's terms."""
    import exit_ref as X
    x = np.asarray(d['x'], dt)
    a = X.act(x, d['mode'], d['gamma'], d['beta'], dt=dt).reshape(d['n'], d['K'])
    if d['mode'] == 'identity':
        return a, np.abs(np.asarray(a, F64))
    x64 = np.asarray(d['x'], F64).reshape(-1, d['C'])
    m, v = x64.mean(0), ((x64 - x64.mean(0)) ** 2).mean(0)
    k = np.abs(np.asarray(d['gamma'], F64)) / np.sqrt(v + 1e-6)
    bound = k * (np.abs(x64) + np.abs(m)) + np.abs(np.asarray(d['beta'], F64))
    return a, bound.reshape(d['n'], d['K'])


# ---- whole nets ------------------------------------------------------------------------------------------------------
class RefNetDropout(AR.RefNetActivity if AR is not None else object):
    """RefNet whose `_link` knows Dropout: x m / λ on torch float64 tensors in 'tr', with m = mask(seed, t, leaf, n, K, λ)
    of the layer's seed (offset by `rank`), the leaf index of the LogReg chain it stands in and the step counter t -- by
    default the step the net's engine took LAST (the parity tests run the oracle behind the product's step); in 'ev' the
    layer is the identity (the deliberate departure from the reference's line; `literal` restates the
    line as it stands, for the reference-graph golden)."""
    step = None                    # None: net.dropout_step - 1
    rank = 0
    literal = False                # True: the reference's line as it stands -- the mask in every mode

    def _link(self, ℓ, x, y, mode, out):
        if type(ℓ).__name__ != 'Dropout':
            return super()._link(ℓ, x, y, mode, out)
        out[id(ℓ)] = dict(c_err=0.0, c_mod=0.0, n_ops=0, x=x)
        λ = float(ℓ.hypers.λ)
        if (mode != 'tr' and not self.literal) or λ == 1.0:
            return x
        leaf = [id(c) for c in self.net.leaves].index(id(ℓ._chain))
        t = self.net.dropout_step - 1 if self.step is None else self.step
        n, K = int(x.shape[0]), int(np.prod(x.shape[1:]))
        m = mask(rank_seed(ℓ.hypers.seed, self.rank), t, leaf, n, K, λ)
        import torch
        x = x * torch.as_tensor(m.reshape(tuple(x.shape)), dtype=self.dtype) / λ
        out[id(ℓ)]['x'] = x
        return x
