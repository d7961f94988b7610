// mpnn_dropout_fwd / mpnn_dropout_bwd: Dropout in front of an exit's classifier (reference layer_types.py:212-217,
// tf.nn.dropout(x, λ) of TF 0.12: x / keep_prob * floor(keep_prob + u)) on the block's coarsest map, flattened NHWC as
// LinTrans flattens it.  One launch each: all rows, all features, all records of a table.
//
// The mask is a pure function of (seed, t, leaf, s, k) -- s the sample's row, k = (h W + w) C + c the feature: one
// Philox4x32-10 block per quad of four consecutive features, key (seed_lo, seed_hi), counter (k >> 2, s, leaf, t), word
// k & 3 decides element k; kept iff word >= thresh (thresh = ceil((1 - λ) 2^32), from the host).  Nothing of the mask is
// stored: the backward launch draws it again.  t is read from DEVICE memory (a->step), so a captured graph replays with a
// new step counter.  Neither the grid, the record's place in the table nor the other records' sizes enter a value.
//
//   fwd:  xd[s][k] = keep ? act(x[s][k]) * inv_keep : +0          act: relu(bn(x)) with the coefficients and the expression
//                                                                 of mpnn_bn_relu_fwd (bn_coef, common.h), or the identity
//   bwd:  dx[s][k] = (accumulate ? dx[s][k] : +0) + (keep ? dxd[s][k] * inv_keep : 0); an accumulating dx keeps its bits
//                    where the element was dropped
//
// Memory-bound elementwise kernels: a grid-stride loop over the n * ceil(K / 4) quads of a record, 16-byte loads and stores
// where K % 4 == 0 (every row then starts on a 16-byte boundary) and element accesses otherwise; a thread keeps the
// BatchNorm coefficients of its quad's channels while the stride leaves it on the same columns (the launcher picks a
// power-of-two grid: K / 4 a power of two up to the grid's threads -- every shipped exit map -- never recomputes them).
// No atomics, no LDS.
#include "common.h"
#include <cmath>
#include <cstddef>

struct DropoutG {
    ActG a;  int HW;  int n;
    unsigned seed_lo, seed_hi, leaf, thresh;  float inv_keep;
    gptr<const unsigned> step;
    gptr<float> xd;
    gptr<const float> dxd;  gptr<float> dx;  int accumulate;
};
static_assert(sizeof(DropoutG) == sizeof(mpnn_dropout_args) && offsetof(DropoutG, step) == offsetof(mpnn_dropout_args, step) &&
              offsetof(DropoutG, thresh) == offsetof(mpnn_dropout_args, thresh) && offsetof(DropoutG, dx) == offsetof(mpnn_dropout_args, dx) &&
              offsetof(DropoutG, accumulate) == offsetof(mpnn_dropout_args, accumulate), "DropoutG mirrors mpnn_dropout_args");

#define DROP_THREADS 256

// Philox4x32-10 (Salmon et al., SC'11): the published multipliers and Weyl increments, ten rounds.
struct Philox4 { unsigned w[4]; };
__host__ __device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;  c3 = (unsigned)p0;  c0 = n0;  c2 = n2;
        k0 += 0x9E3779B9u;  k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

template <bool BWD>
__global__ __launch_bounds__(DROP_THREADS) void dropout_k(const mpnn_dropout_args *__restrict__ table) {
    const DropoutG a = ((const DropoutG *)table)[blockIdx.y];
    const int C = a.a.C, K = a.HW * C, Q = (K + 3) >> 2;
    const long total = (long)a.n * Q, stride = (long)gridDim.x * DROP_THREADS;
    long q = (long)blockIdx.x * DROP_THREADS + threadIdx.x;
    if (q >= total) return;
    const unsigned t = *a.step;
    const bool vec = (K & 3) == 0;
    const bool bn = !BWD && a.a.mode != MPNN_ACT_IDENTITY;
    const float inv_keep = a.inv_keep;
    float cm[4] = {0.f, 0.f, 0.f, 0.f}, ck[4] = {1.f, 1.f, 1.f, 1.f}, cb[4] = {0.f, 0.f, 0.f, 0.f};
    int have = -1;                                     // the column quad the coefficients are of
    for (; q < total; q += stride) {
        const int s = (int)(q / Q), kq = (int)(q - (long)s * Q), k0 = kq * 4;
        const int cnt = min(4, K - k0);
        const Philox4 r = philox4x32_10((unsigned)kq, (unsigned)s, a.leaf, t, a.seed_lo, a.seed_hi);
        const size_t at = (size_t)s * K + k0;
        if constexpr (!BWD) {
            if (bn && kq != have) {
                have = kq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < cnt) { const BnC c = bn_coef(a.a, (k0 + j) % C); cm[j] = c.m; ck[j] = c.gamma * c.rstd; cb[j] = c.beta; }
                }
            }
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec) {
                const f32x4 v = *pcast<const f32x4>(a.a.x + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < cnt) x[j] = a.a.x[at + j];
            }
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = bn ? fmaxf((x[j] - cm[j]) * ck[j] + cb[j], 0.f) : x[j];
                y[j] = r.w[j] >= a.thresh ? v * inv_keep : 0.f;
            }
            if (vec) *pcast<f32x4>(a.xd + at) = f32x4{y[0], y[1], y[2], y[3]};
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < cnt) a.xd[at + j] = y[j];
            }
        } else {
            float g[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec) {
                const f32x4 v = *pcast<const f32x4>(a.dxd + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = v[j];
                if (a.accumulate) {
                    const f32x4 w = *pcast<const f32x4>(a.dx + at);
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[j] = w[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < cnt) { g[j] = a.dxd[at + j]; if (a.accumulate) d[j] = a.dx[at + j]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = r.w[j] >= a.thresh ? d[j] + g[j] * inv_keep : d[j];      // (dropped: d's own bits, +0 without accumulate)
            if (vec) *pcast<f32x4>(a.dx + at) = f32x4{d[0], d[1], d[2], d[3]};
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < cnt) a.dx[at + j] = d[j];
            }
        }
    }
}

extern "C" int mpnn_dropout_check(const mpnn_dropout_args *rec) {
    if (!rec || !rec->step || rec->n < 1 || rec->HW < 1) return MPNN_E_ARG;
    if (!std::isfinite(rec->inv_keep) || !(rec->inv_keep >= 1.0f)) return MPNN_E_ARG;
    if (rec->accumulate != 0 && rec->accumulate != 1) return MPNN_E_ARG;
    if (rec->a.x && !rec->xd) return MPNN_E_ARG;                              // (a forward record)
    if ((rec->dxd == nullptr) != (rec->dx == nullptr)) return MPNN_E_ARG;     // (a backward record)
    if (!rec->a.x && !rec->dxd) return MPNN_E_ARG;
    if (rec->a.x) {
        if (rec->a.mode != MPNN_ACT_IDENTITY && rec->a.mode != MPNN_ACT_BN_BATCH) return MPNN_E_ARG;
        if (rec->a.mode == MPNN_ACT_BN_BATCH &&
            (!rec->a.sum || !rec->a.gamma || !rec->a.beta || rec->a.cnt < 1 || rec->a.nslot < 1 || rec->a.nslot > MPNN_BN_SLOTS))
            return MPNN_E_ARG;
    }
    if (rec->a.shift != 0 || rec->a.C < 1 || rec->a.C > 512) return MPNN_E_SHAPE;
    // 32-bit byte offsets of the map, as everywhere in the engine; the Philox counter holds any k >> 2 and s below that
    if ((long long)rec->HW * rec->a.C > (1LL << 30) / 4 || (long long)rec->n * rec->HW * rec->a.C >= (1LL << 30)) return MPNN_E_SHAPE;
    return 0;
}

template <bool BWD>
static int dropout_launch(const mpnn_dropout_args *dev_table, int count, int n_max, int k_max, void *stream) {
    if (!dev_table || count < 1 || n_max < 1 || k_max < 1) return MPNN_E_ARG;
    if (count > 65535 || (long long)n_max * k_max >= (1LL << 30)) return MPNN_E_SHAPE;
    // about eight quads per thread (a thread's BatchNorm coefficients are sixteen slot loads per channel), a power of two
    const long long quads = (long long)n_max * ((k_max + 3) / 4);
    unsigned gx = 1;
    while (gx < 1024 && (long long)gx * DROP_THREADS * 8 < quads) gx *= 2;
    hipLaunchKernelGGL(dropout_k<BWD>, dim3(gx, (unsigned)count), dim3(DROP_THREADS), 0, (hipStream_t)stream, dev_table);
    MPNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mpnn_dropout_fwd(const mpnn_dropout_args *dev_table, int count, int n_max, int k_max, void *stream) {
    return dropout_launch<false>(dev_table, count, n_max, k_max, stream);
}

extern "C" int mpnn_dropout_bwd(const mpnn_dropout_args *dev_table, int count, int n_max, int k_max, void *stream) {
    return dropout_launch<true>(dev_table, count, n_max, k_max, stream);
}

// The generator on the host (three published known answers: tests/test_dropout_ref_cpu.py holds the same table to the
// numpy reference; this entry point lets a test hold the kernels' own routine to it without a GPU).
extern "C" int mpnn_philox4x32_10(const unsigned *counter, const unsigned *key, unsigned *out) {
    if (!counter || !key || !out) return MPNN_E_ARG;
    const Philox4 r = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    for (int j = 0; j < 4; ++j) out[j] = r.w[j];
    return 0;
}
