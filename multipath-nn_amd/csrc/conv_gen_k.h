// The general forward / input-gradient conv kernel gen_conv_k and what it is built from (tile geometry, operands, act
// tables), shared by conv_gen.hip (every launch without a sample list, and the weight-gradient kernel) and
// conv_gen_list.hip (the forward kernel on a sample list); conv_gen_ch.hip holds the fitted-tile instantiations and the
// scalar-g weight-gradient kernel of the any-channel family (mpnn_msconv_*_ch).  See conv_gen.hip for the contraction.
#pragma once
#include "common.h"

#define GEN_KMAX 7           // largest filter side
#define GEN_CMAX 512         // channels of any operand

enum { GEN_FWD = 0, GEN_DGH_BN = 1, GEN_DGH_RAW = 2, GEN_DGV = 3 };

// Pixel tiles of 64 output pixels, TSy x TSx pixels of TP images: a side of 8 on an axis longer than 4, of 4 otherwise
// (8x8x1, 8x4x2, 4x8x2, 4x4x4), ceil(H / TSy) x ceil(W / TSx) tiles per group of TP images.  A tile may hang over the
// bottom / right edge of the map (H or W not a multiple of the side): those pixels are computed on zeros and masked
// wherever they would be stored or summed.  On the maps of mpnn_msconv_gen_check (square, 4 or a multiple of 8) this is
// 8x8 tiles of one image / 4x4 maps of four images with no pixel masked.
struct GenGeo { int TSy, TSx, TP, tpy, tpx, tiles; };
__host__ __device__ inline GenGeo gen_geo(int n, int H, int W) {
    GenGeo g;
    g.TSy = H > 4 ? 8 : 4;
    g.TSx = W > 4 ? 8 : 4;
    g.TP = 64 / (g.TSy * g.TSx);
    g.tpy = (H + g.TSy - 1) / g.TSy;
    g.tpx = (W + g.TSx - 1) / g.TSx;
    g.tiles = (n + g.TP - 1) / g.TP * g.tpy * g.tpx;
    return g;
}
__device__ __forceinline__ void gen_tile_origin(const GenGeo &g, int t, int &n0, int &y0, int &x0) {
    const int per = g.tpy * g.tpx, r = t % per;
    n0 = (t / per) * g.TP;  y0 = (r / g.tpx) * g.TSy;  x0 = (r % g.tpx) * g.TSx;
}
__device__ __forceinline__ void gen_pix(const GenGeo &g, int p, int &img, int &ty, int &tx) {
    const int a = g.TSy * g.TSx;
    img = p / a;
    const int r = p - img * a;
    ty = r / g.TSx;  tx = r - ty * g.TSx;
}

// One operand of the contraction (input map and filter).
struct GenOp {
    const float *x;  int C;  int shift;  int bn;      // bn: the act table cA applies (forward operand A only)
    const float *w;  int kh, kw, pt, pl;              // filter, padding before
    int wk, wn, wtap;                                 // strides of input channel, output channel, tap in w
    int flip;                                         // input gradient: taps mirrored
};

struct GenP {
    GenOp op[2];  int nops;
    int n, H, W, Cout;
    const float *bias;  float *out;  float *pool_out;  double *out_sum;  int out_nslot;      // GEN_FWD
    const float *extra;  int acc_out;                                                        // GEN_DGH_*
    const float *sprev;  mpnn_act pbn;  double *red_out;  int red_out_nslot;                 // GEN_DGH_BN / GEN_DGV
    const double *red;  int has_dz;  int red_nslot;                                          // GEN_DGV
    mpnn_act a;                                                                              // GEN_FWD: operand A's act
    const int *idx;  const int *cnt;                                                         // GEN_FWD with a sample list
};

constexpr int GEN_HALO = 4 * (4 + GEN_KMAX - 1) * (4 + GEN_KMAX - 1) * 16;      // floats: >= 8x8 + halo of one image
constexpr int GEN_WROW = GEN_KMAX * 16 * 64;                                      // floats: one tap row of a chunk
static_assert(GEN_HALO >= (8 + GEN_KMAX - 1) * (8 + GEN_KMAX - 1) * 16, "halo buffer");
static_assert(GEN_HALO >= 2 * (8 + GEN_KMAX - 1) * (4 + GEN_KMAX - 1) * 16, "halo buffer: 8x4 / 4x8 tiles of two images");
static_assert(GEN_HALO >= 64 * 64, "the pool buffer reuses the halo");

// The act table of operand A (forward): coefficients (m, gamma * rstd, beta), as the tuned forward bodies use them.
__device__ __forceinline__ void gen_act_table(const mpnn_act &a, float *cA) {
    if (a.mode == MPNN_ACT_IDENTITY) return;
    for (int c = threadIdx.x; c < a.C; c += blockDim.x) {
        const BnC k = bn_coef(a, c);
        cA[c * 3] = k.m;  cA[c * 3 + 1] = k.gamma * k.rstd;  cA[c * 3 + 2] = k.beta;
    }
}

// The BatchNorm-backward coefficients of output channels co0 .. co0 + 63 (as conv_kernel.h: m, rstd, gamma * rstd and
// beta, 0 (dgrad-horz) or the two reductions / cnt (dgrad-vert)).
__device__ __forceinline__ void gen_bwd_table(const mpnn_act &bn, const double *red, int red_nslot, int co0, int Cout,
                                              bool horz, float *cE, int nc = 64) {
    const int c = (int)threadIdx.x;
    if (c >= nc || co0 + c >= Cout) return;
    float *e = cE + c * 5;
    if (bn.mode == MPNN_ACT_BN_BATCH) { bn_bwd_row(bn, horz ? nullptr : red, red_nslot, co0 + c, horz, e); return; }
    const BnC k = bn_coef(bn, co0 + c);
    e[0] = k.m;  e[1] = k.rstd;  e[2] = k.gamma * k.rstd;
    if (horz) { e[3] = k.beta;  e[4] = 0.f; }
    else {
        const double inv = 1.0 / (double)bn.cnt;
        double r0 = 0.0, r1 = 0.0;
        if (red) slot_sum2(red, 2 * bn.C, co0 + c, bn.C + co0 + c, red_nslot, r0, r1);
        e[3] = (float)(r0 * inv);  e[4] = (float)(r1 * inv);
    }
}

// Four channels c .. c + 3 of pixel (n, y, x) of an operand, act applied (zero outside the map / the channels).
__device__ __forceinline__ f32x4 gen_ld4(const GenOp &o, const float *cA, int n, int y, int x, int H, int W, int c) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int sh = o.shift;
    const size_t pix = ((size_t)n * (size_t)(H << sh) + (size_t)(y << sh)) * (size_t)(W << sh) + (size_t)(x << sh);
    const float *src = o.x + pix * (size_t)o.C;
    if ((o.C & 3) == 0) {
        if (c < o.C) v = *(const f32x4 *)(src + c);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c + j < o.C ? src[c + j] : 0.f;
    }
    if (o.bn) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = c + j < o.C ? fmaxf((v[j] - cA[(c + j) * 3]) * cA[(c + j) * 3 + 1] + cA[(c + j) * 3 + 2], 0.f) : 0.f;
    }
    return v;
}

// mfma_drain() with the accumulators of one or two output tiles held in their AGPRs across the wait.
template <int NT>
__device__ __forceinline__ void gen_drain_acc(f32x4 (&acc)[NT]) {
    static_assert(NT == 1 || NT == 2, "tiles");
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NT == 1) asm volatile("s_nop 15" : "+a"(acc[0]) : : "memory");
    else asm volatile("s_nop 15" : "+a"(acc[0]), "+a"(acc[1]) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ---------------------------------------------------------------------------
// Forward / input gradients.  grid (pixel tiles, 16 NT-channel output groups), 256 threads.
//
// NT: 16-channel output tiles per wave (4: a workgroup makes 64 output channels; the any-channel family also runs 2 and 1
// on layers of <= 32 / <= 16 output channels, conv_gen_ch.hip).  The weight stage, the accumulators, the epilogue, the
// pool buffer and the statistics reduction follow NT; the contraction of an output element (chunk, tap row, tap, k-step)
// does not, so every NT writes the same bits.
//
// IDX (GEN_FWD only): the launch runs on the sample list p.idx[0 .. *p.cnt) -- slot s of the launch is image idx[s] of
// every buffer (mpnn_conv_fwd_args.idx / cnt).  The tiles are laid over the SLOTS (p.n is the capacity the grid is sized
// for); the count is read here, on the device.  A workgroup whose first slot is beyond the count leaves before its first
// barrier; the images of the tile's <= 4 slots are resolved once (simg: -1 for a slot beyond the count) and the halo
// loader and the epilogue go through that table, so a slot beyond the count is staged as zeros and stored nowhere.  A
// pixel's arithmetic does not depend on its slot: a listed image gets the bits of the dense launch.
// The IDX instantiation is a translation unit of its own (conv_gen_list.hip: gen_fwd_list_launch), so that this one's
// kernels stay what they are.
// ---------------------------------------------------------------------------
int gen_fwd_list_launch(const GenP &p, dim3 grid, hipStream_t stream);

template <int EPI, bool IDX = false, int NT = 4>
__global__ __launch_bounds__(256) void gen_conv_k(const GenP p) {
    static_assert(!IDX || EPI == GEN_FWD, "sample lists: forward only");
    static_assert(NT == 1 || NT == 2 || NT == 4, "16-channel tiles per wave");
    constexpr int NC = 16 * NT, LNC = NT == 4 ? 6 : NT == 2 ? 5 : 4;      // output channels of a workgroup, log2
    __shared__ __attribute__((aligned(16))) float halo[GEN_HALO];
    __shared__ __attribute__((aligned(16))) float wl[GEN_WROW / 64 * NC];
    __shared__ float cA[EPI == GEN_FWD ? 3 * GEN_CMAX : 1];
    __shared__ float cE[EPI == GEN_FWD || EPI == GEN_DGH_RAW ? 1 : 5 * NC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i16 = lane & 15, q = lane >> 4;
    const GenGeo g = gen_geo(p.n, p.H, p.W);
    const int t = blockIdx.x, co0 = blockIdx.y * NC;
    int n0, y0, x0;
    gen_tile_origin(g, t, n0, y0, x0);
    [[maybe_unused]] __shared__ int simg[IDX ? 4 : 1];
    if constexpr (IDX) {
        const int cnt = min(*p.cnt, p.n);                  // (uniform: every lane reads the same word)
        if (n0 >= cnt) return;
        if (tid < 4) {
            const int s = n0 + tid, im = s < cnt && tid < g.TP ? p.idx[s] : -1;
            simg[tid] = (unsigned)im < (unsigned)p.n ? im : -1;      // (an index beyond the buffers is no image)
        }
    }
    if constexpr (EPI == GEN_FWD) gen_act_table(p.a, cA);
    if constexpr (EPI == GEN_DGH_BN) gen_bwd_table(p.pbn, nullptr, 0, co0, p.Cout, true, cE, NC);
    if constexpr (EPI == GEN_DGV) gen_bwd_table(p.pbn, p.red, p.red_nslot, co0, p.Cout, false, cE, NC);
    __syncthreads();

    int img, ty, tx;
    gen_pix(g, wave * 16 + i16, img, ty, tx);              // this lane's A row
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int part = 0; part < p.nops; ++part) {
        const GenOp o = p.op[part];
        const int HH = g.TSy + o.kh - 1, HWd = g.TSx + o.kw - 1, nsl = g.TP * HH * HWd;
        const bool kfast = o.wk == 1;
        for (int c0 = 0; c0 < o.C; c0 += 16) {
            __syncthreads();                               // (the previous chunk's MFMAs are done with the halo)
            for (int e = tid; e < nsl * 4; e += 256) {
                const int s = e >> 2, qq = e & 3;
                const int im = s / (HH * HWd), r = s - im * HH * HWd, hy = r / HWd, hx = r - hy * HWd;
                const int n = IDX ? simg[im] : n0 + im, y = y0 + hy - o.pt, x = x0 + hx - o.pl;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if ((IDX ? n >= 0 : n < p.n) && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
                    v = gen_ld4(o, cA, n, y, x, p.H, p.W, c0 + 4 * qq);
                *(f32x4 *)&halo[s * 16 + 4 * qq] = v;
            }
            for (int dy = 0; dy < o.kh; ++dy) {
                const int wy = o.flip ? o.kh - 1 - dy : dy;
                if (dy) __syncthreads();                   // (the previous tap row's MFMAs are done with wl)
                for (int e = tid; e < o.kw * 16 * NC; e += 256) {
                    const int dx = e >> (4 + LNC);
                    const int k = kfast ? (e & 15) : ((e >> LNC) & 15), nn = kfast ? ((e >> 4) & (NC - 1)) : (e & (NC - 1));
                    const int ci = c0 + k, co = co0 + nn;
                    float v = 0.f;
                    if (ci < o.C && co < p.Cout) {
                        const int wx = o.flip ? o.kw - 1 - dx : dx;
                        v = o.w[(size_t)(wy * o.kw + wx) * o.wtap + (size_t)ci * o.wk + (size_t)co * o.wn];
                    }
                    wl[((dx * 4 + (k >> 2)) * NC + nn) * 4 + (k & 3)] = v;
                }
                __syncthreads();
                const float *hrow = halo + ((img * HH + ty + dy) * HWd + tx) * 16 + 4 * q;
                for (int dx = 0; dx < o.kw; ++dx) {
                    const f32x4 av = *(const f32x4 *)(hrow + dx * 16);
                    f32x4 bv[NT];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bv[nt] = *(const f32x4 *)&wl[((dx * 4 + q) * NC + nt * 16 + i16) * 4];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[nt][s], acc[nt], 0, 0, 0);
                }
            }
        }
    }
    // (fewer than four tiles: the compiler carries the accumulators in VGPRs between the MFMA loops and would copy them
    // out of the AGPRs ahead of the drain -- they are operands of it, so the copies come after the wait)
    if constexpr (NT == 4) mfma_drain();
    else gen_drain_acc<NT>(acc);

    // ---- epilogue: lane holds rows 4q + r (pixels wave * 16 + 4q + r) of column i16 of the NT channel tiles ----
    [[maybe_unused]] float s1[NT] = {}, s2[NT] = {};
    [[maybe_unused]] float bias_r[NT];
    if constexpr (EPI == GEN_FWD) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { const int co = co0 + nt * 16 + i16; bias_r[nt] = co < p.Cout ? p.bias[co] : 0.f; }
        if (p.pool_out) __syncthreads();                   // (the halo becomes the pool buffer)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pp = wave * 16 + 4 * q + r;
        int im, py, px;
        gen_pix(g, pp, im, py, px);
        const int n = IDX ? simg[im] : n0 + im, y = y0 + py, x = x0 + px;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int cl = nt * 16 + i16, co = co0 + cl;
            float val = acc[nt][r];
            if constexpr (EPI == GEN_FWD) {
                val += bias_r[nt];
                if (p.pool_out) halo[pp * NC + cl] = val;
            }
            if ((IDX ? n < 0 : n >= p.n) || co >= p.Cout || y >= p.H || x >= p.W) continue;      // (beyond the batch, the channels, the map)
            const size_t idx = (((size_t)n * p.H + y) * p.W + x) * p.Cout + co;
            if constexpr (EPI == GEN_FWD) {
                p.out[idx] = val;
                s1[nt] += val;  s2[nt] = __builtin_fmaf(val, val, s2[nt]);      // (spelled out: the same rounding for every NT)
            } else if constexpr (EPI == GEN_DGH_RAW) {
                if (p.extra) val += p.extra[idx];
                if (p.acc_out) val += p.out[idx];
                p.out[idx] = val;
            } else if constexpr (EPI == GEN_DGH_BN) {
                const float *e = cE + cl * 5;
                const float ex = p.extra ? p.extra[idx] : 0.f;
                const float d = p.sprev[idx] - e[0];
                const float yv = __builtin_fmaf(d, e[2], e[3]);
                const float dz = yv > 0.f ? val + ex : 0.f;
                p.out[idx] = p.acc_out ? p.out[idx] + dz : dz;
                s1[nt] += dz;  s2[nt] = __builtin_fmaf(dz, d * e[1], s2[nt]);
            } else {  // GEN_DGV: val = gradient of the pooled finer map at coarse pixel (y, x)
                const float *e = cE + cl * 5;
                const size_t W2 = (size_t)p.W * 2;
                const size_t i00 = (((size_t)n * (p.H * 2) + 2 * y) * W2 + 2 * x) * p.Cout + co;
                const size_t ix[4] = {i00, i00 + p.Cout, i00 + W2 * p.Cout, i00 + W2 * p.Cout + p.Cout};
                float sv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) sv[k] = p.sprev[ix[k]];
                int arg = 0;  float mx = sv[0];
#pragma unroll
                for (int k = 1; k < 4; ++k) if (sv[k] > mx) { mx = sv[k]; arg = k; }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dzf = p.has_dz ? p.out[ix[k]] : 0.f;
                    const float xh = (sv[k] - e[0]) * e[1];
                    float gk = e[2] * (dzf - e[3] - xh * e[4]);
                    if (k == arg) gk += val;
                    p.out[ix[k]] = gk;
                }
            }
        }
    }
    if constexpr (EPI == GEN_FWD) {
        if (p.pool_out) {                                  // 2x2 max-pool of the tile (layer_types.py:185)
            __syncthreads();
            const int PSy = g.TSy / 2, PSx = g.TSx / 2;     // (H, W and the tile origins are even: no window straddles an edge)
            for (int e = tid; e < 16 * NC; e += 256) {
                const int c = e & (NC - 1), pq = e >> LNC;
                const int pim = pq / (PSy * PSx), pr = pq - pim * PSy * PSx, py = pr / PSx, px = pr - py * PSx;
                const float *q0 = halo + (pim * g.TSy * g.TSx + 2 * py * g.TSx + 2 * px) * NC + c;
                const float m4 = fmaxf(fmaxf(q0[0], q0[NC]), fmaxf(q0[g.TSx * NC], q0[g.TSx * NC + NC]));
                const int n = IDX ? simg[pim] : n0 + pim, co = co0 + c, oy = (y0 >> 1) + py, ox = (x0 >> 1) + px;
                if ((IDX ? n >= 0 : n < p.n) && co < p.Cout && oy < (p.H >> 1) && ox < (p.W >> 1))
                    p.pool_out[(((size_t)n * (p.H >> 1) + oy) * (p.W >> 1) + ox) * p.Cout + co] = m4;
            }
        }
    }
    if constexpr (EPI == GEN_FWD || EPI == GEN_DGH_BN) {
        double *dst = EPI == GEN_FWD ? p.out_sum : p.red_out;
        const int ns = EPI == GEN_FWD ? p.out_nslot : p.red_out_nslot;
        if (dst) {
            __syncthreads();                               // (wl becomes the reduction buffer)
            double *rb = (double *)wl;                     // [4 waves][NC channels][2]
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const double a1 = reduce_g4((double)s1[nt]), a2 = reduce_g4((double)s2[nt]);
                if (q == 0) { rb[(wave * NC + nt * 16 + i16) * 2] = a1;  rb[(wave * NC + nt * 16 + i16) * 2 + 1] = a2; }
            }
            __syncthreads();
            if (tid < NC && co0 + tid < p.Cout) {
                double a1 = 0.0, a2 = 0.0;
#pragma unroll
                for (int w = 0; w < 4; ++w) { a1 += rb[(w * NC + tid) * 2];  a2 += rb[(w * NC + tid) * 2 + 1]; }
                double *slot = dst + (size_t)(blockIdx.x % (unsigned)ns) * 2 * p.Cout;
                atomicAdd(slot + co0 + tid, a1);
                atomicAdd(slot + p.Cout + co0 + tid, a2);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Weight gradients.  grid (n_split, operand chunk x tap row, 64-channel output groups), 256 threads.
// ---------------------------------------------------------------------------
struct GenWP {
    GenOp op[2];  int nops;
    const float *g;  float *dw[2];  float *db;  long split_stride;
    int n, H, W, Cout, n_split;
    mpnn_act a;
};

constexpr int GEN_WHALO = 4 * 4 * (4 + GEN_KMAX - 1) * 16;                      // one tap row's halo, floats
static_assert(GEN_WHALO >= 8 * (8 + GEN_KMAX - 1) * 16, "wgrad halo buffer");
static_assert(GEN_WHALO >= 2 * 8 * (4 + GEN_KMAX - 1) * 16 && GEN_WHALO >= 2 * 4 * (8 + GEN_KMAX - 1) * 16,
              "wgrad halo buffer: 8x4 / 4x8 tiles of two images");

// GS: the g tile is loaded by scalars (Cout % 4 != 0: a pixel's channels are not 16-byte aligned; conv_gen_ch.hip).
template <bool GS = false>
__global__ __launch_bounds__(256) void gen_wgrad_k(const GenWP p) {
    __shared__ __attribute__((aligned(16))) float halo[GEN_WHALO];
    __shared__ __attribute__((aligned(16))) float gl[64 * 64];
    __shared__ float cA[3 * GEN_CMAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i16 = lane & 15, q = lane >> 4;
    const GenGeo g = gen_geo(p.n, p.H, p.W);
    const int split = blockIdx.x, co0 = blockIdx.z * 64, cw = wave * 16;
    // work item: (operand, 16-channel chunk, tap row)
    int item = blockIdx.y, part = 0;
    const int items0 = ((p.op[0].C + 15) / 16) * p.op[0].kh;
    if (item >= items0) { part = 1; item -= items0; }
    const GenOp o = p.op[part];
    const int c0 = (item / o.kh) * 16, dy = item % o.kh;
    const int HWd = g.TSx + o.kw - 1, nsl = g.TP * g.TSy * HWd;
    const bool db_owner = blockIdx.y == 0;
    gen_act_table(p.a, cA);

    f32x4 acc[GEN_KMAX];
#pragma unroll
    for (int dx = 0; dx < GEN_KMAX; ++dx) acc[dx] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;
    // halo offsets of the A columns this lane reads: pixel 4 ks + q of the tile, for the 16 k-steps
    int hoff[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        int im, py, px;
        gen_pix(g, 4 * ks + q, im, py, px);
        hoff[ks] = ((im * g.TSy + py) * HWd + px) * 16 + i16;
    }
    const long t_lo = (long)g.tiles * split / p.n_split, t_hi = (long)g.tiles * (split + 1) / p.n_split;
    for (long t = t_lo; t < t_hi; ++t) {
        int n0, y0, x0;
        gen_tile_origin(g, (int)t, n0, y0, x0);
        __syncthreads();                                   // (cA is ready; the previous tile's reads are done)
        for (int e = tid; e < nsl * 4; e += 256) {
            const int s = e >> 2, qq = e & 3;
            const int im = s / (g.TSy * HWd), r = s - im * g.TSy * HWd, hy = r / HWd, hx = r - hy * HWd;
            const int n = n0 + im, y = y0 + hy + dy - o.pt, x = x0 + hx - o.pl;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (n < p.n && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
                v = gen_ld4(o, cA, n, y, x, p.H, p.W, c0 + 4 * qq);
            *(f32x4 *)&halo[s * 16 + 4 * qq] = v;
        }
        for (int e = tid; e < 64 * 16; e += 256) {
            const int pp = e >> 4, cq = e & 15, co = co0 + 4 * cq;
            int im, py, px;
            gen_pix(g, pp, im, py, px);
            const int n = n0 + im, y = y0 + py, x = x0 + px;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};              // (a pixel beyond the map adds nothing to dW and db)
            if (n < p.n && co < p.Cout && y < p.H && x < p.W) {
                const float *src = p.g + (((size_t)n * p.H + y) * p.W + x) * p.Cout + co;
                if constexpr (GS) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = co + j < p.Cout ? src[j] : 0.f;
                } else {
                    v = *(const f32x4 *)src;
                }
            }
            *(f32x4 *)&gl[pp * 64 + 4 * cq] = v;
        }
        __syncthreads();
        if (db_owner && tid < 64)
            for (int pp = 0; pp < 64; ++pp) dbs += gl[pp * 64 + tid];
        if (co0 + cw < p.Cout) {                           // (uniform per wave)
            float bk[16];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) bk[ks] = gl[(4 * ks + q) * 64 + cw + i16];
#pragma unroll
            for (int dx = 0; dx < GEN_KMAX; ++dx) {
                if (dx >= o.kw) break;
#pragma unroll
                for (int ks = 0; ks < 16; ++ks)
                    acc[dx] = __builtin_amdgcn_mfma_f32_16x16x4f32(halo[hoff[ks] + dx * 16], bk[ks], acc[dx], 0, 0, 0);
            }
        }
    }
    mfma_drain();
    // lane holds dW[dy][dx][c0 + 4q + r][co0 + cw + i16]
    const int co = co0 + cw + i16;
    float *dw = p.dw[part] + (size_t)split * p.split_stride;
    if (co < p.Cout) {
#pragma unroll
        for (int dx = 0; dx < GEN_KMAX; ++dx) {
            if (dx >= o.kw) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = c0 + 4 * q + r;
                if (ci < o.C) dw[((size_t)(dy * o.kw + dx) * o.C + ci) * p.Cout + co] = acc[dx][r];
            }
        }
    }
    if (db_owner && tid < 64 && co0 + tid < p.Cout) p.db[(size_t)split * p.split_stride + co0 + tid] = dbs;
}

// ------------------------------- host side, shared by the three families -------------------------------
enum { GEN_FAM_GEN = 0, GEN_FAM_HW = 1, GEN_FAM_CH = 2 };
// conv_gen.hip: record checks and launches of every family (fam picks the shape check and the tiles per wave)
int gen_fwd(int fam, const mpnn_conv_fwd_args *a, int kh, int kw, int kvh, int kvw, void *stream);
int gen_dgrad_horz(int fam, const mpnn_dgrad_horz_args *a, int kh, int kw, void *stream);
int gen_dgrad_vert(int fam, const mpnn_dgrad_vert_args *a, int kvh, int kvw, void *stream);
int gen_wgrad(int fam, const mpnn_wgrad_args *a, int kh, int kw, int kvh, int kvw, void *stream);
// conv_gen_ch.hip: the shape check of the any-channel family, its kernels with nt = 1 or 2 output tiles per wave (list:
// the forward kernel on a sample list), and the weight-gradient kernel with scalar g loads
int gen_ch_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw);
int gen_ch_launch(int epi, bool list, int nt, const GenP &p, dim3 grid, hipStream_t stream);
int gen_ch_wgrad_launch(const GenWP &p, dim3 grid, hipStream_t stream);
