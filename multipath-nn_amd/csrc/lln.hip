// mpnn_lln_fwd: MultiscaleLLN (reference layer_types.py:127-147) -- every scale of the input pyramid divided by its
// Gaussian-weighted local mean luminance plus eps.  One launch: all scales, all samples, all records of a table.
//
// A workgroup owns one (record, sample, scale, tile of LLN_T x LLN_T pixels):
//   1. luminance Y = 0.2126 r + 0.7152 g + 0.0722 b of the tile plus a halo of `radius` into LDS, zero outside the map
//      (SAME padding).  Scale i is read from the input image through ToPyramid's strided pick x[r << i][c << i]: the
//      pyramid is never materialised;
//   2. horizontal pass over the 2 * radius + 1 taps into LDS, taps in the order v = -radius .. radius;
//   3. vertical pass in the same order, then m = lum / (dr[r] * dc[c]) and the denominator m + eps into LDS.  dr / dc
//      are the sums of the taps that fall inside the map on each axis (the density of the reference is their product),
//      read as differences of the taps' prefix sums, which the host adds up in double;
//   4. out = x / (m + eps), IEEE division, for the three channels: one dword store per lane, coalesced over the tile row.
// A pixel's summation order is fixed and the out-of-map terms are exact zeros, so its value depends on its own image
// alone -- not on the tile it falls in, the batch size or the record's place in the table.  No atomics.
#include "common.h"

#define LLN_T 32                         // tile side (pixels)
#define LLN_S MPNN_LLN_MAX_RADIUS
#define LLN_E (LLN_T + 2 * LLN_S)        // tile + halo
#define LLN_THREADS 256

struct lln_params {
    int n_max, H, W, n_scales, radius, tiles_total;
    int tile_start[MPNN_LLN_MAX_SCALES + 1];     // first tile of scale i among the tiles of one sample
    float tap[2 * LLN_S + 1];
    float cum[2 * LLN_S + 2];                    // cum[k] = tap[0] + ... + tap[k - 1]
};

__global__ __launch_bounds__(LLN_THREADS) void lln_fwd_k(const mpnn_lln_args *__restrict__ table, const lln_params p) {
    __shared__ float Y[LLN_E][LLN_E + 1];        // luminance with halo; later the denominators of the tile
    __shared__ float Hs[LLN_E][LLN_T];           // after the horizontal pass
    __shared__ float tap[2 * LLN_S + 1], cum[2 * LLN_S + 2];
    const int tid = threadIdx.x;
    const int t_all = blockIdx.x % p.tiles_total;
    const int sample = (blockIdx.x / p.tiles_total) % p.n_max;
    const mpnn_lln_args *__restrict__ a = table + blockIdx.x / p.tiles_total / p.n_max;
    if (sample >= a->n) return;                  // (uniform over the workgroup)
    int i = 0;
    while (i + 1 < p.n_scales && t_all >= p.tile_start[i + 1]) ++i;
    const int s = p.radius, h = p.H >> i, w = p.W >> i;
    const int tiles_x = (w + LLN_T - 1) / LLN_T, t = t_all - p.tile_start[i];
    const int r0 = (t / tiles_x) * LLN_T, c0 = (t % tiles_x) * LLN_T;
    const int th = min(LLN_T, h - r0), tw = min(LLN_T, w - c0);
    const int eh = th + 2 * s, ew = tw + 2 * s;
    const float *__restrict__ x = a->x + (size_t)sample * p.H * p.W * 3;
    float *__restrict__ out = a->out[i] + (size_t)sample * h * w * 3;
    const float eps = a->eps;

    if (tid < 2 * s + 1) tap[tid] = p.tap[tid];
    if (tid < 2 * s + 2) cum[tid] = p.cum[tid];
    for (int k = tid; k < eh * ew; k += LLN_THREADS) {
        const int rr = k / ew, cc = k - rr * ew;
        const int r = r0 - s + rr, c = c0 - s + cc;
        float y = 0.f;
        if (r >= 0 && r < h && c >= 0 && c < w) {
            const float *px = x + ((size_t)(r << i) * p.W + (c << i)) * 3;
            y = fmaf(0.0722f, px[2], fmaf(0.7152f, px[1], 0.2126f * px[0]));
        }
        Y[rr][cc] = y;
    }
    __syncthreads();
    for (int k = tid; k < eh * tw; k += LLN_THREADS) {
        const int rr = k / tw, c = k - rr * tw;
        float acc = 0.f;
        for (int v = 0; v <= 2 * s; ++v) acc = fmaf(tap[v], Y[rr][c + v], acc);
        Hs[rr][c] = acc;
    }
    __syncthreads();
    for (int k = tid; k < th * tw; k += LLN_THREADS) {
        const int rr = k / tw, cc = k - rr * tw;
        const int r = r0 + rr, c = c0 + cc;
        float lum = 0.f;
        for (int u = 0; u <= 2 * s; ++u) lum = fmaf(tap[u], Hs[rr + u][cc], lum);
        // taps u - s with 0 <= r + u - s < h (and the same for the columns)
        const float dr = cum[min(2 * s, h - 1 - r + s) + 1] - cum[max(0, s - r)];
        const float dc = cum[min(2 * s, w - 1 - c + s) + 1] - cum[max(0, s - c)];
        Y[rr][cc] = lum / (dr * dc) + eps;         // (Y's halo is dead: every wave is past the horizontal pass)
    }
    __syncthreads();
    for (int k = tid; k < th * tw * 3; k += LLN_THREADS) {
        const int rr = k / (tw * 3), e = k - rr * (tw * 3), cc = e / 3, ch = e - cc * 3;
        const int r = r0 + rr, c = c0 + cc;
        out[((size_t)r * w + c) * 3 + ch] = x[((size_t)(r << i) * p.W + (c << i)) * 3 + ch] / Y[rr][cc];
    }
}

extern "C" int mpnn_lln_fwd(const mpnn_lln_args *dev_table, int count, const mpnn_lln_geom *geom, void *stream) {
    if (!dev_table || !geom || count < 1 || geom->n_max < 1) return MPNN_E_ARG;
    const int S = geom->n_scales, s = geom->radius, H = geom->H, W = geom->W;
    if (s < 1 || s > MPNN_LLN_MAX_RADIUS || S < 1 || S > MPNN_LLN_MAX_SCALES) return MPNN_E_SHAPE;
    if (H < 1 || H > 256 || W < 1 || W > 256 || H % (1 << (S - 1)) || W % (1 << (S - 1))) return MPNN_E_SHAPE;
    lln_params p = {};
    p.n_max = geom->n_max; p.H = H; p.W = W; p.n_scales = S; p.radius = s;
    for (int i = 0; i < S; ++i) {
        p.tile_start[i] = p.tiles_total;
        p.tiles_total += (((H >> i) + LLN_T - 1) / LLN_T) * (((W >> i) + LLN_T - 1) / LLN_T);
    }
    p.tile_start[S] = p.tiles_total;
    double c = 0.0;
    for (int k = 0; k <= 2 * s; ++k) {
        p.tap[k] = geom->tap[k];
        p.cum[k] = (float)c;
        c += (double)geom->tap[k];
    }
    p.cum[2 * s + 1] = (float)c;
    const long long wgs = (long long)p.tiles_total * geom->n_max * count;
    if (wgs > 0x7fffffffLL) return MPNN_E_SHAPE;
    hipLaunchKernelGGL(lln_fwd_k, dim3((unsigned)wgs), dim3(LLN_THREADS), 0, (hipStream_t)stream, dev_table, p);
    MPNN_LAUNCH_CHECK();
    return 0;
}
