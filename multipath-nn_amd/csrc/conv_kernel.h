// Direct (im2col-free) 3x3 SAME convolution on v_mfma_f32_16x16x4_f32 for gfx950.
//
// One template serves the forward conv of a MultiscaleConvMax scale and both
// input-gradient convs (they are the same contraction with a transposed,
// tap-flipped weight pack); what differs is the operand transform applied while
// staging and the epilogue:
//
//   EPI_FWD      out = bias + conv(act(a)) [+ conv(maxpool2(v))], BN sum/sumsq
//   EPI_DGH_BN   dz = [y>0] * (conv^T(g) [+ extra]),  BN-backward reductions
//   EPI_DGH_RAW  dy = conv^T(g) [+ extra]
//   EPI_DGV      g_fine = bn_bwd(dz_fine) + maxpool_bwd(conv^T(g))
//
// Implicit GEMM: M = output pixels, N = output channels, K = 9 taps x input
// channels.  A workgroup (4 waves) owns a tile of 64 output pixels x CT output
// channels.  Input channels are processed in chunks of 16: the chunk's halo
// tile is staged into LDS as 4 "planes" of float4 (4 consecutive channels of
// one pixel per 16-byte slot, layout [plane][halo pixel]), so that ONE
// ds_read_b128 gives a lane the A operands of four consecutive MFMAs (MFMA j
// of the group contracts channels {4g+j}, g = lane>>4), and the k-interleaved
// weight pack gives the matching B operands with ONE global_load_dwordx4
// (L2-resident, no LDS staging, no barrier inside the 9-tap loop).
//
// Bank conflicts: ds_read_b128 is served in 16-lane groups that mix lanes of
// two g values; with the plane stride P a multiple of 16 slots and the 16
// pixels of an M-tile on distinct slots mod 16 (row stride R chosen per
// geometry) every read is conflict-free; staging writes put 8 consecutive
// pixels of one plane in the 8 lanes of a ds_write_b128 group.
#pragma once
#include "common.h"
#include <cstdlib>

enum { EPI_FWD = 0, EPI_DGH_BN = 1, EPI_DGH_RAW = 2, EPI_DGV = 3 };

// Ablation bits (skip the MFMAs / the staging / the epilogue of a unit; tools/ablate_conv.py): compiled in only with
// -DMPNN_ABLATE -- as run-time tests they put five uniform branches into every unit of every production kernel.
#ifdef MPNN_ABLATE
#define MPNN_DBG(p, bit) ((p).dbg & (bit))
#else
#define MPNN_DBG(p, bit) 0
#endif

// (every pointer global-typed, see gptr in common.h: the grouped launches read these records from device memory)
struct ConvP {
    ActG a;                     // operand A (identity transform for dgrad)
    gptr<const float> v;  int Cv;    // operand V: the finer scale's pre-BN map, ALREADY 2x2-max-pooled by its producer
    gptr<const float> wa, wv;   // weight packs
    int n, H, W, Cout;
    gptr<const float> bias;  gptr<float> out;  gptr<double> out_sum;      // EPI_FWD
    gptr<float> pool_out;                                   // EPI_FWD: 2x2 max-pool of `out` (NULL: none)
    gptr<const float> extra;                                // EPI_DGH_*
    gptr<const float> sprev;  ActG pbn;  gptr<double> red_out;    // EPI_DGH_BN / EPI_DGV
    gptr<const double> red;  int has_dz;  int red_nslot;    // EPI_DGV
    int out_nslot;                                          // slots of out_sum / red_out
    // operand A = BatchNorm backward of dz (mpnn_bn_bwd_apply on load): A = k1*(dz - r0 - xhat*r1)
    gptr<const float> ga_s;  ActG ga_bn;  gptr<const double> ga_red;  int ga_nslot;  int ga_on;
    int n_tiles;                                            // set by the launcher
    int dbg;                                                // ablation mask (MPNN_CONV_DBG): only read in -DMPNN_ABLATE builds
    // Routed evaluation (IDX bodies): sample slot s of this launch is image idx[s] of EVERY buffer
    // (inputs, outputs, pooled map); `n` is then the device-side count of slots.  The gather and the
    // scatter are this indirection in the tile loader and the epilogue: no sub-batch is materialised.
    gptr<const int> idx;
    int acc_out;                                            // EPI_DGH_*: out += result (several child blocks)
    // XCD-aware tile order (set by the launcher when the row has a multiple of 8 workgroups): workgroups are dealt
    // round-robin to the 8 XCDs (blockIdx % 8), each XCD has its own L2, and a tile's producer in the previous
    // launch left its output in the L2 of the XCD it ran on.  With xcd set, image n is ALWAYS processed on XCD
    // (n / 4) % 8 -- in every launch, whatever the map size -- so a tile's inputs (the same images) are found
    // in the local L2.  Speed only: any placement gives the same results.
    int xcd;
};

// Tile j (0 .. n_tiles / 8) of XCD x under the image -> XCD rule above (n % 32 == 0).
template <int GK>
__device__ __forceinline__ int xcd_tile(int j, int x, int tpi) {
    if (GK == 2) return 8 * j + x;                          // a tile = images 4t .. 4t + 3
    const int ij = GK == 0 ? j / tpi : j, inner = GK == 0 ? j - ij * tpi : 0;
    const int n = ((ij >> 2) << 5) + 4 * x + (ij & 3);      // image: 32 q + 4 x + i
    return n * tpi + inner;
}

// Geometry kinds.  TH x TW output pixels per image x IMG images = 64 pixels;
// an M-tile is 16 of them.  R = LDS row stride (slots), P = plane stride.
// The small-map geometries use DENSE halo rows (R = halo width): two of the 16
// lanes of a ds_read_b128 group then share a bank (one extra LDS cycle per read),
// in exchange for half the LDS footprint -> 4 instead of 2 workgroups per CU for
// kernels that are bound by latency, not by LDS bandwidth.
template <int GK> struct Geom;
template <> struct Geom<0> { static constexpr int TH = 4, TW = 16, IMG = 1, R = 18, P = 112; };  // W % 16 == 0
template <> struct Geom<1> { static constexpr int TH = 8, TW = 8,  IMG = 1, R = 10, P = 112; };  // 8 x 8 maps
template <> struct Geom<2> { static constexpr int TH = 4, TW = 4,  IMG = 4, R = 6,  P = 144; };  // 4 x 4 maps

template <int GK>
__device__ __forceinline__ void mtile_pix(int m, int i, int &img, int &ty, int &tx) {
    if (GK == 0) { img = 0; ty = m; tx = i; }
    else if (GK == 1) { img = 0; ty = 2 * m + (i >> 3); tx = i & 7; }
    else { img = m; ty = i >> 2; tx = i & 3; }
}

template <int GK>
__device__ __forceinline__ void tile_origin(const ConvP &p, int bid, int &n0, int &y0, int &x0) {
    if (GK == 0) {
        const int tx_n = p.W >> 4, tpi = tx_n * (p.H >> 2);
        n0 = bid / tpi;
        const int rem = bid - n0 * tpi;
        const int ty = rem / tx_n;
        y0 = ty * 4; x0 = (rem - ty * tx_n) * 16;
    } else if (GK == 1) { n0 = bid; y0 = 0; x0 = 0; }
    else { n0 = bid * 4; y0 = 0; x0 = 0; }
}

template <int GK>
__host__ __device__ static inline int conv_grid_x(int n, int H, int W) {
    if (GK == 0) return n * (W >> 4) * (H >> 2);
    if (GK == 1) return n;
    return (n + 3) >> 2;
}

// ---------------------------------------------------------------------------
// Staging: global -> registers (RAW, no arithmetic, so the loads stay in flight
// under the MFMAs of the unit being computed) and registers -> LDS (transform
// applied here).  An "item" is one float4 slot of the halo tile: item i of a
// thread block maps to (plane q, halo pixel hp) with 8 consecutive pixels of
// one plane in 8 consecutive lanes (conflict-free ds_write_b128 groups, 512-B
// contiguous global segments).
// MODE 0: operand A (optional BN+ReLU, optional pyramid subsampling); MODE 1:
// operand V (the finer scale's map, max-pooled once by its producer's epilogue);
// MODE 2: BatchNorm backward of dz (two float4 per item: dz and s).
// ---------------------------------------------------------------------------
// On the 8x8 and 4x4 maps a tile IS a whole image (four of them on the 4x4 maps): the halo ring is always
// outside the image, i.e. always zero.  Those geometries stage the 64 INTERIOR pixels only (64 x 4 planes = one
// item per thread instead of two / three) and the ring slots of the LDS tiles are zeroed once per kernel
// (zero_halo) and never written again -- the staging work of the chain-bound small-map launches drops by 2-3x.
template <int GK> struct XItems {
    using G = Geom<GK>;
    static constexpr bool INTERIOR = GK != 0;
    static constexpr int HR = G::TH + 2, HC = G::TW + 2;
    static constexpr int NHP = INTERIOR ? G::IMG * G::TH * G::TW : G::IMG * HR * HC, NHP8 = (NHP + 7) & ~7;
    static constexpr int N = (NHP8 * 4 + 255) / 256;      // items per thread
};
// zero `count` float4 slots of LDS with all `nthreads` threads (a whole tile buffer: the caller puts a barrier
// between this and the first interior store)
__device__ __forceinline__ void zero_halo(f32x4 *lds, int count, int tid, int nthreads) {
    for (int i = tid; i < count; i += nthreads) lds[i] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// the same for `planes` planes of stride PS, but ONLY the slots interior staging never writes (the halo ring and the
// padding behind the frame): no ordering against the interior stores is needed
template <int GK, int PS>
__device__ __forceinline__ void zero_ring(f32x4 *lds, int planes, int tid, int nthreads) {
    using G = Geom<GK>;
    constexpr int HR = G::TH + 2, FR = G::IMG * HR * G::R;        // slots of the halo frame of one plane
    for (int i = tid; i < planes * PS; i += nthreads) {
        const int t = i % PS;
        bool ring = t >= FR;
        if (!ring) {
            const int r = t % (HR * G::R), hy = r / G::R, hx = r - hy * G::R;
            ring = hy == 0 || hy == HR - 1 || hx == 0 || hx > G::TW;
        }
        if (ring) lds[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---------------------------------------------------------------------------
// Lean staging (conv_body; wgrad_body in bwd_bodies.h does the same).  Everything about an item that does not depend on the tile (its LDS
// slot, its halo pixel) is computed ONCE per kernel (ItemK); everything that depends on the tile
// but not on the channel chunk (pixel index, in-bounds bit) once per TILE (TileGeo); a unit then
// costs one multiply-add per item for its address.  (x_item recomputed all of it for every item
// of every unit, twice: ~40% of a unit's instructions on the deep 4x4 layers.)
// ---------------------------------------------------------------------------
// Branch- and table-free selects on a 0/1 flag (hipcc turned `flag ? x : y` on loop-varying uniform
// flags into a lookup table in SCRATCH memory, i.e. a memory load per use inside the pipeline).
__device__ __forceinline__ int sel_i(int flag, int a, int b) { const int m = -flag; return (a & ~m) | (b & m); }
// (pointer form: an offset from `a`, so the result stays a GLOBAL pointer -- through an integer cast
// the compiler lost the address space and emitted flat loads, which also count against lgkmcnt and
// made every LDS wait of the MFMA loop wait for the prefetch as well)
template <class P>
__device__ __forceinline__ P sel_p(int flag, P a, P b) {
    const long delta = pcast<const char>(b) - pcast<const char>(a);       // (loop-invariant at every call site)
    return pcast<const float>(pcast<const char>(a) + (delta & -(long)flag));
}
template <int GK> struct ItemK {
    static constexpr int N = XItems<GK>::N;
    int slot[N];            // float4 index in the LDS tile (plane included)
    int geo[N];             // img << 16 | hy << 8 | hx  of the halo pixel
    unsigned ok;            // bit k: item k exists
    int q;                  // channel quad (LDS plane) of all items of this thread
};
template <int GK, int PS>
__device__ __forceinline__ void item_consts(ItemK<GK> &ik, int tid) {
    using X = XItems<GK>;
    using G = Geom<GK>;
    ik.ok = 0;
    ik.q = (tid >> 3) & 3;                         // (256 k >> 3) & 3 == 0: the same for every k
#pragma unroll
    for (int k = 0; k < X::N; ++k) {
        const int i = tid + k * 256;
        const int hp = ((i >> 5) << 3) + (i & 7);
        const bool ok = hp < X::NHP;
        const int hq = ok ? hp : 0;
        int img, hy, hx;
        if (X::INTERIOR) {                             // interior pixel hq of the tile -> its place inside the halo frame
            img = hq / (G::TH * G::TW);
            const int rem = hq - img * (G::TH * G::TW);
            hy = rem / G::TW + 1; hx = rem % G::TW + 1;
        } else {
            img = hq / (X::HR * X::HC);
            const int rem = hq - img * (X::HR * X::HC);
            hy = rem / X::HC; hx = rem - hy * X::HC;
        }
        ik.slot[k] = ik.q * PS + (img * X::HR + hy) * G::R + hx;
        ik.geo[k] = (img << 16) | (hy << 8) | hx;
        ik.ok |= (ok ? 1u : 0u) << k;
    }
}
template <int GK, bool SHIFTED> struct TileGeo {
    static constexpr int N = XItems<GK>::N;
    int pix[N];                       // (n*H + y)*W + x of the halo pixel (0 when out of range)
    int pixs[SHIFTED ? N : 1];        // the same in the un-subsampled pyramid input (ToPyramid's pick)
    // BYTE offset of the item's float4 in operand A / operand V (pixel * channels + this thread's channel quad; 0 when
    // out of range): a unit's load address is then scalar base (+ chunk) + one of these -- no vector arithmetic per
    // unit.  (fp32 MFMAs and vector instructions share the SIMD's ALUs on gfx950: their times ADD, profiles/
    // r06_mfma_loop_probe.txt, and address arithmetic was most of the 4-6 vector instructions per MFMA.)
    unsigned offa[N], offv[N];
    unsigned inb;                     // bit k: pixel inside the image and the batch
};
// Image of slot `img` of a tile: a mask select over the (uniform) table im[] -- a `?:` chain on a
// lane-varying index was compiled to a scratch-memory table.
template <int IMG>
__device__ __forceinline__ int pick_img(const int *im, int img) {
    int r = im[0];
#pragma unroll
    for (int j = 1; j < IMG; ++j) { const int m = -(int)(img == j); r = (r & ~m) | (im[j] & m); }
    return r;
}
// im != nullptr (routed evaluation): im[j] = image behind slot n0 + j of the tile.
template <int GK, bool SHIFTED>
__device__ __forceinline__ void tile_geo(TileGeo<GK, SHIFTED> &tg, const ItemK<GK> &ik, const ConvP &p, int n0, int y0, int x0,
                                         const int *im = nullptr, const int aC = 0, const int vC = 0) {
    tg.inb = 0;
#pragma unroll
    for (int k = 0; k < ItemK<GK>::N; ++k) {
        const int slot = n0 + (ik.geo[k] >> 16), y = y0 + ((ik.geo[k] >> 8) & 255) - 1, x = x0 + (ik.geo[k] & 255) - 1;
        // (interior staging: y, x are inside the image by construction)
        const bool ok = ((ik.ok >> k) & 1) && slot < p.n &&
                        (XItems<GK>::INTERIOR || ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W));
        const int n = im ? pick_img<Geom<GK>::IMG>(im, ik.geo[k] >> 16) : slot;
        tg.pix[k] = ok ? (n * p.H + y) * p.W + x : 0;
        tg.offa[k] = ok ? (unsigned)(tg.pix[k] * aC + ik.q * 4) * 4u : 0u;
        tg.offv[k] = ok ? (unsigned)(tg.pix[k] * vC + ik.q * 4) * 4u : 0u;
        if (SHIFTED) {
            const int sh = p.a.shift;
            tg.pixs[k] = ok ? (n * (p.H << sh) + (y << sh)) * (p.W << sh) + (x << sh) : 0;
        }
        tg.inb |= (ok ? 1u : 0u) << k;
    }
}
// Raw loads of one 16-channel chunk.  NO control flow around the loads and the same number of loads
// whatever the operand: the compiler can then count them and wait with vmcnt(N > 0) for an OLDER
// unit while this one stays in flight (behind a branch it falls back to vmcnt(0), which drains the
// prefetch that was just issued: the waves sat in s_waitcnt 60% of the time).
//   KIND 0: forward, operand A or V selected by `part` (pointer/stride select, one load per item)
//   KIND 1: forward, 1- or 3-channel pyramid image as operand A (scalar loads) / V (vector)
//   KIND 2: dgrad: dz and, when BatchNorm-backward is applied on load, s
template <int GK, int KIND, int XW, bool SHIFTED>
__device__ __forceinline__ void ld_items(f32x4 (*xr)[XW], const ConvP &p, const TileGeo<GK, SHIFTED> &tg, const ItemK<GK> &ik,
                                         int part, int c0, int np, gptr<const float> src, int C, const bool odd_c) {
    static_assert(KIND != 2 || XW >= 2, "dgrad staging keeps two raw registers per item");
    const int c = c0 + ik.q * 4;
    const bool qin = ik.q < np;
    if (KIND == 1 && part == 0) {                  // (block 0 only)
#pragma unroll
        for (int k = 0; k < ItemK<GK>::N; ++k) {
            const bool live = qin && ((tg.inb >> k) & 1);
            const int base = live ? (SHIFTED ? tg.pixs[k] : tg.pix[k]) * C : 0;
            if ((C & 3) == 0) xr[k][0] = *pcast<const f32x4>(p.a.x + base + (live ? c : 0));
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) xr[k][0][j] = p.a.x[base + (live && c + j < C ? c + j : 0)];
            }
        }
        return;
    }
    // UNSIGNED 32-bit byte offset from a uniform base: the load takes the scalar-base + 32-bit-offset form (a signed
    // element offset costs a sign extension and a 64-bit shift-add per load; the host keeps every activation tensor
    // below 4 GB).  The chunk's channel offset goes into the SCALAR base, the per-thread part was computed with the tile.
    const gptr<const char> sb = pcast<const char>(src) + (size_t)c0 * 4, sb2 = pcast<const char>(p.ga_s) + (size_t)c0 * 4;
    (void)c;
#pragma unroll
    for (int k = 0; k < ItemK<GK>::N; ++k) {
        unsigned off = (KIND != 2 && part) ? tg.offv[k] : tg.offa[k];
        if (odd_c) off = qin ? off : 0u;           // (uniform: a channel count that is not a multiple of 16 somewhere)
        xr[k][0] = ld_at<f32x4>(sb, off);
        if (KIND == 2 && p.ga_on) xr[k][1 % XW] = ld_at<f32x4>(sb2, off);      // (uniform)
    }
}
// transform + LDS store of one chunk; `inb` is the tile's in-bounds mask the chunk was loaded with
template <int GK, int MODE, int XW>
__device__ __forceinline__ void st_items(f32x4 *tile, const f32x4 (*xr)[XW], const ConvP &p, const float *cA,
                                         unsigned inb, const ItemK<GK> &ik, int c0, int np) {
    const int c = c0 + ik.q * 4;
    const bool qin = ik.q < np;
    float cc[4][5];
    if (MODE == 2) {                               // cA rows: m, rstd, k1, r0, r1
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 5; ++e) cc[j][e] = cA[(c + j) * 5 + e];
    } else if (MODE == 0 && p.a.mode != MPNN_ACT_IDENTITY) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 3; ++e) cc[j][e] = cA[(c + j) * 3 + e];
    }
#pragma unroll
    for (int k = 0; k < ItemK<GK>::N; ++k) {
        // branch-free: transform whatever was loaded, then select (one exec-masked store at the end)
        const bool live = qin && ((inb >> k) & 1);
        f32x4 v = xr[k][0];
        if (MODE == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (xr[k][1 % XW][j] - cc[j][0]) * cc[j][1];
                v[j] = cc[j][2] * (xr[k][0][j] - cc[j][3] - xh * cc[j][4]);
            }
        } else if (MODE == 0) {
            if (p.a.mode != MPNN_ACT_IDENTITY) {       // uniform
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fmaxf((v[j] - cc[j][0]) * cc[j][1] + cc[j][2], 0.f);
            }
            if (p.a.C & 3) {                           // uniform (a live quad of a count % 4 == 0 has all four channels)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (c + j < p.a.C) ? v[j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = live ? v[j] : 0.f;
        if ((ik.ok >> k) & 1) tile[ik.slot[k]] = v;
    }
}

// ---------------------------------------------------------------------------
// The kernel.  A workgroup is persistent over its share of the 64-pixel tiles;
// its work is a sequence of units (tile, operand part, 16-channel chunk).  LDS
// is double-buffered: while the MFMAs of unit u read buffer u&1, the raw global
// loads of unit u+1 are in flight, and they are transformed and written to the
// other buffer before the single barrier that ends the unit.
// ---------------------------------------------------------------------------
template <int WNT> struct CT_OK { static constexpr bool v = WNT == 1; };      // (the K-split exchange holds 16-channel tiles)
// The 32-channel output tiles keep ONE weight buffer instead of two, at the price of a second LDS barrier per unit (the next
// unit's weights may only be stored once every wave has read this unit's).  Their two weight buffers were 36 KB of the 58 KB
// that kept them at two workgroups per CU; with one buffer (40 KB: three per CU) and units of 72 MFMAs per wave the second
// barrier is cheap.  Same arithmetic, bit-identical results.  (An A/B switch until round 6; result: dense evaluation at 4 096
// images 2.127 -> 2.063 ms, routed 1.530 -> 1.480 ms, 8 192: 3.990 -> 3.882 / 2.653 -> 2.581 ms.  One buffer for every tile
// width -- 31.5 instead of 40.8 KB, five instead of three workgroups per CU -- was a second switch, left off.)
template <int CT> struct WtSingle { static constexpr bool v = CT == 32; };
// LDS bytes of one workgroup (all variants of a launch share one arena).
template <int GK, int WM, int CT, int NCH = 1>
struct ConvSmem {
    // POOL: the 2x2-pooling exchange [64 px][CT]; the K-split bodies' partial-sum exchange (4 KB) shares it
    static constexpr int TILE = NCH * 2 * 4 * Geom<GK>::P * 16, WT = NCH * (WtSingle<CT>::v ? 1 : 2) * 36 * CT * 16, CA = 128 * 5 * 4, CE = CT * 5 * 4,
                         RED = WM * CT * 2 * 8, POOL = 64 * CT * 4;
    static constexpr int BYTES = TILE + WT + CA + ((CE + 15) & ~15) + RED + POOL;
};

// NCH = 16-channel chunks per unit (1 or 2).  With 2 a unit spans 32 input channels: half as many
// barriers and load round trips on the deep-K, small-M layers whose per-unit MFMA time (~0.5 us)
// cannot cover a load latency (~2 us).  Requires every operand's channel count % 32 == 0.
// KSPLIT (with NCH == 2, 512 threads): the workgroup's two 256-thread groups each stage and multiply ONE
// of the unit's two chunks; their partial sums meet in LDS when a tile is finished.  For the deep 4x4 /
// 8x8 layers, whose 128-256 workgroups otherwise leave one wave per SIMD with nothing to overlap.
// IDX (forward only): routed evaluation -- the tile's image slots go through p.idx (see ConvP).
template <int GK, int MT, int NT, int WM, int WN, bool SMALL_A, int EPI, int NCH = 1, bool KSPLIT = false, bool IDX = false>
__device__ __forceinline__ void conv_body(const ConvP &p, const int bx, const int by, const int gx, char *smem) {
    static_assert(!KSPLIT || (NCH == 2 && MT == 1 && NT == 1 && !SMALL_A && EPI == EPI_FWD && CT_OK<WN * NT>::v), "K-split: forward, 32-channel units");
    static_assert(!IDX || (EPI == EPI_FWD && !KSPLIT), "index lists: forward bodies of the evaluation path");
    constexpr int SC = KSPLIT ? 1 : NCH;            // chunks staged / multiplied by ONE thread group per unit
    using G = Geom<GK>;
    constexpr int P = G::P, R = G::R, HR = G::TH + 2;
    constexpr int CT = WN * NT * 16;
    constexpr int XW = EPI == EPI_FWD ? 1 : 2;      // dgrad: dz + s when BatchNorm-backward is applied on load
    constexpr int XN = XItems<GK>::N;
    static_assert(WM * WN == 4 && WM * MT == 4, "4 waves, 4 M-tiles per workgroup");

    constexpr int BI = 36 * CT;                     // float4 items of one weight chunk: [9 taps][4 g][CT]
    constexpr int BN = (BI + 255) / 256;
    using SM = ConvSmem<GK, WM, CT, NCH>;
    f32x4 (*tile)[NCH * 4 * P] = (f32x4 (*)[NCH * 4 * P])smem;
    f32x4 (*wtile)[NCH * BI] = (f32x4 (*)[NCH * BI])(smem + SM::TILE);
    float *cA = (float *)(smem + SM::TILE + SM::WT);
    float *cE = cA + 128 * 5;
    double *redbuf = (double *)(smem + SM::TILE + SM::WT + SM::CA + ((SM::CE + 15) & ~15));
    float *pool_lds = (float *)(smem + SM::TILE + SM::WT + SM::CA + ((SM::CE + 15) & ~15) + SM::RED);   // [64 px][CT]

    trace_stamp(0);
    const int tid = KSPLIT ? (threadIdx.x & 255) : threadIdx.x, lane = tid & 63;
    const int kg = KSPLIT ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 8) : 0;      // K-group of this wave
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int wm = wid / WN, wn = wid - wm * WN;
    const int co0 = by * CT;
    const int cw = co0 + wn * NT * 16 + li;          // this lane's first output channel


    float bias_r[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bias_r[nt] = (EPI == EPI_FWD) ? p.bias[cw + nt * 16] : 0.f;
    int slot0[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int img, ty, tx;
        mtile_pix<GK>(wm * MT + mt, li, img, ty, tx);
        slot0[mt] = (img * HR + ty) * R + tx;
    }
    // (operand V -- the pooled finer map -- exists in forward convs only: for the input-gradient bodies every
    // operand select below folds to operand A at compile time)
    constexpr bool HAS_V = EPI == EPI_FWD;
    const int nchA = (p.a.C + 15) >> 4, nchV = (HAS_V && p.v) ? ((p.Cv + 15) >> 4) : 0;
    const int upt = (nchA + nchV) / NCH;            // NCH == 2: both counts are even (host-checked)

    // tile sequence of this workgroup: t = sq0, sq0 + sqd, ... < sqn; XCD-aware launches number the tiles of
    // their own XCD (xcd_tile), the others all tiles
    const bool xa = p.xcd != 0 && (p.n & 31) == 0 && (gx & 7) == 0;      // (uniform)
    const int xcd_id = blockIdx.x & 7;
    const int tpi = GK == 0 ? (p.W >> 4) * (p.H >> 2) : 1;
    const int sq0 = xa ? (bx >> 3) : bx, sqd = xa ? (gx >> 3) : gx, sqn = xa ? (p.n_tiles >> 3) : p.n_tiles;
    const int my_tiles = (sq0 < sqn) ? (sqn - 1 - sq0) / sqd + 1 : 0;
    const int n_units = my_tiles * upt;

    // ---- staging: one unit = NCH 16-channel chunks of operand A or V plus its weight chunk ----
    ItemK<GK> ik;
    item_consts<GK, P>(ik, tid);
    // weight item k of this thread: element offset  tap * 16 * Cout * nch + (g * Cout + co) * 4  (+ chunk)
    auto w_off = [&](int k, int nch) {
        const int i0 = tid + k * 256, i = i0 < BI ? i0 : 0;          // clamped: the load is unconditional
        const int c4 = i % CT, tg = i / CT, gg = tg & 3, tap = tg >> 2;
        return tap * 16 * p.Cout * nch + (gg * p.Cout + co0 + c4) * 4;
    };
    // ... as BYTE offsets, once per kernel, for both operands' chunk counts (a unit adds its chunk to the scalar base)
    unsigned wofA[BN], wofV[BN];
    // The unit sequence is generated incrementally (no divisions): chunk, then operand part, then tile.
    struct UI { int t, part, ch, np, n0, y0, x0; unsigned inb; int im[IDX ? G::IMG : 1]; };
    TileGeo<GK, SMALL_A> tgeo;                       // geometry of the tile the generator stands on
    UI gen = {};
    const int aC = p.a.C, vC = HAS_V ? p.Cv : 0;
    const gptr<const float> aX = p.a.x, vX = p.v, wAp = p.wa, wVp = p.wv;
    const bool odd_c = ((aC | vC) & 15) != 0;        // (uniform) some chunk has fewer than four channel quads
#pragma unroll
    for (int k = 0; k < BN; ++k) { wofA[k] = (unsigned)w_off(k, nchA) * 4u; wofV[k] = (unsigned)w_off(k, nchV) * 4u; }
    auto set_np = [&](UI &r) {
        const int C = HAS_V ? sel_i(r.part, aC, vC) : aC;
        r.np = (C - r.ch * 16 + 3) >> 2;           // channel quads left from this chunk on (may exceed 4)
    };
    auto gen_tile = [&](UI &r, int t) {
        r.t = t; r.part = 0; r.ch = 0;
        tile_origin<GK>(p, xa ? xcd_tile<GK>(t, xcd_id, tpi) : t, r.n0, r.y0, r.x0);
        if constexpr (IDX) {                         // (uniform loads; slots past the count read slot 0 and are masked)
#pragma unroll
            for (int j = 0; j < G::IMG; ++j) r.im[j] = p.idx[r.n0 + j < p.n ? r.n0 + j : 0];
            tile_geo<GK, SMALL_A>(tgeo, ik, p, r.n0, r.y0, r.x0, r.im, aC, vC);
        } else
        tile_geo<GK, SMALL_A>(tgeo, ik, p, r.n0, r.y0, r.x0, nullptr, aC, vC);
        r.inb = tgeo.inb;
        set_np(r);
    };
    auto gen_next = [&](UI &r) {
        r.ch += NCH;
        if (r.ch >= (HAS_V ? sel_i(r.part, nchA, nchV) : nchA)) {
            if (HAS_V && !r.part && nchV) { r.part = 1; r.ch = 0; }
            else { gen_tile(r, r.t + sqd); return; }
        }
        set_np(r);
    };
    const bool b_once = upt == 1;                    // one unit per tile: the weights never change
    // loads of the unit the generator stands on (its tile geometry is in tgeo); unconditional: a unit
    // past the end has every item out of range (clamped addresses) and is never stored
    constexpr int LK = EPI != EPI_FWD ? 2 : (SMALL_A ? 1 : 0);
    auto unit_load = [&](const UI &q, f32x4 (*xq)[XW], f32x4 *bq) {
        // (operand selects on LOCALS: a select between two fields of the by-value kernel argument
        // was compiled to a scratch-memory table indexed by `part`)
        const gptr<const float> src = HAS_V ? sel_p(q.part, aX, vX) : aX, wp = HAS_V ? sel_p(q.part, wAp, wVp) : wAp;
        const int C = HAS_V ? sel_i(q.part, aC, vC) : aC;
#pragma unroll
        for (int sc = 0; sc < SC; ++sc) {
            const int cs = KSPLIT ? kg : sc;           // chunk of the unit this thread group handles
            ld_items<GK, LK, XW, SMALL_A>(xq + sc * XN, p, tgeo, ik, q.part, (q.ch + cs) * 16, q.np - 4 * cs, src, C, odd_c);
        }
#pragma unroll
        for (int sc = 0; sc < SC; ++sc) {
            const int cs = KSPLIT ? kg : sc;
            const gptr<const char> wb = pcast<const char>(wp) + (size_t)((q.ch + cs) * 16 * p.Cout) * 4;       // (uniform: the unit's chunk)
#pragma unroll
            for (int k = 0; k < BN; ++k) bq[sc * BN + k] = ld_at<f32x4>(wb, (HAS_V && q.part) ? wofV[k] : wofA[k]);
        }
    };
    auto unit_store = [&](const UI &q, f32x4 (*xq)[XW], f32x4 *bq, int buf, bool with_b) {
#pragma unroll
        for (int sc = 0; sc < SC; ++sc) {
            const int cs = KSPLIT ? kg : sc;
            f32x4 *td = tile[buf] + cs * 4 * P;
            f32x4 (*xs)[XW] = xq + sc * XN;
            const int c0 = (q.ch + cs) * 16, np = q.np - 4 * cs;
            bool done = false;
            if constexpr (EPI == EPI_FWD) {
                if (q.part) { done = true; st_items<GK, 1, XW>(td, xs, p, cA, q.inb, ik, c0, np); }
            }
            if constexpr (EPI != EPI_FWD) {
                if (p.ga_on) { done = true; st_items<GK, 2, XW>(td, xs, p, cA, q.inb, ik, c0, np); }
            }
            if (!done) st_items<GK, 0, XW>(td, xs, p, cA, q.inb, ik, c0, np);
        }
        if (with_b) {
            f32x4 *dst = wtile[(b_once || WtSingle<CT>::v) ? 0 : buf];
#pragma unroll
            for (int sc = 0; sc < SC; ++sc)
#pragma unroll
                for (int k = 0; k < BN; ++k) { const int i = tid + k * 256; if (i < BI) dst[(KSPLIT ? kg : sc) * BI + i] = bq[sc * BN + k]; }
        }
    };

    // Two register sets (unit 0 -> A, unit 1 -> B in the prologue): while unit u computes, unit u+1 is
    // landed/landing in one set (written to LDS at the end of the step) and unit u+2 is being loaded
    // into the other: the prefetch distance is
    // two units, enough to cover a load round trip with ~0.5 us of MFMAs per unit.
    f32x4 xrA[SC * XN][XW], xrB[SC * XN][XW];
    f32x4 brA[SC * BN], brB[SC * BN];
    f32x4 acc[MT][NT];
    float s1[NT], s2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { s1[nt] = 0.f; s2[nt] = 0.f; }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Prologue: coefficient tables first, then units 0 and 1 requested together.  (Requesting unit 0
    // before the tables was measured slower: memory returns in order, so the table loads queue behind
    // the tile loads and nothing is saved, while the registers stay live across the table code.)
    UI cu = {}, n1 = {}, n2 = {};
    // Forward, batch statistics: the slot array (nslot x 2C doubles, contiguous) is REQUESTED here, spread
    // over all threads (<= TABQ loads each), and only summed after the first two units' loads have been
    // issued -- the coefficient round trip and the tile round trip overlap instead of following each other.
    // Same summation order as bn_coef (slots ascending), so the coefficients are bit-identical.
    constexpr int TABQ = 8;
    [[maybe_unused]] double tabq[TABQ];
    [[maybe_unused]] float tab_g = 1.f, tab_b = 0.f;
    bool tab_late = false;
    if constexpr (EPI == EPI_FWD) {
        const int tot = p.a.nslot * 2 * p.a.C;
        tab_late = p.a.mode == MPNN_ACT_BN_BATCH && tot <= TABQ * 256 && p.a.C <= 256;     // (uniform)
        if (tab_late) {
#pragma unroll
            for (int j = 0; j < TABQ; ++j) { const int k = tid + 256 * j; tabq[j] = p.a.sum[k < tot ? k : 0]; }
            const int c = tid < p.a.C ? tid : 0;
            tab_g = p.a.gamma[c]; tab_b = p.a.beta[c];
        }
    }
    if (EPI == EPI_FWD && p.a.mode != MPNN_ACT_IDENTITY && !tab_late) {
        for (int c = tid; c < p.a.C; c += 256) {
            const BnC k = bn_coef(p.a, c);
            cA[c * 3] = k.m; cA[c * 3 + 1] = k.gamma * k.rstd; cA[c * 3 + 2] = k.beta;
        }
    }
    // (training: batch statistics -- bn_bwd_row requests every input of a row at once; other modes: the general path)
    if (EPI != EPI_FWD && p.ga_on) {
        if (p.ga_bn.mode == MPNN_ACT_BN_BATCH) {               // (uniform)
            for (int c = tid; c < p.a.C; c += 256) bn_bwd_row(p.ga_bn, p.ga_red, p.ga_nslot, c, false, cA + c * 5);
        } else {
            const double inv = 1.0 / (double)p.ga_bn.cnt;
            for (int c = tid; c < p.a.C; c += 256) {
                const BnC k = bn_coef(p.ga_bn, c);
                float *e = cA + c * 5;
                e[0] = k.m; e[1] = k.rstd; e[2] = k.gamma * k.rstd;
                double r0, r1;
                slot_sum2(p.ga_red, 2 * p.a.C, c, p.a.C + c, p.ga_nslot, r0, r1);
                e[3] = (float)(r0 * inv); e[4] = (float)(r1 * inv);
            }
        }
    }
    if (EPI == EPI_DGH_BN || EPI == EPI_DGV) {
        for (int c = tid - 128; c >= 0 && c < CT; c += 256) {     // waves 2-3: beside the table above
            float *e = cE + c * 5;
            if (p.pbn.mode == MPNN_ACT_BN_BATCH) {             // (uniform)
                bn_bwd_row(p.pbn, EPI == EPI_DGV ? p.red : gptr<const double>(nullptr), p.red_nslot, co0 + c, EPI == EPI_DGH_BN, e);
                continue;
            }
            const BnC k = bn_coef(p.pbn, co0 + c);
            e[0] = k.m; e[1] = k.rstd; e[2] = k.gamma * k.rstd;
            if (EPI == EPI_DGH_BN) { e[3] = k.beta; e[4] = 0.f; }
            else {
                const double inv = 1.0 / (double)p.pbn.cnt;
                double r0 = 0.0, r1 = 0.0;                         // dbeta, dgamma
                if (p.red) slot_sum2(p.red, 2 * p.pbn.C, co0 + c, p.pbn.C + co0 + c, p.red_nslot, r0, r1);
                e[3] = (float)(r0 * inv); e[4] = (float)(r1 * inv);
            }
        }
    }
    if (!tab_late) __syncthreads();
    trace_stamp(1);
    gen_tile(gen, sq0);
    cu = gen;
    unit_load(cu, xrA, brA);
    if (n_units > 1) {
        gen_next(gen);
        n1 = gen;
        unit_load(n1, xrB, brB);
    }
    if constexpr (EPI == EPI_FWD) {
        if (tab_late) {
            // (the slot values are older than the tile loads: the wait below is vmcnt(tile loads), not 0)
            double *scr = (double *)smem;            // the tile / weight buffers are not in use yet
            const int C = p.a.C, tot = p.a.nslot * 2 * C;
#pragma unroll
            for (int j = 0; j < TABQ; ++j) { const int k = tid + 256 * j; if (k < tot) scr[k] = tabq[j]; }
            __syncthreads();
            if (tid < C) {
                double s1 = 0.0, s2 = 0.0;
                for (int sl = 0; sl < p.a.nslot; ++sl) { s1 += scr[(2 * sl) * C + tid]; s2 += scr[(2 * sl + 1) * C + tid]; }
                const double inv = 1.0 / (double)p.a.cnt, mean = s1 * inv;
                double var = s2 * inv - mean * mean;
                var = var < 0.0 ? 0.0 : var;
                cA[tid * 3] = (float)mean; cA[tid * 3 + 1] = tab_g * rsqrtf((float)var + p.a.eps); cA[tid * 3 + 2] = tab_b;
            }
            __syncthreads();
        }
    }
    if constexpr (XItems<GK>::INTERIOR)                // the halo ring of both tile buffers: zero for the whole kernel
        zero_ring<GK, P>(&tile[0][0], 2 * NCH * 4, threadIdx.x, KSPLIT ? NCH * 256 : 256);
    if (n_units > 0) unit_store(cu, xrA, brA, 0, true);
    __syncthreads();
    trace_stamp(2);

    // One step: compute unit u (LDS buffer u&1); RN1 holds unit u+1, RN2 receives unit u+2.
    auto step = [&](const int u, f32x4 (*xn1)[XW], f32x4 *bn1, f32x4 (*xn2)[XW], f32x4 *bn2) {
        const f32x4 *cur = tile[u & 1];
        const bool more = u + 1 < n_units, more2 = u + 2 < n_units;
        const int part = cu.part, t = cu.t, n0 = cu.n0, y0 = cu.y0, x0 = cu.x0;
        const int t2 = n1.t;
        if (more2) {       // (unconditional loads past the end were measured slower: short workgroups doubled their loads)
            gen_next(gen);
            n2 = gen;
            unit_load(n2, xn2, bn2);
        }
        // dgrad-vert: the epilogue's operands (the finer map's conv sums and its masked dz, four per
        // coarse pixel) are requested BEFORE the MFMAs of the tile's last unit, not after them: one
        // memory round trip less in the chain of every tile.
        [[maybe_unused]] float e_sv[MT][4][NT][4], e_dz[MT][4][NT][4];
        if constexpr (EPI == EPI_DGV) {
            if ((!more || t2 != t) && !MPNN_DBG(p, 4)) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int img, ty, tx;
                        mtile_pix<GK>(wm * MT + mt, g * 4 + r, img, ty, tx);
                        const int n = n0 + img < p.n ? n0 + img : 0, y = y0 + ty, x = x0 + tx;
                        const int W2 = p.W * 2;
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const unsigned i00 = (((unsigned)n * (p.H * 2) + 2 * y) * W2 + 2 * x) * p.Cout + cw + nt * 16;
                            const unsigned ix[4] = {i00, i00 + p.Cout, i00 + (unsigned)W2 * p.Cout, i00 + (unsigned)W2 * p.Cout + p.Cout};
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                e_sv[mt][r][nt][k] = p.sprev[ix[k]];
                                e_dz[mt][r][nt][k] = p.has_dz ? p.out[ix[k]] : 0.f;
                            }
                        }
                    }
            }
        }
        // dgrad-horz: likewise the producer's conv sums (ReLU mask, xhat) and the exit's dX of the tile's
        // output pixels: requested before the last unit's MFMAs instead of in the epilogue.
        [[maybe_unused]] float h_sp[MT][4][NT], h_ex[MT][4][NT];
        if constexpr (EPI == EPI_DGH_BN) {
            if ((!more || t2 != t) && !MPNN_DBG(p, 4)) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int img, ty, tx;
                        mtile_pix<GK>(wm * MT + mt, g * 4 + r, img, ty, tx);
                        const int n = n0 + img < p.n ? n0 + img : 0, y = y0 + ty, x = x0 + tx;
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const unsigned idx = (((unsigned)n * p.H + y) * p.W + x) * p.Cout + cw + nt * 16;
                            h_sp[mt][r][nt] = p.sprev[idx];
                            h_ex[mt][r][nt] = p.extra ? p.extra[idx] : 0.f;
                        }
                    }
            }
        }
        // ----------------------------- MFMAs of unit u -----------------------------
        if (!MPNN_DBG(p, 1)) {
            const f32x4 *wl = (b_once || WtSingle<CT>::v) ? wtile[0] : wtile[u & 1];
            const int wcol = wn * NT * 16 + li;
            if (SMALL_A && part == 0) {
                const float *tf = (const float *)cur;
                const float *wf = (const float *)wl;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int dy = tap / 3, dx = tap - dy * 3;
                    float b[NT], a[MT];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) b[nt] = wf[((tap * 4) * CT + wcol + nt * 16) * 4 + g];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) a[mt] = tf[(slot0[mt] + dy * R + dx) * 4 + g];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
                }
            } else {
                // Software-pipelined over the NCH * 9 (chunk, tap) fragments: the LDS reads of fragment
                // t + 1 are issued before the MFMAs of fragment t, so their latency hides under 4 * MT * NT
                // MFMAs instead of stalling the wave once per tap.
                f32x4 fa[2][MT], fb[2][NT];
                auto frag = [&](int it, f32x4 *a, f32x4 *bq) {
                    const int s9 = it / 9, tap = it - s9 * 9, dy = tap / 3, dx = tap - dy * 3;
                    const int sc = KSPLIT ? kg : s9;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bq[nt] = wl[sc * BI + (tap * 4 + g) * CT + wcol + nt * 16];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) a[mt] = cur[sc * 4 * P + g * P + slot0[mt] + dy * R + dx];
                };
                frag(0, fa[0], fb[0]);
#pragma unroll
                for (int it = 0; it < SC * 9; ++it) {
                    if (it + 1 < SC * 9) frag(it + 1, fa[(it + 1) & 1], fb[(it + 1) & 1]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[it & 1][mt][j], fb[it & 1][nt][j], acc[mt][nt], 0, 0, 0);
                    // pin the order for the machine scheduler (it otherwise sinks the reads to their use)
                    if (it + 1 < SC * 9) __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);   // DS reads of t+1
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * MT * NT, 0);                        // MFMAs of t
                }
            }
        }
        mfma_drain();
        if (WtSingle<CT>::v && !b_once) lds_barrier();      // (single weight buffer: every wave is done with this unit's weights)
        if (u == 0) trace_stamp(8);
        // ----------------------------- stage unit u+1 ------------------------------
        // BEFORE the epilogue: its wait then covers exactly the loads of unit u+2 issued above
        // (vmcnt(N)); behind the epilogue's conditional global stores the count would be unknown.
        if (more && !MPNN_DBG(p, 2)) unit_store(n1, xn1, bn1, (u + 1) & 1, !b_once);
        if (u == 0) trace_stamp(9);
        // ----------------------------- epilogue of a finished tile -----------------
        // D layout: col = lane & 15 (channel), row = (lane >> 4) * 4 + r (pixel of the M-tile).
        if ((!more || t2 != t) && !MPNN_DBG(p, 4)) {
            if constexpr (KSPLIT) {                     // partial sums of the second K-group -> LDS -> first group
                f32x4 *kred = (f32x4 *)pool_lds;          // [group - 1][wave][lane]
                if (kg > 0) kred[(kg - 1) * 256 + wid * 64 + lane] = acc[0][0];
                lds_barrier();
                if (kg == 0) acc[0][0] += kred[wid * 64 + lane];
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int img, ty, tx;
                    mtile_pix<GK>(wm * MT + mt, g * 4 + r, img, ty, tx);
                    const int y = y0 + ty, x = x0 + tx;
                    if (n0 + img >= p.n || kg != 0) continue;
                    int n = n0 + img;
                    if constexpr (IDX) n = pick_img<G::IMG>(cu.im, img);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const int co = cw + nt * 16;
                        const int cl = co - co0;
                        float val = acc[mt][nt][r];
                        if (EPI == EPI_FWD) {
                            const unsigned idx = (((unsigned)n * p.H + y) * p.W + x) * p.Cout + co;
                            val += bias_r[nt];
                            p.out[idx] = val;
                            s1[nt] += val; s2[nt] += val * val;
                            if (GK != 2 && p.pool_out) pool_lds[((wm * MT + mt) * 16 + g * 4 + r) * CT + cl] = val;
                        } else if (EPI == EPI_DGH_RAW) {
                            const unsigned idx = (((unsigned)n * p.H + y) * p.W + x) * p.Cout + co;
                            if (p.extra) val += p.extra[idx];
                            if (p.acc_out) val += p.out[idx];
                            p.out[idx] = val;
                        } else if (EPI == EPI_DGH_BN) {
                            const unsigned idx = (((unsigned)n * p.H + y) * p.W + x) * p.Cout + co;
                            const float *e = cE + cl * 5;
                            const float d = h_sp[mt][r][nt] - e[0];
                            const float yv = d * e[2] + e[3];
                            const float dz = yv > 0.f ? val + h_ex[mt][r][nt] : 0.f;
                            p.out[idx] = p.acc_out ? p.out[idx] + dz : dz;      // (tree nets: siblings' earlier sum)
                            s1[nt] += dz; s2[nt] += dz * (d * e[1]);
                        } else {  // EPI_DGV: val = d(pooled fine map) at coarse pixel (y, x)
                            const float *e = cE + cl * 5;
                            const int W2 = p.W * 2;
                            const unsigned i00 = (((unsigned)n * (p.H * 2) + 2 * y) * W2 + 2 * x) * p.Cout + co;
                            const unsigned ix[4] = {i00, i00 + p.Cout, i00 + (unsigned)W2 * p.Cout,
                                                  i00 + (unsigned)W2 * p.Cout + p.Cout};
                            float sv[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) sv[k] = e_sv[mt][r][nt][k];
                            int arg = 0; float mx = sv[0];
#pragma unroll
                            for (int k = 1; k < 4; ++k) if (sv[k] > mx) { mx = sv[k]; arg = k; }
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const float dzf = e_dz[mt][r][nt][k];
                                const float xh = (sv[k] - e[0]) * e[1];
                                float gk = e[2] * (dzf - e[3] - xh * e[4]);
                                if (k == arg) gk += val;
                                p.out[ix[k]] = gk;
                            }
                        }
                    }
                }
            }
            // 2x2 max-pool of the finished tile for the next coarser scale's vert conv
            // (layer_types.py:185): the tile's 64 pixels meet in LDS, each thread pools one value.
            if (EPI == EPI_FWD && GK != 2 && p.pool_out) {        // uniform across the workgroup
                lds_barrier();                     // LDS only: __syncthreads would also wait for the output stores just issued
                if (n0 < p.n && kg == 0) {
                    constexpr int TWp = GK == 0 ? 8 : 4, ROW = GK == 0 ? 16 : 8;   // pooled tile width, tile row length
                    const int H2 = p.H >> 1, W2 = p.W >> 1;
                    for (int e = tid; e < 16 * CT; e += 256) {
                        const int c = e % CT, pp = e / CT, py = pp / TWp, px = pp - py * TWp;
                        const float *q0 = pool_lds + ((2 * py) * ROW + 2 * px) * CT + c;
                        const float m4 = fmaxf(fmaxf(q0[0], q0[CT]), fmaxf(q0[ROW * CT], q0[ROW * CT + CT]));
                        const int np0 = IDX ? cu.im[0] : n0;          // (one image per tile in these geometries)
                        p.pool_out[(((unsigned)np0 * H2 + (y0 >> 1) + py) * W2 + (x0 >> 1) + px) * p.Cout + co0 + c] = m4;
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        cu = n1; n1 = n2;
        if (u == 0) trace_stamp(10);
        lds_barrier();              // LDS-only: the prefetch loads of unit u+2 stay in flight
    };
    for (int u = 0; u < n_units; u += 2) {
        step(u, xrB, brB, xrA, brA);
        if (u == 0) trace_stamp(3);
        if (u + 1 < n_units) step(u + 1, xrA, brA, xrB, brB);
    }
    trace_stamp(4);

    if (EPI == EPI_FWD || EPI == EPI_DGH_BN) {
        const gptr<double> dst = EPI == EPI_FWD ? p.out_sum : p.red_out;
        if (dst) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const double a1 = reduce_g4((double)s1[nt]);
                const double a2 = reduce_g4((double)s2[nt]);
                if (g == 0 && kg == 0) {
                    const int cl = wn * NT * 16 + nt * 16 + li;
                    redbuf[(wm * CT + cl) * 2] = a1;
                    redbuf[(wm * CT + cl) * 2 + 1] = a2;
                }
            }
            lds_barrier();                         // (LDS only: do not wait for the tile stores before the statistics atomics)
            if (tid < CT && kg == 0) {
                double a1 = 0.0, a2 = 0.0;
#pragma unroll
                for (int w = 0; w < WM; ++w) { a1 += redbuf[(w * CT + tid) * 2]; a2 += redbuf[(w * CT + tid) * 2 + 1]; }
                const gptr<double> slot = dst + (size_t)(bx % p.out_nslot) * 2 * p.Cout;
                atomic_add_d(slot + co0 + tid, a1);
                atomic_add_d(slot + p.Cout + co0 + tid, a2);
            }
        }
    }
    trace_stamp(5);
    trace_note(6, EPI + 1); trace_note(7, n_units);
}

template <int GK, int MT, int NT, int WM, int WN, bool SMALL_A, int EPI>
__global__ __launch_bounds__(256) void conv_k(const ConvP p) {
    __shared__ __attribute__((aligned(16))) char smem[ConvSmem<GK, WM, WN * NT * 16>::BYTES];
    conv_body<GK, MT, NT, WM, WN, SMALL_A, EPI>(p, blockIdx.x, blockIdx.y, gridDim.x, smem);
}

// Two independent convs over the SAME input map in one launch: rows [0, gy0) of the grid run the
// first (dgrad-horz) body, the rest the second (dgrad-vert) body.  Their serial latency chains
// (prologue, first loads, epilogue drain) overlap instead of adding up across two launches.
template <int GK, int MT, int NT, int WM, int WN, int EPI0, int EPI1>
__global__ __launch_bounds__(256) void conv_pair_k(const ConvP p0, const ConvP p1, const int gy0, const int gx0,
                                                   const int gx1) {
    __shared__ __attribute__((aligned(16))) char smem[ConvSmem<GK, WM, WN * NT * 16>::BYTES];
    if ((int)blockIdx.y < gy0) {
        if ((int)blockIdx.x < gx0) conv_body<GK, MT, NT, WM, WN, false, EPI0>(p0, blockIdx.x, blockIdx.y, gx0, smem);
    } else {
        if ((int)blockIdx.x < gx1) conv_body<GK, MT, NT, WM, WN, false, EPI1>(p1, blockIdx.x, blockIdx.y - gy0, gx1, smem);
    }
}

// ------------------------------- host dispatch -------------------------------
static inline int conv_cap_gx(int n_tiles, int gy) {
    const int cap = 1024 / gy > 64 ? 1024 / gy : 64;      // persistent: a few workgroups per CU
    return n_tiles > cap ? cap : n_tiles;
}

// Pair launch (both convs use 16-channel tiles: cfg <1,1,4,1>).
template <int GK, int EPI0, int EPI1>
static int conv_launch_pair_geom(ConvP &p0, ConvP &p1, hipStream_t st) {
    if ((p0.Cout % 16) || (p1.Cout % 16)) return MPNN_E_SHAPE;
    p0.n_tiles = p1.n_tiles = conv_grid_x<GK>(p0.n, p0.H, p0.W);
    p0.dbg = p1.dbg = 0;
    const int gy0 = p0.Cout / 16, gy1 = p1.Cout / 16;
    const int gx0 = conv_cap_gx(p0.n_tiles, gy0), gx1 = conv_cap_gx(p1.n_tiles, gy1);
    dim3 grid(gx0 > gx1 ? gx0 : gx1, gy0 + gy1), block(256);
    hipLaunchKernelGGL((conv_pair_k<GK, 1, 1, 4, 1, EPI0, EPI1>), grid, block, 0, st, p0, p1, gy0, gx0, gx1);
    MPNN_LAUNCH_CHECK();
    return 0;
}

template <int EPI0, int EPI1>
static int conv_launch_pair(ConvP &p0, ConvP &p1, hipStream_t st) {
    if (p0.n <= 0) return 0;
    if (p0.H != p1.H || p0.W != p1.W || p0.n != p1.n) return MPNN_E_ARG;
    if (p0.a.C > 128 || p1.a.C > 128 || (p0.a.C & 3) || (p1.a.C & 3)) return MPNN_E_SHAPE;
    if (p0.W >= 16 && (p0.W % 16) == 0 && (p0.H % 4) == 0) return conv_launch_pair_geom<0, EPI0, EPI1>(p0, p1, st);
    if (p0.W == 8 && p0.H == 8) return conv_launch_pair_geom<1, EPI0, EPI1>(p0, p1, st);
    if (p0.W == 4 && p0.H == 4) return conv_launch_pair_geom<2, EPI0, EPI1>(p0, p1, st);
    return MPNN_E_SHAPE;
}

template <int GK, int MT, int NT, int WM, int WN, int EPI>
static int conv_launch_cfg(ConvP &p, bool small_a, hipStream_t st) {
    constexpr int CT = WN * NT * 16;
    p.n_tiles = conv_grid_x<GK>(p.n, p.H, p.W);
#ifdef MPNN_ABLATE
    static const int dbg_env = [] { const char *e = getenv("MPNN_CONV_DBG"); return e ? atoi(e) : 0; }();   // (read once)
    p.dbg = dbg_env;
#else
    p.dbg = 0;
#endif
    const int gy = p.Cout / CT;
    const int gx = conv_cap_gx(p.n_tiles, gy);
    dim3 grid(gx, gy), block(256);
    if constexpr (EPI == EPI_FWD) {
        if (small_a) {
            hipLaunchKernelGGL((conv_k<GK, MT, NT, WM, WN, true, EPI>), grid, block, 0, st, p);
            MPNN_LAUNCH_CHECK();
            return 0;
        }
    }
    hipLaunchKernelGGL((conv_k<GK, MT, NT, WM, WN, false, EPI>), grid, block, 0, st, p);
    MPNN_LAUNCH_CHECK();
    return 0;
}

template <int GK, int EPI>
static int conv_launch_geom(ConvP &p, bool small_a, hipStream_t st) {
    const int Co = p.Cout;
    if (Co % 16) return MPNN_E_SHAPE;
    // Small maps have few spatial tiles and are latency-bound: narrow channel tiles give more,
    // shorter workgroups there (measured: 16 beats 32/64 on 8x8 and 4x4 maps).
    if constexpr (GK == 0) {
        if (Co % 64 == 0) return conv_launch_cfg<GK, 2, 2, 2, 2, EPI>(p, small_a, st);
    }
    return conv_launch_cfg<GK, 1, 1, 4, 1, EPI>(p, small_a, st);
}

template <int EPI>
static int conv_launch(ConvP &p, hipStream_t st) {
    if (p.n <= 0) return 0;
    if (p.a.C > 128 || p.Cv > 128 || (p.Cv & 3)) return MPNN_E_SHAPE;
    const bool small_a = p.a.C <= 4;
    if (!small_a && (p.a.C & 3)) return MPNN_E_SHAPE;
    if (p.W >= 16 && (p.W % 16) == 0 && (p.H % 4) == 0) return conv_launch_geom<0, EPI>(p, small_a, st);
    if (p.W == 8 && p.H == 8) return conv_launch_geom<1, EPI>(p, small_a, st);
    if (p.W == 4 && p.H == 4) return conv_launch_geom<2, EPI>(p, small_a, st);
    return MPNN_E_SHAPE;
}
