// mpnn_decode_u8: 8-bit pixels to the floats a net is trained on -- dst[i] = lut[src[i]], a pure table lookup (bit-exact
// for ANY table).  HBM-bound: 1 byte in, 4 bytes out per element.
//
// The 256-entry table sits in LDS (1 KB per workgroup).  Where the two pointers allow it -- some head of h < 16 elements
// makes src + h AND dst + h 16-byte aligned -- a thread reads 16 pixels with one 16-byte load and writes them with four
// float4 stores; a workgroup sweeps DEC_U * 256 such groups per pass with all its loads issued before the first lookup.
// The head and the tail (< 16 elements each) are written one element per thread by workgroup 0.  When no head aligns both
// pointers (src and dst disagree modulo 4 elements: a uniform test on the host), the scalar kernel runs instead: one
// element per thread, byte loads and dword stores, coalesced over the wave.  Neither kernel loads or stores outside
// [src, src + count) and [dst, dst + count).
#include "common.h"

#define DEC_T 256
#define DEC_U 4                         // 16-element groups per thread and pass (loads in flight per thread)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void decode_table_to_lds(float *tab, const float *__restrict__ lut) {
    tab[threadIdx.x] = lut[threadIdx.x];            // (DEC_T == 256 entries)
    __syncthreads();
}

__global__ __launch_bounds__(DEC_T) void decode_u8_vec_k(const unsigned char *__restrict__ src, float *__restrict__ dst,
                                                         const float *__restrict__ lut, long head, long n_vec, long tail) {
    __shared__ float tab[256];
    decode_table_to_lds(tab, lut);
    const u32x4 *s = (const u32x4 *)(src + head);    // 16-byte aligned (host)
    f32x4 *d = (f32x4 *)(dst + head);                // 16-byte aligned (host)
    for (long base = (long)blockIdx.x * (DEC_U * DEC_T); base < n_vec; base += (long)gridDim.x * (DEC_U * DEC_T)) {
        u32x4 v[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const long i = base + u * DEC_T + threadIdx.x;
            v[u] = i < n_vec ? s[i] : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const long i = base + u * DEC_T + threadIdx.x;
            if (i >= n_vec) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned w = v[u][j];          // (little endian: the first pixel is the low byte)
                d[i * 4 + j] = f32x4{tab[w & 255u], tab[(w >> 8) & 255u], tab[(w >> 16) & 255u], tab[w >> 24]};
            }
        }
    }
    if (blockIdx.x == 0) {                           // head and tail: < 16 elements each, one per thread
        const long t = threadIdx.x, at = head + 16 * n_vec;
        if (t < head) dst[t] = tab[src[t]];
        if (t < tail) dst[at + t] = tab[src[at + t]];
    }
}

__global__ __launch_bounds__(DEC_T) void decode_u8_scalar_k(const unsigned char *__restrict__ src, float *__restrict__ dst,
                                                            const float *__restrict__ lut, long count) {
    __shared__ float tab[256];
    decode_table_to_lds(tab, lut);
    for (long i = (long)blockIdx.x * DEC_T + threadIdx.x; i < count; i += (long)gridDim.x * DEC_T) dst[i] = tab[src[i]];
}

extern "C" int mpnn_decode_u8(const unsigned char *src, float *dst, const float *lut, long count, void *stream) {
    if (!src || !dst || !lut || count < 0 || ((size_t)dst & 3) || ((size_t)lut & 3)) return MPNN_E_ARG;
    if (count == 0) return 0;
    const long s_off = (long)((size_t)src & 15), d_off = (long)(((size_t)dst >> 2) & 3);
    // a head of h elements aligns src (h = -s_off mod 16) and dst (h = -d_off mod 4) iff s_off = d_off (mod 4)
    if (((s_off - d_off) & 3) != 0) {
        long wgs = (count + DEC_T - 1) / DEC_T;
        wgs = wgs > 4096 ? 4096 : wgs;
        hipLaunchKernelGGL(decode_u8_scalar_k, dim3((unsigned)wgs), dim3(DEC_T), 0, (hipStream_t)stream, src, dst, lut, count);
        MPNN_LAUNCH_CHECK();
        return 0;
    }
    long head = (16 - s_off) & 15;
    if (head > count) head = count;
    const long n_vec = (count - head) / 16, tail = count - head - 16 * n_vec;
    long wgs = (n_vec + DEC_U * DEC_T - 1) / (DEC_U * DEC_T);
    wgs = wgs < 1 ? 1 : (wgs > 65536 ? 65536 : wgs);
    hipLaunchKernelGGL(decode_u8_vec_k, dim3((unsigned)wgs), dim3(DEC_T), 0, (hipStream_t)stream, src, dst, lut, head, n_vec, tail);
    MPNN_LAUNCH_CHECK();
    return 0;
}
