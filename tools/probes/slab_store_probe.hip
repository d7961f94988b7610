// How should the weight-gradient slabs leave a backward launch?  MEASURED with a model of the launch's end instead of argued:
// a producer of 256 workgroups x 256 threads spins on the clock for 8 us (the unit loop), then writes a [rows][64] fp32
// tile per workgroup (144 rows = 36 KB: nine taps x 16 input channels x 64 output channels; 72 and 36 rows too); a DEPENDENT
// consumer kernel (the slab reduction: workgroups on every XCD, each reads a tile another XCD wrote) reads all of it with
// 16-byte loads and checks every word.  Both sit in one captured graph, 20 pairs per graph.
//   form a: plain dword stores in the accumulator's shape -- a wave instruction writes 16 lanes x 4 B in each of four rows
//           (rows 4 g + r of a 16-row chunk, the wave's own 64-byte column), 36 instructions per lane for 36 KB;
//   form b: plain 16-byte stores of whole 256-byte rows (a wave instruction = four consecutive rows), nine per lane;
//   form c: form b, stored write-through (sc1: the line leaves the XCD's L2 at once instead of at the kernel's end);
//   form d: form c while the odd workgroups write nothing and spin 16 us (the deep launches: the weight-gradient workgroups
//           exit 8 us before the input-gradient chains);
//   form e: form d with form a's stores (what form d is to be compared with).
// Per form and tile size: the time per pair (events over 50 replays, an empty pair's spin included), and from the clock
// stamps of single pairs (median of 9): producer first start -> last end, producer's last end -> consumer's first start
// and first loaded word, the whole pair.
//   hipcc --offload-arch=gfx950 -O3 tools/probes/slab_store_probe.hip -o tools/probes/slab_store_probe && tools/probes/slab_store_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define NWG 256
#define MAXROWS 144
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct Args {
    float *tiles;                // [NWG][MAXROWS][64]
    unsigned *epoch;             // [0] epoch, [1] consumer ticket
    unsigned long long *stamp;   // [2][NWG][3]: start / first data (consumer) or first store (producer) / end
    int *bad;
    int rows;
    long spin;                   // ticks of the 100 MHz clock
};

__device__ __forceinline__ void spin(long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while ((long)(__builtin_amdgcn_s_memrealtime() - t0) < ticks) __builtin_amdgcn_s_sleep(2);
}
__device__ __forceinline__ float word(unsigned epoch, int wg, int i) { return (float)((epoch * 131u + (unsigned)wg * 17u + (unsigned)i) & 0xfffffu); }

template <int FORM>
__global__ __launch_bounds__(256) void producer(const Args a) {
    const int tid = threadIdx.x, wg = blockIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const unsigned e = a.epoch[0];
    unsigned long long *s = a.stamp + (size_t)wg * 3;
    if (tid == 0) s[0] = __builtin_amdgcn_s_memrealtime();
    const bool late = (FORM == 3 || FORM == 4) && (wg & 1);
    spin(late ? 2 * a.spin : a.spin);
    if (tid == 0) s[1] = __builtin_amdgcn_s_memrealtime();
    float *t = a.tiles + (size_t)wg * MAXROWS * 64;
    if (!late) {
        if (FORM == 0 || FORM == 4) {
            for (int k = 0; k * 16 < a.rows; ++k)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = k * 16 + g * 4 + r, i = row * 64 + wid * 16 + li;
                    if (row < a.rows) t[i] = word(e, wg, i);
                }
        } else {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(t, 0, MAXROWS * 64 * 4, 0x00020000);
            for (int i = tid * 4; i < a.rows * 64; i += 1024) {
                const f32x4 v = {word(e, wg, i), word(e, wg, i + 1), word(e, wg, i + 2), word(e, wg, i + 3)};
                if (FORM == 1) *(f32x4 *)(t + i) = v;
                else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, i * 4, 0, 16);     // sc1
            }
        }
    }
    __syncthreads();
    if (tid == 0) s[2] = __builtin_amdgcn_s_memrealtime();
}

__global__ __launch_bounds__(256) void consumer(const Args a) {
    const int tid = threadIdx.x, wg = blockIdx.x;
    unsigned long long *s = a.stamp + (size_t)(NWG + wg) * 3;
    if (tid == 0) s[0] = __builtin_amdgcn_s_memrealtime();
    const unsigned e = a.epoch[0];
    const int src = (wg + 3) & (NWG - 1);            // a tile written on another XCD (workgroups are dealt round-robin)
    const float *t = a.tiles + (size_t)src * MAXROWS * 64;
    int nbad = 0;
    bool first = true;
    for (int i = tid * 4; i < a.rows * 64; i += 1024) {
        const f32x4 v = *(const f32x4 *)(t + i);
        if (first && tid == 0) { s[1] = __builtin_amdgcn_s_memrealtime() + (v[0] == -1.f ? 1 : 0); first = false; }
#pragma unroll
        for (int j = 0; j < 4; ++j) nbad += v[j] != word(e, src, i + j);
    }
    if (nbad && !(a.bad[1] && (src & 1)))      // (forms d, e: the late workgroups' tiles hold an older epoch)
        atomicAdd(a.bad, nbad);
    __syncthreads();
    if (tid == 0) {
        s[2] = __builtin_amdgcn_s_memrealtime();
        if (atomicAdd(a.epoch + 1, 1u) == NWG - 1) { a.epoch[1] = 0; atomicAdd(a.epoch, 1u); }     // the last workgroup of the pair turns the epoch
    }
}

static void launch_producer(int form, hipStream_t st, const Args &a) {
    switch (form) {
    case 0: hipLaunchKernelGGL(producer<0>, dim3(NWG), dim3(256), 0, st, a); break;
    case 1: hipLaunchKernelGGL(producer<1>, dim3(NWG), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(producer<2>, dim3(NWG), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(producer<3>, dim3(NWG), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(producer<4>, dim3(NWG), dim3(256), 0, st, a); break;
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    Args a{};
    CK(hipMalloc(&a.tiles, (size_t)NWG * MAXROWS * 64 * 4));
    CK(hipMalloc(&a.epoch, 8)); CK(hipMemset(a.epoch, 0, 8));
    CK(hipMalloc(&a.stamp, 2 * NWG * 3 * 8));
    CK(hipMalloc(&a.bad, 8)); CK(hipMemset(a.bad, 0, 8));
    a.spin = 800;
    hipStream_t st; CK(hipStreamCreate(&st));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int CH = 20, REP = 50, NS = 9;
    const char *names[5] = {"a plain dword, accumulator shape", "b plain 16-byte rows", "c sc1 16-byte rows",
                            "d sc1 rows, half the grid 8 us late", "e dword shape, half the grid 8 us late"};
    const int rows_of[3] = {144, 72, 36};
    printf("%-40s %5s %9s | %9s %9s %9s %9s | %s\n", "form", "KB/WG", "us/pair", "prod", "end->start", "end->data", "pair", "bad words");
    for (int ri = 0; ri < 3; ++ri)
    for (int form = 0; form < 5; ++form) {
        a.rows = rows_of[ri];
        const int late = form >= 3;
        CK(hipMemcpy(a.bad + 1, &late, 4, hipMemcpyHostToDevice));      // (the late workgroups' tiles hold an older epoch: not checked)
        hipGraph_t g, g1; hipGraphExec_t ge, ge1;
        CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        for (int c = 0; c < CH; ++c) { launch_producer(form, st, a); hipLaunchKernelGGL(consumer, dim3(NWG), dim3(256), 0, st, a); }
        CK(hipStreamEndCapture(st, &g));
        CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        launch_producer(form, st, a); hipLaunchKernelGGL(consumer, dim3(NWG), dim3(256), 0, st, a);
        CK(hipStreamEndCapture(st, &g1));
        CK(hipGraphInstantiate(&ge1, g1, nullptr, nullptr, 0));
        float ms = 0;
        for (int w = 0; w < 3; ++w) CK(hipGraphLaunch(ge, st));
        CK(hipEventRecord(e0, st));
        for (int r = 0; r < REP; ++r) CK(hipGraphLaunch(ge, st));
        CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        std::vector<double> prod, gap0, gap1, pair;
        std::vector<unsigned long long> s(2 * NWG * 3);
        for (int k = 0; k < NS; ++k) {
            CK(hipGraphLaunch(ge, st));              // (warm clocks and caches as in the timed run)
            CK(hipGraphLaunch(ge1, st));
            CK(hipStreamSynchronize(st));
            CK(hipMemcpy(s.data(), a.stamp, s.size() * 8, hipMemcpyDeviceToHost));
            unsigned long long p0 = ~0ull, p1 = 0, c0 = ~0ull, cd = ~0ull, c1 = 0;
            for (int i = 0; i < NWG; ++i) {
                p0 = std::min(p0, s[i * 3]); p1 = std::max(p1, s[i * 3 + 2]);
                c0 = std::min(c0, s[(NWG + i) * 3]); c1 = std::max(c1, s[(NWG + i) * 3 + 2]);
                cd = std::min(cd, s[(NWG + i) * 3 + 1]);
            }
            prod.push_back((double)(long long)(p1 - p0) * 0.01); gap0.push_back((double)(long long)(c0 - p1) * 0.01);
            gap1.push_back((double)(long long)(cd - p1) * 0.01); pair.push_back((double)(long long)(c1 - p0) * 0.01);
        }
        auto med = [](std::vector<double> &v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
        int bad = 0; CK(hipMemcpy(&bad, a.bad, 4, hipMemcpyDeviceToHost));
        printf("%-40s %5.0f %9.2f | %9.2f %9.2f %9.2f %9.2f | %d\n", names[form], a.rows * 0.25, ms * 1e3 / (CH * REP),
               med(prod), med(gap0), med(gap1), med(pair), bad);
        CK(hipGraphExecDestroy(ge)); CK(hipGraphExecDestroy(ge1)); CK(hipGraphDestroy(g)); CK(hipGraphDestroy(g1));
    }
    return 0;
}
