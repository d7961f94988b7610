// mpnn_conf_gate: the confidence-threshold exit policy of the label-free evaluation (Net.predict(exit_conf=)) -- leave at
// the first exit whose head is sure.  The reference has no such policy (its nets leave where the learnt router says:
// net_types.py:127-129); this is the inference-time knob of other early-exit libraries, run on the same nets.
//
// The launch stands BEHIND mpnn_exit_ev / mpnn_exit_ev_gen, which stored the head's confidence by image (conf) and the
// switch's router outputs (r), and in front of everything that reads r: the prefix walk, mpnn_route, mpnn_ev_select.  One
// thread per sample of the node's list:
//   d = exit_sink                            if conf[img] >= *tau   (plain fp32 comparison: a NaN on either side is "no")
//   d = arg-max of r[img][i], i != exit_sink otherwise              (first index on ties: the rule of exit_ev_k; the learnt
//                                                                    router still chooses among the child blocks)
//   r[img][i] = (i == d) ? 1 : 0             for i < n_sinks        (a finite one-hot row: every later reader reproduces d
//                                                                    by its own arg-max; mpnn_route's softmax(r / tau) stays finite)
// and img is appended to child_idx[d] where that list exists -- wave64 ballot, popcount prefix, ONE atomicAdd per (wave,
// sink), the `pos < n` guard: the compaction of exit_ev_k, which gives a gated switch no child lists.  The threshold is one
// float in DEVICE memory: a sweep rewrites a float, a captured program replays for any value.  Rows of images that are not
// on the list are not touched; nothing depends on a list's order.
#include "common.h"

#define CG_THREADS 256
#define TS MPNN_MAX_SINKS

__global__ __launch_bounds__(CG_THREADS) void conf_gate_k(const mpnn_conf_gate_args *__restrict__ tab) {
    const mpnn_conf_gate_args &a = tab[blockIdx.y];
    int n = a.n;
    if (a.cnt) { const int c = *a.cnt; n = c < n ? c : n; }
    if ((int)(blockIdx.x * CG_THREADS) >= n) return;             // (uniform over the workgroup)
    const int s = blockIdx.x * CG_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = s < n;
    const int img = live ? (a.idx ? a.idx[s] : s) : 0;
    const int S = a.n_sinks;
    int d = 0;
    if (live) {
        float *r = a.r + (size_t)img * a.r_stride;
        if (a.conf[img] >= *a.tau) d = a.exit_sink;
        else {
            bool any = false; float best = 0.f;
#pragma unroll
            for (int i = 0; i < TS; ++i) {
                if (i < S && i != a.exit_sink) {
                    const float v = r[i];
                    if (!any || v > best) { best = v; d = i; any = true; }      // first index on ties (tf.argmax)
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TS; ++i) if (i < S) r[i] = i == d ? 1.f : 0.f;
    }
    // ---- the children's lists: ballot + popcount prefix, one atomic per (wave, sink), as in exit_ev_k ----
    unsigned long long m[TS];
    int base[TS];
#pragma unroll
    for (int i = 0; i < TS; ++i) {
        m[i] = (i < S && a.child_idx[i]) ? __ballot(live && d == i) : 0ull;          // (uniform condition)
        base[i] = 0;
        if (m[i] && lane == 0) base[i] = atomicAdd(a.child_cnt[i], (int)__popcll(m[i]));
    }
#pragma unroll
    for (int i = 0; i < TS; ++i) {
        if (!m[i]) continue;
        const int b0 = __shfl(base[i], 0);
        const int pos = b0 + __popcll(m[i] & ((1ull << lane) - 1ull));
        if (live && d == i && pos >= 0 && pos < a.n) a.child_idx[i][pos] = img;       // (a list holds at most n samples: counts not cleared by the caller must not write past it)
    }
}

extern "C" int mpnn_conf_gate(const mpnn_conf_gate_args *dev_table, int count, int n_max, void *stream) {
    if (count <= 0 || n_max <= 0) return 0;
    if (!dev_table) return MPNN_E_ARG;
    if (count > 65535) return MPNN_E_SHAPE;
    hipLaunchKernelGGL(conf_gate_k, dim3((n_max + CG_THREADS - 1) / CG_THREADS, count), dim3(CG_THREADS), 0, (hipStream_t)stream, dev_table);
    MPNN_LAUNCH_CHECK();
    return 0;
}

// Host-side check of one record (the table itself lives in device memory, so the caller validates each record before
// uploading it).
extern "C" int mpnn_conf_gate_check(const mpnn_conf_gate_args *host_rec) {
    if (!host_rec) return MPNN_E_ARG;
    const mpnn_conf_gate_args &a = *host_rec;
    if (!a.conf || !a.tau || !a.r) return MPNN_E_ARG;
    if (a.n_sinks < 2 || a.n_sinks > TS || a.exit_sink < 0 || a.exit_sink >= a.n_sinks) return MPNN_E_SHAPE;
    if (a.r_stride < a.n_sinks) return MPNN_E_ARG;
    if (a.idx && !a.cnt) return MPNN_E_ARG;
    for (int i = 0; i < TS; ++i) if ((a.child_idx[i] != nullptr) != (a.child_cnt[i] != nullptr)) return MPNN_E_ARG;
    return 0;
}
