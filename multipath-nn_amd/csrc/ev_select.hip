// mpnn_ev_select: the answer of a label-free evaluation -- per sample the exit taken, its class, that class's probability,
// optionally the softmax row, and the operations spent.
//
// The exit kernels store every head's prediction by image (mpnn_exit_ev_args.cls / conf / p_cls).  In a dense pass, and
// in the dense prefix of a routed one, exits also run on samples that never reach them; the routing decision is p_ev
// (mpnn_route), so the sample's exit is chosen here, after mpnn_route: one thread per sample walks the leaves in order,
// the first leaf with p_ev == 1 is the sample's.  Every load and store is coalesced over the samples; the softmax rows
// are copied by the whole workgroup (the chosen leaf of its 256 samples goes through LDS), element by element in row
// order.  The record is a kernel argument: nothing to upload, and a captured graph holds it.
#include "common.h"

#define SEL_T 256

__global__ __launch_bounds__(SEL_T) void ev_select_k(const mpnn_ev_select_args a) {
    __shared__ int leaf_s[SEL_T];
    const int tid = threadIdx.x, s0 = blockIdx.x * SEL_T, s = s0 + tid, n = a.n;
    const bool live = s < n;
    const size_t sv = live ? s : 0;
    // one pass over the nodes' p_ev: the operation count, and the reach bits (n_nodes <= MPNN_MAX_NODES = 128) the leaf
    // walk below reads instead of loading p_ev again
    long long ops = 0;
    unsigned long long reach_lo = 0ull, reach_hi = 0ull;
    for (int j = 0; j < a.n_nodes; ++j)
        if (a.p_ev[(size_t)j * n + sv] == 1.f) {
            ops += a.node_ops[j];
            if (j < 64) reach_lo |= 1ull << j; else reach_hi |= 1ull << (j - 64);
        }
    int leaf = -1;
    for (int l = a.n_leaves - 1; l >= 0; --l) {          // (descending: the FIRST reached leaf stays)
        const int j = a.leaf_node[l];                    // (uniform; 0 <= j < n_nodes is the caller's obligation)
        if (((j < 64 ? reach_lo >> j : reach_hi >> (j - 64)) & 1ull) != 0ull) leaf = l;
    }
    leaf_s[tid] = live ? leaf : -1;
    if (live) {
        const size_t at = (size_t)(leaf >= 0 ? leaf : 0) * a.leaf_stride + sv;
        a.leaf[s] = leaf;
        a.cls[s] = leaf >= 0 ? a.leaf_cls[at] : -1;
        a.conf[s] = leaf >= 0 ? a.leaf_conf[at] : 0.f;
        a.ops[s] = ops;
    }
    if (!a.probs) return;                                // (uniform)
    __syncthreads();
    const int nc = a.n_cls, rows = n - s0 < SEL_T ? n - s0 : SEL_T;
    for (int e = tid; e < rows * nc; e += SEL_T) {
        const int r = e / nc, k = e - r * nc, l = leaf_s[r];
        a.probs[(size_t)s0 * nc + e] = l >= 0 ? a.leaf_p[((size_t)l * a.leaf_stride + s0 + r) * a.p_stride + k] : 0.f;
    }
}

extern "C" int mpnn_ev_select(const mpnn_ev_select_args *args, void *stream) {
    if (!args) return MPNN_E_ARG;
    const mpnn_ev_select_args &a = *args;
    if (a.n_nodes < 1 || a.n_nodes > MPNN_MAX_NODES || a.n_leaves < 1 || a.n_leaves > a.n_nodes) return MPNN_E_SHAPE;
    if (a.n <= 0) return 0;
    if (!a.p_ev || !a.node_ops || !a.leaf_node || !a.leaf_cls || !a.leaf_conf || a.leaf_stride < a.n ||
        !a.leaf || !a.cls || !a.conf || !a.ops) return MPNN_E_ARG;
    if (a.probs && (!a.leaf_p || a.n_cls < 1 || a.p_stride < a.n_cls)) return MPNN_E_ARG;
    hipLaunchKernelGGL(ev_select_k, dim3((a.n + SEL_T - 1) / SEL_T), dim3(SEL_T), 0, (hipStream_t)stream, a);
    MPNN_LAUNCH_CHECK();
    return 0;
}
