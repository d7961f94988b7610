// mpnn_exit_curve: the accuracy-versus-operations curve of confidence-threshold exits (Net.exit_conf_curve) -- what every
// image of a labelled batch does under each of T threshold points, summed into T x (correct, operations, exit histogram).
//
// The launch stands BEHIND a dense labelled evaluation whose exit records also stored the predictions: every head's
// confidence (conf) and hit (d_cor) and every switch's router outputs (r) are resident, by image.  What an image does under
// one threshold row is then a walk of at most tree-depth steps over those numbers -- no conv, no head, no router runs again:
//   leaf                        the image exits there
//   one sink                    go there
//   switch (a router) with the exit sink e and tau = taus[t][leaf(e)] not NaN:
//                               e if conf[leaf(e)][img] >= tau (plain fp32: a NaN confidence is "no"), else the arg-max of r
//                               over the sinks other than e (first index on ties) -- the decision of conf_gate_k
//   switch, tau NaN or no e     the arg-max of r over all sinks: the learnt policy
//   static fork (no router: exactly one leaf sink e and one other sink c)
//                               e if tau is not NaN and conf >= tau, else c
// The operations of an image are the sum of node_ops over the nodes it visits (the router of a gated switch included:
// it ran), which is `ops` of predict(exit_conf=).
//
// One thread per image, workgroups of 256; blockIdx.y selects a range of points (the launcher splits them while the grid is
// small).  A workgroup stages ONCE, for its 256 images:
//   * the tree, one 64-bit word per node (four sink ids, the sink count, the exit sink, the switch id and a leaf id -- the
//     node's own, or that of its exit sink: one LDS read per step of the walk), and node_ops;
//   * per switch and image ONE byte: the arg-max of the router row over all sinks (bits 0-1) and over the sinks other than
//     the exit sink (bits 2-3) -- the T walks never read r again;
//   * per leaf and image the confidence (dynamic LDS: the first `n_stage` leaves, as many as fit beside the switch bytes in
//     58 KB -- a tree with more leaves reads the confidences of the others from global memory, where consecutive lanes
//     read consecutive floats);
//   * d_cor == 1 of every leaf as 128 bits in four registers of the image's thread.
// Then it loops over the T points (their thresholds staged in LDS a chunk of points at a time): every thread walks, and each
// wave reduces -- ballot + popcount for `correct` and for every exit leaf that occurs in the wave, a
// shuffle sum for the operations -- and issues ONE integer atomic per counter.  Integer sums: exact, independent of the
// order, bit-identical from run to run; a second launch on another chunk keeps adding.
#include "common.h"

#define XC_T 256
#define XC_MAX_SWITCHES (MPNN_MAX_NODES / 2)
#define XC_TAU_FLOATS 1024        // thresholds staged at a time: 1024 / n_leaves points, at least 8
#define XC_DYN_LDS 59392          // (dynamic LDS of a workgroup: 64 KB less the 6 KB of static tables below)
#define XC_GRID 1024              // workgroups up to which a launch splits its points over grid.y
#define XC_MIN_POINTS 8           // ... and the fewest points of a workgroup
#define TS MPNN_MAX_SINKS

__host__ __device__ static inline int xc_stage_leaves(int n_leaves, int n_switches) {
    const int fit = (XC_DYN_LDS - n_switches * XC_T) / (XC_T * (int)sizeof(float));
    return n_leaves < fit ? n_leaves : fit;
}

// first index on ties, candidates in sink order: the arg-max of exit_ev_k and conf_gate_k
__device__ __forceinline__ int xc_argmax(const float *v, int S, int skip) {
    bool any = false; float best = 0.f; int d = 0;
#pragma unroll
    for (int i = 0; i < TS; ++i)
        if (i < S && i != skip) {
            if (!any || v[i] > best) { best = v[i]; d = i; any = true; }
        }
    return d;
}

__global__ __launch_bounds__(XC_T) void exit_curve_k(const mpnn_exit_curve_args a, const int pts) {
    __shared__ unsigned long long node_s[MPNN_MAX_NODES];
    __shared__ long long ops_s[MPNN_MAX_NODES];
    __shared__ float tau_s[XC_TAU_FLOATS];
    extern __shared__ unsigned char dyn_s[];
    const int tid = threadIdx.x, lane = tid & 63, n = a.n;
    const int img = blockIdx.x * XC_T + tid;
    const bool live = img < n;
    const size_t iv = live ? img : 0;
    const int NN = a.n_nodes, NL = a.n_leaves, NS = a.n_switches;
    const int n_stage = xc_stage_leaves(NL, NS);
    float *conf_s = reinterpret_cast<float *>(dyn_s);                    // [n_stage][XC_T]
    unsigned char *pick_s = dyn_s + (size_t)n_stage * XC_T * sizeof(float);      // [NS][XC_T]

    // ---- the tree: one word per node; ids that are out of range become "none" (the walk never indexes with them) ----
    for (int j = tid; j < NN; j += XC_T) {
        const mpnn_curve_node nd = a.tree[j];
        int ns = nd.n_sinks < 0 ? 0 : nd.n_sinks > TS ? TS : nd.n_sinks;
        unsigned long long w = 0ull;
        for (int i = 0; i < TS; ++i) {
            const int s = i < ns ? nd.sink[i] : 0;
            if (i < ns && (s <= j || s >= NN)) ns = 0;                    // (a child has a larger id than its parent: the walk ends)
            w |= (unsigned long long)(s & 0xff) << (8 * i);
        }
        int e = (ns >= 2 && nd.exit_sink >= 0 && nd.exit_sink < ns) ? nd.exit_sink : -1;
        int leaf = ns == 0 ? nd.leaf_id : (e >= 0 ? a.tree[nd.sink[e]].leaf_id : -1);
        if (leaf < 0 || leaf >= NL) { leaf = -1; e = -1; }
        const int sw = (ns >= 2 && nd.switch_id >= 0 && nd.switch_id < NS) ? nd.switch_id : -1;
        w |= (unsigned long long)ns << 32 | (unsigned long long)(e + 1) << 40 | (unsigned long long)(sw + 1) << 48 |
             (unsigned long long)(leaf + 1) << 56;
        node_s[j] = w;
        ops_s[j] = a.node_ops[j];
    }
    // ---- per switch and image: the router's choice among all sinks, and among the sinks other than the exit sink ----
    for (int j = 0; j < NN; ++j) {
        const mpnn_curve_node nd = a.tree[j];                             // (uniform)
        const int sw = nd.switch_id, S = nd.n_sinks;
        if (sw < 0 || sw >= NS || S < 2 || S > TS) continue;
        const float *row = a.r + (size_t)sw * a.r_switch_stride + iv * a.r_stride;
        float v[TS];
#pragma unroll
        for (int i = 0; i < TS; ++i) v[i] = i < S ? row[i] : 0.f;
        const int e = (nd.exit_sink >= 0 && nd.exit_sink < S) ? nd.exit_sink : -1;
        pick_s[sw * XC_T + tid] = (unsigned char)(xc_argmax(v, S, -1) | xc_argmax(v, S, e) << 2);
    }
    // ---- per leaf and image: the confidence (LDS while it fits), and the hit as one bit ----
    unsigned cor[4] = {0u, 0u, 0u, 0u};
    for (int l = 0; l < NL; ++l) {
        if (l < n_stage) conf_s[l * XC_T + tid] = a.conf[(size_t)l * a.conf_stride + iv];
        const bool hit = a.d_cor[(size_t)l * a.dcor_stride + iv] == 1.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) if ((l >> 5) == q && hit) cor[q] |= 1u << (l & 31);
    }
    unsigned long long *const correct = reinterpret_cast<unsigned long long *>(a.correct);
    unsigned long long *const ops_out = reinterpret_cast<unsigned long long *>(a.ops);
    unsigned long long *const hist = reinterpret_cast<unsigned long long *>(a.hist);

    // The thresholds go through LDS in chunks of XC_TAU_FLOATS / n_leaves points (at least 8), two barriers per CHUNK and
    // none per point: a barrier is also a fence, at which a wave waits for the atomics it has issued, and a threshold read
    // from global memory would put a cache round trip on every step of the walk.
    const int per = a.tau_per_leaf ? NL : 1, tau_step = a.tau_per_leaf ? 1 : 0, chunk = XC_TAU_FLOATS / per;
    const int t_lo = blockIdx.y * pts, t_hi = t_lo + pts < a.n_points ? t_lo + pts : a.n_points;      // this workgroup's points
    for (int t0 = t_lo; t0 < t_hi; t0 += chunk) {
        const int np = t_hi - t0 < chunk ? t_hi - t0 : chunk;
        __syncthreads();                      // (behind the staging above, and behind the readers of the chunk before)
        for (int i = tid; i < np * per; i += XC_T) tau_s[i] = a.taus[(size_t)t0 * per + i];
        __syncthreads();
        for (int t = t0; t < t0 + np; ++t) {
            const float *const tau_t = tau_s + (t - t0) * per;
            int cur = 0, leaf = -1;
            long long ops = 0;
            for (int step = 0; step < NN; ++step) {
                const unsigned long long w = node_s[cur];
                ops += ops_s[cur];
                const int ns = (int)(w >> 32) & 0xff;
                const int lf = (int)(w >> 56) - 1;
                if (ns == 0) { leaf = lf; break; }
                int d = 0;
                if (ns >= 2) {
                    const int e = ((int)(w >> 40) & 0xff) - 1, sw = ((int)(w >> 48) & 0xff) - 1;
                    bool gated = false, out = false;
                    if (e >= 0) {
                        const float tau = tau_t[lf * tau_step];
                        const float c = lf < n_stage ? conf_s[lf * XC_T + tid] : a.conf[(size_t)lf * a.conf_stride + iv];
                        gated = tau == tau;
                        out = c >= tau;                                       // (a NaN on either side is "no")
                    }
                    if (out) d = e;
                    else if (sw >= 0) { const int p = pick_s[sw * XC_T + tid]; d = gated ? p >> 2 : p & 3; }
                    else d = e == 0 ? 1 : 0;                                  // (static fork: the one other sink)
                }
                cur = (int)(w >> (8 * d)) & 0xff;
            }
            const bool done = live && leaf >= 0;
            // ---- one atomic per wave and counter ----
            const int lq = leaf >> 5;
            const unsigned cw = lq == 0 ? cor[0] : lq == 1 ? cor[1] : lq == 2 ? cor[2] : cor[3];
            const bool hit = done && (cw >> (leaf & 31) & 1u) != 0u;
            const unsigned long long m_cor = __ballot(hit);
            long long o = done ? ops : 0;
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) o += __shfl_xor(o, k);
            if (lane == 0) {
                if (m_cor) atomicAdd(correct + t, (unsigned long long)__popcll(m_cor));
                if (o) atomicAdd(ops_out + t, (unsigned long long)o);
            }
            unsigned long long rest = __ballot(done);
            while (rest) {                                                    // (one round per exit that occurs in the wave)
                const int l0 = __shfl(leaf, (int)__ffsll((long long)rest) - 1);
                const unsigned long long m = __ballot(done && leaf == l0);
                if (lane == 0) atomicAdd(hist + (size_t)t * NL + l0, (unsigned long long)__popcll(m));
                rest &= ~m;
            }
        }
    }
}

// Host-side check of a record and of the HOST copy of the tree table it will run on (a.tree itself is device memory).
extern "C" int mpnn_exit_curve_check(const mpnn_exit_curve_args *host_rec, const mpnn_curve_node *host_tree) {
    if (!host_rec || !host_tree) return MPNN_E_ARG;
    const mpnn_exit_curve_args &a = *host_rec;
    if (!a.tree || !a.node_ops || !a.conf || !a.d_cor || !a.taus || !a.correct || !a.ops || !a.hist) return MPNN_E_ARG;
    if (a.n_nodes < 1 || a.n_nodes > MPNN_MAX_NODES || a.n_leaves < 1 || a.n_leaves > a.n_nodes ||
        a.n_switches < 0 || a.n_switches > XC_MAX_SWITCHES || a.n_points < 1 || a.n < 0) return MPNN_E_SHAPE;
    if (a.n_switches > 0 && !a.r) return MPNN_E_ARG;
    if (a.conf_stride < a.n || a.dcor_stride < a.n) return MPNN_E_ARG;
    bool leaf_seen[MPNN_MAX_NODES] = {false};
    for (int j = 0; j < a.n_nodes; ++j) {
        const mpnn_curve_node &nd = host_tree[j];
        if (nd.n_sinks < 0 || nd.n_sinks > TS) return MPNN_E_SHAPE;
        for (int i = 0; i < nd.n_sinks; ++i)
            if (nd.sink[i] <= j || nd.sink[i] >= a.n_nodes) return MPNN_E_SHAPE;      // (children behind their parent: a tree)
        if (nd.n_sinks == 0) {
            if (nd.leaf_id < 0 || nd.leaf_id >= a.n_leaves || leaf_seen[nd.leaf_id]) return MPNN_E_SHAPE;
            leaf_seen[nd.leaf_id] = true;
        } else if (nd.leaf_id >= 0) return MPNN_E_SHAPE;
        if (nd.switch_id >= a.n_switches || (nd.switch_id >= 0 && nd.n_sinks < 2)) return MPNN_E_SHAPE;
        if (nd.switch_id >= 0 && (a.r_stride < nd.n_sinks || a.r_switch_stride < (long long)a.n * a.r_stride)) return MPNN_E_ARG;
        if (nd.exit_sink >= nd.n_sinks || (nd.exit_sink >= 0 && nd.n_sinks < 2)) return MPNN_E_SHAPE;
        if (nd.exit_sink >= 0 && host_tree[nd.sink[nd.exit_sink]].n_sinks != 0) return MPNN_E_SHAPE;
        if (nd.n_sinks >= 2 && nd.switch_id < 0) {                                    // a static fork: one leaf + one other
            if (nd.n_sinks != 2 || nd.exit_sink < 0 || host_tree[nd.sink[1 - nd.exit_sink]].n_sinks == 0) return MPNN_E_SHAPE;
        }
    }
    return 0;
}

extern "C" int mpnn_exit_curve(const mpnn_exit_curve_args *args, void *stream) {
    if (!args) return MPNN_E_ARG;
    const mpnn_exit_curve_args &a = *args;
    if (a.n_nodes < 1 || a.n_nodes > MPNN_MAX_NODES || a.n_leaves < 1 || a.n_leaves > a.n_nodes ||
        a.n_switches < 0 || a.n_switches > XC_MAX_SWITCHES || a.n_points < 1 || a.n < 0) return MPNN_E_SHAPE;
    if (a.n == 0) return 0;
    if (!a.tree || !a.node_ops || !a.conf || !a.d_cor || !a.taus || !a.correct || !a.ops || !a.hist ||
        (a.n_switches > 0 && !a.r) || a.conf_stride < a.n || a.dcor_stride < a.n) return MPNN_E_ARG;
    const size_t dyn = (size_t)xc_stage_leaves(a.n_leaves, a.n_switches) * XC_T * sizeof(float) + (size_t)a.n_switches * XC_T;
    // The points are split over grid.y while the grid stays below XC_GRID workgroups: a chunk of 4 096 images is 16
    // workgroups, and a workgroup spends far longer on its points (a dependent chain per point) than on the staging that
    // every workgroup of a column repeats.  At least XC_MIN_POINTS points per workgroup, so that the staging stays the
    // smaller part.
    const int gx = (a.n + XC_T - 1) / XC_T;
    int gy = (a.n_points + XC_MIN_POINTS - 1) / XC_MIN_POINTS;
    if (gy > XC_GRID / gx) gy = XC_GRID / gx;
    if (gy < 1) gy = 1;
    const int pts = (a.n_points + gy - 1) / gy;
    gy = (a.n_points + pts - 1) / pts;
    hipLaunchKernelGGL(exit_curve_k, dim3(gx, gy), dim3(XC_T), dyn, (hipStream_t)stream, a, pts);
    MPNN_LAUNCH_CHECK();
    return 0;
}
