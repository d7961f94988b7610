// mpnn_label_map: the labels of an exit that classifies superclasses (reference layer_types.py:274-285, the line
// y_sup = tf.matmul(y, w_cls)) -- y [n][n_cls] times the constant map w_cls [n_cls][n_sup].  One launch: all rows, all
// columns, all records of a table.
//
// A workgroup owns one (record, LM_R rows x LM_S columns of y_sup); a thread owns one element.  The classes go by in
// chunks of LM_C, in class order:
//   1. the chunk of the tile's rows of y into LDS -- LM_C consecutive floats of a row per 64 lanes, coalesced -- and the
//      chunk of the tile's columns of w_cls into LDS (LM_S consecutive floats of a class);
//   2. acc = fmaf(y[r][c], w_cls[c][s], acc) for the classes of the chunk, in order.
// So an element is acc = 0; for c in 0 .. n_cls - 1: acc = fmaf(y[r][c], w_cls[c][s], acc) whatever the tiling, n, n_max
// or the record's place in the table, bit for bit.  Only classes below n_cls enter the chain: nothing is padded, skipped
// or clamped (0 * inf is nan, as in a matmul).  No atomics.  A record with n == 0, the tiles beyond a record's n or
// n_sup: the workgroup leaves before it reads or writes anything.
#include "common.h"

#define LM_R 16                          // rows of a tile
#define LM_S 16                          // columns of a tile
#define LM_C 64                          // classes of a chunk
#define LM_THREADS (LM_R * LM_S)

__global__ __launch_bounds__(LM_THREADS) void label_map_k(const mpnn_label_map_args *__restrict__ table, const int row_tiles) {
    __shared__ float ys[LM_R][LM_C + 1];         // (+ 1: the four rows a wave reads fall on different banks)
    __shared__ float ws[LM_C][LM_S];
    const mpnn_label_map_args a = table[blockIdx.y];
    const int tid = threadIdx.x;
    const int r0 = (blockIdx.x % row_tiles) * LM_R, s0 = (blockIdx.x / row_tiles) * LM_S;
    if (r0 >= a.n || s0 >= a.n_sup) return;      // (uniform over the workgroup)
    const int tr = tid / LM_S, ts = tid % LM_S;
    const bool mine = r0 + tr < a.n && s0 + ts < a.n_sup;
    float acc = 0.0f;
    for (int c0 = 0; c0 < a.n_cls; c0 += LM_C) {
        const int cn = min(LM_C, a.n_cls - c0);
        for (int k = tid; k < LM_R * LM_C; k += LM_THREADS) {
            const int rr = k / LM_C, cc = k % LM_C;
            if (r0 + rr < a.n && cc < cn) ys[rr][cc] = a.y[(size_t)(r0 + rr) * a.n_cls + c0 + cc];
        }
        for (int k = tid; k < LM_C * LM_S; k += LM_THREADS) {
            const int cc = k / LM_S, ss = k % LM_S;
            if (cc < cn && s0 + ss < a.n_sup) ws[cc][ss] = a.w_cls[(size_t)(c0 + cc) * a.n_sup + s0 + ss];
        }
        __syncthreads();
        if (mine)
            for (int c = 0; c < cn; ++c) acc = fmaf(ys[tr][c], ws[c][ts], acc);
        __syncthreads();
    }
    if (mine) a.y_sup[(size_t)(r0 + tr) * a.n_sup + s0 + ts] = acc;
}

extern "C" int mpnn_label_map_check(const mpnn_label_map_args *rec) {
    if (!rec || !rec->y || !rec->w_cls || !rec->y_sup || rec->n < 0) return MPNN_E_ARG;
    if (rec->n_cls < 1 || rec->n_cls > MPNN_LABEL_MAP_MAX_CLS || rec->n_sup < 1 || rec->n_sup > MPNN_LABEL_MAP_MAX_SUP) return MPNN_E_SHAPE;
    return 0;
}

extern "C" int mpnn_label_map(const mpnn_label_map_args *dev_table, int count, int n_max, int n_sup_max, void *stream) {
    if (!dev_table || count < 1 || n_max < 1) return MPNN_E_ARG;
    if (n_sup_max < 1 || n_sup_max > MPNN_LABEL_MAP_MAX_SUP) return MPNN_E_SHAPE;
    const long long row_tiles = ((long long)n_max + LM_R - 1) / LM_R, col_tiles = (n_sup_max + LM_S - 1) / LM_S;
    if (row_tiles * col_tiles > 0x7fffffffLL || count > 65535) return MPNN_E_SHAPE;
    hipLaunchKernelGGL(label_map_k, dim3((unsigned)(row_tiles * col_tiles), (unsigned)count), dim3(LM_THREADS), 0, (hipStream_t)stream,
                       dev_table, (int)row_tiles);
    MPNN_LAUNCH_CHECK();
    return 0;
}
