// General forms of the four multiscale conv contractions, for filters of any size from 1x1 to 7x7:
// mpnn_msconv_fwd_gen / mpnn_msconv_dgrad_horz_gen / mpnn_msconv_dgrad_vert_gen / mpnn_msconv_wgrad_gen, and the same
// kernels on maps of ANY size from 1 to 256 per axis: mpnn_msconv_fwd_hw / _dgrad_horz_hw / _dgrad_vert_hw / _wgrad_hw.
//
// MultiscaleConvMax takes any `supp` (reference scripts/lib/layer_types.py:149-194): w_horz_i is
// min(supp, H_i) x min(supp, W_i) (clipped to the map), w_vert_i is always supp x supp, both applied with TensorFlow's
// SAME padding -- (k - 1) / 2 before and the rest after, so EVEN kernels pad asymmetrically; the input-gradient
// convolution takes the transposed padding (k - 1 - (k - 1) / 2 before).  The tuned bodies (conv_kernel.h,
// conv_strip.h, bwd_*) are specialised for 3x3 and stay as they are; the engine runs a net on these kernels when one of
// its filters is not 3x3 (lib/_eng_alloc.py: generic_convs).  The records are the tuned entry points' (mpnn_hip.h) with
// the weight fields carrying the HWIO tensors themselves: no weight packs.
//
// Forward and input gradients are one implicit GEMM (M = 64 output pixels of a workgroup, N = 64 output channels,
// K = taps x input channels) on v_mfma_f32_16x16x4_f32: per 16-channel chunk the halo tile of the input is staged in
// LDS (BatchNorm + ReLU applied on load), then per tap row the chunk's weights (transposed for the input gradient,
// k-interleaved so one 16-byte LDS read feeds four MFMAs); every wave owns 16 pixels x 64 channels (four independent
// accumulators).  Weight gradients: a workgroup per (pixel split, operand chunk, tap row, 64 output channels) streams
// its split's pixel tiles; every wave owns 16 output channels x 16 input channels for each tap of the row (a GEMM over
// the tile's 64 pixels, the g tile held in registers across the taps).  No scratch; not latency-tuned.
// Both kernels live in conv_gen_k.h; the sample-list form of the forward kernel (routed evaluation:
// mpnn_conv_fwd_args.idx / cnt) is instantiated in conv_gen_list.hip, the forms of the any-channel family
// (mpnn_msconv_*_ch: fitted output tiles, scalar g loads) in conv_gen_ch.hip, which enters through the host side below.
#include "common.h"

#include "conv_gen_k.h"

// ------------------------------- host side -------------------------------
// Output tiles per wave of a forward / input-gradient launch: fitted to Cout in the any-channel family.
static int gen_nt(int fam, int Cout) { return fam != GEN_FAM_CH || Cout > 32 ? 4 : Cout > 16 ? 2 : 1; }

static bool gen_k_ok(int k) { return k >= 1 && k <= GEN_KMAX; }
static bool gen_c16(int c) { return c >= 16 && c <= GEN_CMAX && c % 16 == 0; }

static int gen_chan_check(int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw) {
    if (!(Cin == 1 || Cin == 3 || gen_c16(Cin)) || !gen_c16(Cout)) return MPNN_E_SHAPE;
    if (!gen_k_ok(kh) || !gen_k_ok(kw)) return MPNN_E_SHAPE;
    if (Cv != 0 && (!gen_c16(Cv) || !gen_k_ok(kvh) || !gen_k_ok(kvw))) return MPNN_E_SHAPE;
    return 0;
}

extern "C" int mpnn_msconv_gen_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw) {
    if (H != W || H < 4 || H > 256 || (H != 4 && H % 8)) return MPNN_E_SHAPE;
    return gen_chan_check(Cin, Cv, Cout, kh, kw, kvh, kvw);
}

// The maps of the _hw entry points: any H, W from 1 to 256; channels and filters as mpnn_msconv_gen_check.
extern "C" int mpnn_msconv_hw_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw) {
    if (H < 1 || H > 256 || W < 1 || W > 256) return MPNN_E_SHAPE;
    return gen_chan_check(Cin, Cv, Cout, kh, kw, kvh, kvw);
}
static int gen_shape(int fam, int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw) {
    if (fam == GEN_FAM_CH) return gen_ch_check(H, W, Cin, Cv, Cout, kh, kw, kvh, kvw);
    return fam == GEN_FAM_HW ? mpnn_msconv_hw_check(H, W, Cin, Cv, Cout, kh, kw, kvh, kvw)
                             : mpnn_msconv_gen_check(H, W, Cin, Cv, Cout, kh, kw, kvh, kvw);
}

static GenOp gen_op(const float *x, int C, int shift, int bn, const float *w, int kh, int kw, int Cw_in, int Cw_out, bool dgrad) {
    GenOp o = {};
    o.x = x;  o.C = C;  o.shift = shift;  o.bn = bn;  o.w = w;  o.kh = kh;  o.kw = kw;
    o.wtap = Cw_in * Cw_out;
    if (!dgrad) {                                          // w [kh][kw][C][Cout]: k = input channel
        o.pt = (kh - 1) / 2;  o.pl = (kw - 1) / 2;  o.wk = Cw_out;  o.wn = 1;  o.flip = 0;
    } else {                                               // w [kh][kw][Cout][C]: k = g channel, taps mirrored
        o.pt = kh - 1 - (kh - 1) / 2;  o.pl = kw - 1 - (kw - 1) / 2;  o.wk = 1;  o.wn = Cw_out;  o.flip = 1;
    }
    return o;
}

// A BatchNorm description that cannot be read (the x field is not looked at) / an activation record.
static int gen_bad_bn(const mpnn_act &a) {
    if (a.mode < MPNN_ACT_IDENTITY || a.mode > MPNN_ACT_RELU) return 1;
    if (a.mode == MPNN_ACT_BN_BATCH && (!a.sum || a.cnt < 1 || a.nslot < 1 || a.nslot > MPNN_BN_SLOTS)) return 1;
    if ((a.mode == MPNN_ACT_BN_BATCH || a.mode == MPNN_ACT_BN_MOVING) && (!a.gamma || !a.beta)) return 1;
    return a.mode == MPNN_ACT_BN_MOVING && (!a.m_avg || !a.v_avg);
}
static int gen_bad_act(const mpnn_act &a) { return !a.x || a.C < 1 || a.shift < 0 || a.shift > 8 || gen_bad_bn(a); }

// Every entry point exists three times over one host side: _gen with the limits of mpnn_msconv_gen_check, _hw with those of
// mpnn_msconv_hw_check, both on this file's kernels; _ch (conv_gen_ch.hip) with those of mpnn_msconv_ch_check, on this
// file's kernels where the output is wider than 32 channels (and g is 16-byte aligned) and on its own otherwise.
int gen_fwd(int fam, const mpnn_conv_fwd_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    if (!a || a->n < 0) return MPNN_E_ARG;
    if (gen_shape(fam, a->H, a->W, a->a.C, a->v ? a->Cv : 0, a->Cout, kh, kw, kvh, kvw)) return MPNN_E_SHAPE;
    if (a->pool_out && ((a->H | a->W) & 1)) return MPNN_E_SHAPE;      // (the 2x2 / 2 max-pool takes even maps)
    if (gen_bad_act(a->a) || !a->wa_pack || !a->bias || !a->out) return MPNN_E_ARG;
    if (!a->idx != !a->cnt) return MPNN_E_ARG;
    if (a->idx && (a->out_sum || a->a.mode == MPNN_ACT_BN_BATCH)) return MPNN_E_ARG;      // (sample lists: evaluation only)
    if (a->v && !a->wv_pack) return MPNN_E_ARG;
    if (a->out_sum && (a->out_nslot < 1 || a->out_nslot > MPNN_BN_SLOTS)) return MPNN_E_ARG;
    if (a->a.shift && a->a.mode != MPNN_ACT_IDENTITY) return MPNN_E_ARG;
    if (a->n == 0) return 0;
    GenP p = {};
    p.op[0] = gen_op(a->a.x, a->a.C, a->a.shift, a->a.mode != MPNN_ACT_IDENTITY, a->wa_pack, kh, kw, a->a.C, a->Cout, false);
    p.nops = 1;
    if (a->v) p.op[p.nops++] = gen_op(a->v, a->Cv, 0, 0, a->wv_pack, kvh, kvw, a->Cv, a->Cout, false);
    p.n = a->n;  p.H = a->H;  p.W = a->W;  p.Cout = a->Cout;
    p.bias = a->bias;  p.out = a->out;  p.pool_out = a->pool_out;  p.out_sum = a->out_sum;  p.out_nslot = a->out_nslot;
    p.a = a->a;  p.idx = a->idx;  p.cnt = a->cnt;
    const GenGeo g = gen_geo(a->n, a->H, a->W);
    const int nt = gen_nt(fam, a->Cout);
    const dim3 grid(g.tiles, (a->Cout + 16 * nt - 1) / (16 * nt));
    if (nt < 4) return gen_ch_launch(GEN_FWD, a->idx != nullptr, nt, p, grid, (hipStream_t)stream);      // (conv_gen_ch.hip)
    if (a->idx) return gen_fwd_list_launch(p, grid, (hipStream_t)stream);      // (conv_gen_list.hip)
    hipLaunchKernelGGL(gen_conv_k<GEN_FWD>, grid, dim3(256), 0, (hipStream_t)stream, p);
    MPNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mpnn_msconv_fwd_gen(const mpnn_conv_fwd_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    return gen_fwd(GEN_FAM_GEN, a, kh, kw, kvh, kvw, stream);
}
extern "C" int mpnn_msconv_fwd_hw(const mpnn_conv_fwd_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    return gen_fwd(GEN_FAM_HW, a, kh, kw, kvh, kvw, stream);
}

int gen_dgrad_horz(int fam, const mpnn_dgrad_horz_args *a, int kh, int kw, void *stream) {
    if (!a || a->n < 0) return MPNN_E_ARG;
    if (gen_shape(fam, a->H, a->W, a->Cout, 0, a->Cg, kh, kw, 0, 0) || (fam != GEN_FAM_CH && a->Cout % 16)) return MPNN_E_SHAPE;
    if (!a->g || !a->w_pack || !a->out || a->g_ctx) return MPNN_E_ARG;
    if (a->prev && (!a->prev->s || !a->red_out || a->prev->bn.C != a->Cout || a->prev->bn.mode == MPNN_ACT_IDENTITY ||
                    gen_bad_bn(a->prev->bn))) return MPNN_E_ARG;
    if (a->prev && (a->prev->red_nslot < 1 || a->prev->red_nslot > MPNN_BN_SLOTS)) return MPNN_E_ARG;
    if (a->n == 0) return 0;
    GenP p = {};
    p.op[0] = gen_op(a->g, a->Cg, 0, 0, a->w_pack, kh, kw, a->Cout, a->Cg, true);
    p.nops = 1;
    p.n = a->n;  p.H = a->H;  p.W = a->W;  p.Cout = a->Cout;
    p.extra = a->dy_extra;  p.out = a->out;  p.acc_out = a->accumulate ? 1 : 0;
    const GenGeo g = gen_geo(a->n, a->H, a->W);
    const int nt = gen_nt(fam, a->Cout);
    const dim3 grid(g.tiles, (a->Cout + 16 * nt - 1) / (16 * nt));
    if (a->prev) { p.sprev = a->prev->s;  p.pbn = a->prev->bn;  p.red_out = a->red_out;  p.red_out_nslot = a->prev->red_nslot; }
    if (nt < 4) return gen_ch_launch(a->prev ? GEN_DGH_BN : GEN_DGH_RAW, false, nt, p, grid, (hipStream_t)stream);
    if (a->prev) {
        hipLaunchKernelGGL(gen_conv_k<GEN_DGH_BN>, grid, dim3(256), 0, (hipStream_t)stream, p);
    } else {
        hipLaunchKernelGGL(gen_conv_k<GEN_DGH_RAW>, grid, dim3(256), 0, (hipStream_t)stream, p);
    }
    MPNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mpnn_msconv_dgrad_horz_gen(const mpnn_dgrad_horz_args *a, int kh, int kw, void *stream) {
    return gen_dgrad_horz(GEN_FAM_GEN, a, kh, kw, stream);
}
extern "C" int mpnn_msconv_dgrad_horz_hw(const mpnn_dgrad_horz_args *a, int kh, int kw, void *stream) {
    return gen_dgrad_horz(GEN_FAM_HW, a, kh, kw, stream);
}

// (H x W: the coarse map; the fine map of the pooled operand is 2H x 2W, even on both axes by construction)
int gen_dgrad_vert(int fam, const mpnn_dgrad_vert_args *a, int kvh, int kvw, void *stream) {
    if (!a || a->n < 0) return MPNN_E_ARG;
    if (gen_shape(fam, a->H, a->W, a->Cout, 0, a->Cg, kvh, kvw, 0, 0) || (fam != GEN_FAM_CH && a->Cout % 16)) return MPNN_E_SHAPE;
    if (!a->g || !a->w_pack || !a->fine || !a->fine->s || !a->dz_g_fine || a->g_ctx) return MPNN_E_ARG;
    const mpnn_bn_ctx &f = *a->fine;
    if (f.bn.C != a->Cout || f.bn.mode == MPNN_ACT_IDENTITY || gen_bad_bn(f.bn)) return MPNN_E_ARG;
    if (a->fine_has_dz && f.red && (f.red_nslot < 1 || f.red_nslot > MPNN_BN_SLOTS)) return MPNN_E_ARG;
    if (a->n == 0) return 0;
    GenP p = {};
    p.op[0] = gen_op(a->g, a->Cg, 0, 0, a->w_pack, kvh, kvw, a->Cout, a->Cg, true);
    p.nops = 1;
    p.n = a->n;  p.H = a->H;  p.W = a->W;  p.Cout = a->Cout;
    p.out = a->dz_g_fine;  p.sprev = f.s;  p.pbn = f.bn;
    p.red = a->fine_has_dz ? f.red : nullptr;  p.has_dz = a->fine_has_dz ? 1 : 0;
    p.red_nslot = f.red_nslot < 1 ? 1 : f.red_nslot;
    const GenGeo g = gen_geo(a->n, a->H, a->W);
    const int nt = gen_nt(fam, a->Cout);
    const dim3 grid(g.tiles, (a->Cout + 16 * nt - 1) / (16 * nt));
    if (nt < 4) return gen_ch_launch(GEN_DGV, false, nt, p, grid, (hipStream_t)stream);
    hipLaunchKernelGGL(gen_conv_k<GEN_DGV>, grid, dim3(256), 0, (hipStream_t)stream, p);
    MPNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mpnn_msconv_dgrad_vert_gen(const mpnn_dgrad_vert_args *a, int kvh, int kvw, void *stream) {
    return gen_dgrad_vert(GEN_FAM_GEN, a, kvh, kvw, stream);
}
extern "C" int mpnn_msconv_dgrad_vert_hw(const mpnn_dgrad_vert_args *a, int kvh, int kvw, void *stream) {
    return gen_dgrad_vert(GEN_FAM_HW, a, kvh, kvw, stream);
}

// Pixel tiles of a map (the most useful n_split), or MPNN_E_SHAPE.
extern "C" int mpnn_msconv_gen_tiles(int n, int H, int W) {
    if (n < 1 || H != W || H < 4 || H > 256 || (H != 4 && H % 8)) return MPNN_E_SHAPE;
    return gen_geo(n, H, W).tiles;
}
extern "C" int mpnn_msconv_hw_tiles(int n, int H, int W) {
    if (n < 1 || H < 1 || H > 256 || W < 1 || W > 256) return MPNN_E_SHAPE;
    return gen_geo(n, H, W).tiles;
}

int gen_wgrad(int fam, const mpnn_wgrad_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    if (!a || a->n < 0) return MPNN_E_ARG;
    if (gen_shape(fam, a->H, a->W, a->a.C, a->v ? a->Cv : 0, a->Cout, kh, kw, kvh, kvw)) return MPNN_E_SHAPE;
    if (gen_bad_act(a->a) || !a->g || !a->dwa || !a->db || a->g_ctx || a->n_split < 1 || a->n_split > 65535) return MPNN_E_ARG;
    if (a->v && !a->dwv) return MPNN_E_ARG;
    if (a->a.shift && a->a.mode != MPNN_ACT_IDENTITY) return MPNN_E_ARG;
    if (a->n_split > 1 && a->split_stride < (long)kh * kw * a->a.C * a->Cout) return MPNN_E_ARG;
    if (a->n == 0) return 0;
    GenWP p = {};
    p.op[0] = gen_op(a->a.x, a->a.C, a->a.shift, a->a.mode != MPNN_ACT_IDENTITY, nullptr, kh, kw, a->a.C, a->Cout, false);
    p.nops = 1;
    if (a->v) p.op[p.nops++] = gen_op(a->v, a->Cv, 0, 0, nullptr, kvh, kvw, a->Cv, a->Cout, false);
    p.g = a->g;  p.dw[0] = a->dwa;  p.dw[1] = a->dwv;  p.db = a->db;  p.split_stride = a->split_stride;
    p.n = a->n;  p.H = a->H;  p.W = a->W;  p.Cout = a->Cout;  p.n_split = a->n_split;
    p.a = a->a;
    const int items = ((a->a.C + 15) / 16) * kh + (a->v ? ((a->Cv + 15) / 16) * kvh : 0);
    const dim3 grid(a->n_split, items, (a->Cout + 63) / 64);
    if (a->Cout % 4) return gen_ch_wgrad_launch(p, grid, (hipStream_t)stream);      // (_ch only: conv_gen_ch.hip)
    hipLaunchKernelGGL(gen_wgrad_k<>, grid, dim3(256), 0, (hipStream_t)stream, p);
    MPNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mpnn_msconv_wgrad_gen(const mpnn_wgrad_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    return gen_wgrad(GEN_FAM_GEN, a, kh, kw, kvh, kvw, stream);
}
extern "C" int mpnn_msconv_wgrad_hw(const mpnn_wgrad_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    return gen_wgrad(GEN_FAM_HW, a, kh, kw, kvh, kvw, stream);
}
