/*
 * mpnn_hip.h -- C ABI of libmpnn_hip.so, the MI355X (gfx950) kernel library for
 * the multipath-nn training hot path.
 *
 * The reference (MasonMcGill/multipath-nn) has no FFI: its boundary is the
 * Python class protocol of scripts/lib/layer_types.py + scripts/lib/net_types.py
 * whose arithmetic is delegated to TensorFlow ops.  Each entry point below
 * replaces the TensorFlow op call sites it cites (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated; activations NHWC fp32,
 *     filters HWIO fp32 (TensorFlow defaults, net_types.py:50-51);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     allocates nothing, never synchronises and is hipGraph-capturable;
 *   - return value: 0 = launched, >0 = hipError_t, <0 = MPNN_E_* (bad shape);
 *     nothing throws across the ABI;
 *   - "pre-activation" buffers hold the conv sums BEFORE BatchNorm; BatchNorm
 *     (+ReLU) is applied by the consumer while loading (mpnn_act).
 */
#ifndef MPNN_HIP_H
#define MPNN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MPNN_MAX_NODES 128     /* routing-tree nodes (mpnn_route)            */
#define MPNN_MAX_SINKS 4       /* children of one switch                      */

#define MPNN_E_SHAPE   (-1)   /* unsupported geometry / channel count      */
#define MPNN_E_ARG     (-2)   /* inconsistent arguments                     */

/* BatchNorm statistics are accumulated with fp64 atomics into MPNN_BN_SLOTS
 * replicated slots (a workgroup adds to slot blockIdx % nslot) so that
 * thousands of workgroups do not serialise on one address; readers add the
 * slots.  A statistics buffer is [MPNN_BN_SLOTS][2*C] doubles of which the
 * first `nslot` are used (few slots for layers with few workgroups: every
 * consumer workgroup re-adds them in its prologue).  MPNN_BN_SLOTS is the CAPACITY callers size
 * the buffers for; every record carries the number actually used (mpnn_act.nslot, out_nslot,
 * red_nslot: the engine uses 8 everywhere, lib/_plan.py:_nslot -- measured best). */
#define MPNN_BN_SLOTS 16

#define MPNN_ACT_IDENTITY 0   /* raw values (pyramid input, gradients)      */
#define MPNN_ACT_BN_BATCH 1   /* relu(bn(x)) with batch statistics ('tr')   */
#define MPNN_ACT_BN_MOVING 2  /* relu(bn(x)) with moving averages  ('ev')   */
#define MPNN_ACT_RELU 3       /* relu(x): the `Rect` after a plain `Conv` (layer_types.py:76-79) */

/* An activation as its consumer sees it: pre-activation values plus the
 * BatchNorm + ReLU to apply on load.  Replaces BatchNorm.link / Rect.link /
 * MultiscaleBatchNorm.link / MultiscaleRect.link (layer_types.py:219-249,
 * 76-79, 196-199) and ToPyramid.link's strided pick (layer_types.py:118-125:
 * `shift` = log2 of the subsampling factor). */
typedef struct {
    const float  *x;       /* [n, H<<shift, W<<shift, C]                      */
    const double *sum;     /* [SLOTS][2*C]: sum, sum of squares over (n,H,W)  */
    const float  *gamma, *beta, *m_avg, *v_avg;   /* [C] each                 */
    float eps;             /* BatchNorm eps (layer_types.py:220)              */
    int   cnt;             /* n*H*W: element count behind `sum`               */
    int   C;
    int   shift;
    int   mode;            /* MPNN_ACT_*                                       */
    int   nslot;           /* slots of `sum` actually in use (1..MPNN_BN_SLOTS) */
} mpnn_act;

/* The activation MATERIALISED: y = relu(bn(x)) (identity mode: a copy), [n_pix, C] -- exactly what
 * the consumers compute while loading (same coefficients, same expression).  The hot path never
 * needs it (nothing post-ReLU is stored); callers that want a block's output tensor do, and the
 * parity tests read the ReLU decisions of the device from it.  Any C from 1 to 512, shift == 0 (C % 4 == 0 and
 * C <= 256: the quad kernel, as before; C % 4 != 0 or C > 256: channel = element index mod C, 16-byte accesses where
 * C % 4 == 0). */
int mpnn_bn_relu_fwd(const mpnn_act *a, float *y, long n_pix, void *stream);

/* ---- weight packing ------------------------------------------------------
 * HWIO [3][3][Cin][Cout] -> forward pack [9][ceil(Cin/16)][4][Cout][4]
 * (k-interleaved so one 16-byte load feeds four v_mfma_f32_16x16x4_f32) and
 * transposed+flipped pack for the input-gradient convolution.
 * One launch packs `n_desc` tensors described by the device table `desc`
 * (6 ints each: src_off, fwd_off, bwd_off, Cin, Cout, reserved; offsets in
 * floats relative to `params` / `packs`). */
int mpnn_pack_weights(const float *params, float *packs, const int *desc,
                      int n_desc, void *stream);

/* First launch of a training step: mpnn_pack_weights plus clearing `zero_bytes` bytes at `zero`
 * (both multiples of 16; the step's accumulators: BatchNorm statistic slots, loss sums, gradient
 * tensor) in the same kernel -- one launch instead of a pack and two memsets. */
int mpnn_step_begin(const float *params, float *packs, const int *desc, int n_desc,
                    void *zero, long zero_bytes, void *stream);
/* (n_desc == 0: clear only -- the packs are kept current by mpnn_talr_momentum_step.) */

/* ---- multiscale conv block, forward --------------------------------------
 * One scale of MultiscaleConvMax.link (layer_types.py:181-185):
 *   out = bias + conv3x3_same(act(a)) [+ conv3x3_same(v)]
 * and, fused, the per-channel sum / sum-of-squares that BatchNorm's
 * tf.nn.moments needs (layer_types.py:232) and, if `pool_out` is given, the
 * 2x2/2 max-pool of `out` (the `pool(self.x[i-1])` of layer_types.py:185 that
 * the next coarser scale consumes: pooled ONCE, by the producer).  `v` is that
 * pooled PRE-BN map of the next finer scale, [n, H, W, Cv] (NULL for the first
 * scale). */
typedef struct {
    mpnn_act a;
    const float *v;  int Cv;
    const float *wa_pack;  const float *wv_pack;   /* forward packs           */
    const float *bias;                              /* [Cout]                  */
    float  *out;                                    /* [n, H, W, Cout]         */
    float  *pool_out;                               /* [n, H/2, W/2, Cout] or NULL; the tuned entry points take it on maps
                                                     * with H >= 8 and even H, W (MPNN_E_SHAPE otherwise) */
    double *out_sum;                                /* [SLOTS][2*Cout], accumulated */
    int out_nslot;                                  /* slots of out_sum to spread over */
    int n, H, W, Cout;
    /* Routed evaluation (mpnn_msconv_fwd_group, mpnn_msconv_fwd_gen, _hw and _ch; 'ev' mode, BatchNorm moving
     * averages or an identity / image operand -- never batch statistics, never with out_sum): when
     * `idx` is set, the launch processes the *cnt samples idx[0..*cnt) -- sample slot s is image
     * idx[s] of EVERY buffer of the record (a, v, out, pool_out): inputs are gathered and results
     * scattered by the tile loader / epilogue themselves, nothing is copied.  `cnt` is read on the
     * DEVICE when the kernel starts (written by an earlier mpnn_exit_ev on the same stream: no host
     * sync); `n` stays the capacity the grid is sized for.  The samples that did not reach this
     * node keep whatever the buffers held; a listed sample gets the bits the launch without a list
     * gives it.  Replaces the 0/1 masks p_ev of net_types.py:127-131.  Refused with MPNN_E_ARG before
     * anything is launched: one of idx / cnt alone, a group where only some members carry a list, a
     * list with out_sum or under MPNN_ACT_BN_BATCH, a list on mpnn_msconv_fwd or
     * mpnn_msconv_fwd_group_rep. */
    const int *idx;
    const int *cnt;
} mpnn_conv_fwd_args;
int mpnn_msconv_fwd(const mpnn_conv_fwd_args *args, void *stream);
/* Up to four mutually independent forward convs (one wavefront level of the block x scale grid)
 * as ONE launch; `args` is a HOST array of `count` records (sizes the grid) and `dev_args` a
 * DEVICE copy of it (read by the kernel; uploaded once per plan).  The grid is 1-D, holds exactly
 * the workgroups that have work and is fitted to what is resident at once, shared between the
 * members by work.  A single member on an 8x8 / 4x4 map with >= 64 input channels (multiples of
 * 32 per operand) in TRAINING mode (a.mode == MPNN_ACT_BN_BATCH) takes the K-split body (512
 * threads, two chunks of a 32-channel unit in parallel); results are the same up to fp32 summation
 * order.  Evaluation-mode launches never take it.  Members on maps with W % 16 == 0 whose input is
 * one to three 16-channel chunks -- or a 1/3-channel image plus a 16-channel operand V (block 0's
 * second scale) -- take the wave-per-strip bodies of conv_strip.h when the record's sample capacity
 * `n` is >= 512 (MPNN_STRIP: minimum, 0 = off), in training mode (batch statistics) as in evaluation
 * mode: the one-chunk body gives the same bits as mpnn_msconv_fwd, the multi-chunk / image + V bodies
 * the same values up to fp32 summation order.  Groups of 8x8 / 4x4 members with Cout % 32 == 0 in evaluation mode and
 * `n` >= 1024 (MPNN_FWD_WIDE) use 32-channel output tiles: the same bits.  Which body runs depends only on the shapes and on `n` -- never on the
 * grouping, the index list or the device-side count -- so a conv gives bit-identical rows on all
 * samples or on a routed sub-batch of the same capacity. */
int mpnn_msconv_fwd_group(const mpnn_conv_fwd_args *args, const mpnn_conv_fwd_args *dev_args, int count,
                          void *stream);
/* CO-TRAINING (no reference counterpart in one call: scripts/train-nets:81-88,159-164 trains the nets of an experiment one
 * after another, each at batch 128 -- one net cannot fill 256 compute units).  The `_rep` / `_multi` entry points run the
 * SAME launch of `reps` nets of one architecture as ONE grid: `args` / `dev_args` hold reps * count records, net r's at
 * [r * count, (r + 1) * count) -- identical shapes and modes, every pointer net r's own (its batch, its parameters, its
 * BatchNorm statistics).  Per net the arithmetic is that of the single-net launch on resident slots / reps. */
int mpnn_msconv_fwd_group_rep(const mpnn_conv_fwd_args *args, const mpnn_conv_fwd_args *dev_args, int count,
                              int reps, int share, void *stream);
/* (share: every net's grid is sized for resident slots / share; <= 0 means reps.  reps = 1 with share = K launches ONE net
 * with exactly the grid it has inside a joint launch of K.  Refused with MPNN_E_ARG before anything is launched: reps < 1,
 * count > 4, nets that differ in a shape, a mode or the presence of v / pool_out / out_sum, and, in ANY of the reps * count
 * records, a NULL a.x, wa_pack, bias or out, or a v without wv_pack.) */

/* ---- BatchNorm(+ReLU) backward pieces ------------------------------------
 * Backward of `y = relu(gamma * (s - m) / sqrt(v + eps) + beta)` THROUGH the
 * batch statistics (autodiff of layer_types.py:231-236):
 *   dz   = dy * [y > 0]
 *   red  = [sum dz, sum dz * xhat]                 (-> dbeta, dgamma)
 *   g    = gamma*rstd * (dz - red0/cnt - xhat*red1/cnt)
 * mpnn_bn_bwd_reduce computes dz and accumulates red; mpnn_bn_bwd_apply
 * turns dz into g in place once red is complete.  Any C from 1 to 512: the
 * quad kernels where C % 4 == 0, (C / 4) | 256 and C <= 256; for every other C
 * (48 and 96 included) kernels that take channel = element index mod C (per-workgroup partials added
 * in a fixed order, then one fp64 atomic per channel and slot). */
typedef struct {
    const float *s;        /* pre-BN values [n,H,W,C]                          */
    mpnn_act bn;           /* the BatchNorm of s (x field unused)              */
    const double *red;     /* [SLOTS][2*C] sum dz, sum dz*xhat (NULL: zero)    */
    int red_nslot;         /* slots of red in use                              */
} mpnn_bn_ctx;
int mpnn_bn_bwd_reduce(const float *dy, const mpnn_bn_ctx *ctx, float *dz,
                       double *red_out, long n_pix, void *stream);
int mpnn_bn_bwd_apply(float *dz_inout, const mpnn_bn_ctx *ctx, long n_pix,
                      void *stream);

/* ---- multiscale conv block, input gradients --------------------------------
 * mpnn_msconv_dgrad_horz: dy = conv3x3_same^T(g, w_horz) [+ dy_extra], i.e. the
 * gradient w.r.t. the block's (post-ReLU) input at this scale, fused with the
 * producer's mpnn_bn_bwd_reduce (prev != NULL) or stored raw (prev == NULL).
 * mpnn_msconv_dgrad_vert: dv = conv3x3_same^T(g, w_vert) at the coarse scale,
 * routed through the 2x2 max-pool to the FIRST maximum of each window of the
 * finer pre-BN map and added to that map's BatchNorm backward:
 *   g_fine = bn_bwd_apply(dz_fine) + maxpool_bwd(dv)        (in place on dz_fine)
 * Autodiff of layer_types.py:181-185. */
typedef struct {
    const float *g;  int Cg;            /* [n,H,W,Cg] gradient w.r.t. pre-BN sums */
    const mpnn_bn_ctx *g_ctx;            /* non-NULL: `g` holds dz and the BatchNorm backward
                                            (mpnn_bn_bwd_apply) is applied while loading it */
    const float *w_pack;                 /* backward pack                          */
    const float *dy_extra;               /* [n,H,W,Cout] or NULL                   */
    const mpnn_bn_ctx *prev;             /* producer BatchNorm context or NULL     */
    float  *out;                         /* dz (prev != NULL) or dy                */
    double *red_out;                     /* [SLOTS][2*Cout] accumulated (prev != NULL) */
    int n, H, W, Cout;
    int accumulate;                      /* 1: out += result (a map feeding SEVERAL child blocks, tree nets:
                                            the ReLU mask and the reductions are linear in dy, so each child's
                                            launch adds its own masked share) */
} mpnn_dgrad_horz_args;
int mpnn_msconv_dgrad_horz(const mpnn_dgrad_horz_args *args, void *stream);

typedef struct {
    const float *g;  int Cg;            /* coarse gradient [n,H,W,Cg]             */
    const mpnn_bn_ctx *g_ctx;            /* as in mpnn_dgrad_horz_args              */
    const float *w_pack;                 /* backward pack of w_vert                */
    const mpnn_bn_ctx *fine;             /* BatchNorm context of the finer scale   */
    int fine_has_dz;                     /* 0: finer BN output has no consumer     */
    float *dz_g_fine;                    /* [n,2H,2W,Cout]: dz in, g out           */
    int n, H, W, Cout;                   /* H, W = COARSE size; Cout = fine chans  */
} mpnn_dgrad_vert_args;
int mpnn_msconv_dgrad_vert(const mpnn_dgrad_vert_args *args, void *stream);
/* Both input gradients of one scale (same g, independent outputs) as ONE launch. */
int mpnn_msconv_dgrad_pair(const mpnn_dgrad_horz_args *horz, const mpnn_dgrad_vert_args *vert,
                           void *stream);

/* ---- multiscale conv block, weight gradients -------------------------------
 * dW_horz = act(a)^T (*) g, dW_vert = v^T (*) g (v = the pooled finer map, as in
 * mpnn_conv_fwd_args), db = sum g.
 * The pixel range is divided over `n_split` workgroup rows; split s WRITES its
 * partial sums (plain stores, every element exactly once) to dwa/dwv/db +
 * s*split_stride.  With n_split == 1 those may be the gradient tensors
 * themselves; otherwise they point into a scratch slab and mpnn_slab_reduce
 * adds the splits in a fixed order (bitwise-reproducible gradients; fp32
 * atomics from hundreds of workgroups onto a few-KB tensor serialise). */
typedef struct {
    mpnn_act a;
    const float *v;  int Cv;
    const float *g;                      /* [n,H,W,Cout]                           */
    const mpnn_bn_ctx *g_ctx;            /* as in mpnn_dgrad_horz_args              */
    float *dwa;  float *dwv;  float *db; /* HWIO partial sums of split 0, [Cout]   */
    long split_stride;                   /* floats between consecutive splits      */
    int n, H, W, Cout;
    int n_split;
} mpnn_wgrad_args;
int mpnn_msconv_wgrad(const mpnn_wgrad_args *args, void *stream);
/* Everything the backward pass does with g of one scale -- dgrad-horz (NULL: none), dgrad-vert
 * (NULL: none) and the weight gradients -- as ONE launch of independent workgroups. */
int mpnn_msconv_bwd_scale(const mpnn_dgrad_horz_args *horz, const mpnn_dgrad_vert_args *vert,
                          const mpnn_wgrad_args *wgrad, void *stream);
/* One DEPENDENCY LEVEL of the backward pass as one launch: g(b, S) (block b, absolute scale S) is final once
 * the child block's dgrad-horz B(b+1, S) and the coarser scale's dgrad-vert B(b, S+1) have run, so the
 * mpnn_msconv_bwd_scale triples with equal (blocks from the end) + (scales from the coarsest) are mutually
 * independent (autodiff of layer_types.py:181-185; the reference leaves the order to TensorFlow's executor,
 * net_types.py:35).  Members must not write the same output map (tree nets: siblings that accumulate into one
 * parent map go to different launches).  The CALLER budgets the workgroups: wg_horz / wg_vert = workgroups per
 * 16-channel tile row of the two input-gradient bodies, wgrad->n_split = pixel split of the weight gradients;
 * mpnn_msconv_bwd_level_slots gives the workgroups that are resident at once for a set of member shapes
 * (H, W, Cout of g), or MPNN_E_SHAPE when no kernel variant covers the set.
 * The member records live in DEVICE memory: _prepare fills `count` records of _record_size() bytes in host
 * memory, the caller copies them to the device once per plan and passes the device pointer to every launch. */
#define MPNN_BWD_LEVEL_MAX 4
typedef struct {
    const mpnn_dgrad_horz_args *horz;    /* NULL: none */
    const mpnn_dgrad_vert_args *vert;    /* NULL: none */
    const mpnn_wgrad_args *wgrad;
    int wg_horz, wg_vert;
} mpnn_bwd_member;
int mpnn_msconv_bwd_level_record_size(void);
int mpnn_msconv_bwd_level_slots(const int *H, const int *W, const int *Cout, int count);
int mpnn_msconv_bwd_level_prepare(const mpnn_bwd_member *members, int count, void *host_records);
int mpnn_msconv_bwd_level(const mpnn_bwd_member *members, int count, const void *dev_records, void *stream);
/* One dependency level of `reps` co-trained nets (see mpnn_msconv_fwd_group_rep): reps * count members / records, net r's
 * at [r * count, ...); the same shapes and the same workgroup budgets in every net (budget against _slots / reps). */
int mpnn_msconv_bwd_level_prepare_rep(const mpnn_bwd_member *members, int count, int reps, void *host_records);
int mpnn_msconv_bwd_level_rep(const mpnn_bwd_member *members, int count, int reps, const void *dev_records, void *stream);
/* Number of 64-pixel tiles (upper bound of n_split) for a map, or MPNN_E_SHAPE. */
int mpnn_wgrad_tiles(int n, int H, int W);
/* dst[i] = sum_{s<n_split} src[s*stride + i].  table: 6 ints per work item:
 * src_off (floats in `slabs`), dst_off (floats in `grads`), count (<= MPNN_SLAB_ITEM),
 * n_split, stride, reserved.  One workgroup per item; a larger count is MPNN_E_ARG-free
 * undefined behaviour, so split larger tensors into several items. */
#define MPNN_SLAB_ITEM 1024
int mpnn_slab_reduce(const float *slabs, float *grads, const int *table, int n_items,
                     void *stream);

/* ---- multiscale conv block with filters of ANY size (csrc/conv_gen.hip) ------------------------------------------------
 * MultiscaleConvMax takes any `supp` (layer_types.py:149-194): w_horz_i is min(supp, H_i) x min(supp, W_i), w_vert_i
 * supp x supp, applied with TensorFlow's SAME padding ((k - 1) / 2 before, k - 1 - (k - 1) / 2 after: even sizes pad
 * asymmetrically; the input-gradient convolutions take the transposed padding).  The tuned entry points above are 3x3
 * only; these take the SAME records with the weight fields carrying the HWIO TENSORS (no packs) and the filter geometry
 * as arguments: kh x kw of w_horz, kvh x kvw of w_vert.  Semantics as the tuned forms, with these differences:
 *   mpnn_msconv_fwd_gen        == mpnn_msconv_fwd; wa_pack = w_horz [kh][kw][a.C][Cout], wv_pack = w_vert
 *                                 [kvh][kvw][Cv][Cout]; sample lists (idx / cnt) as mpnn_msconv_fwd_group: both set or
 *                                 neither, and only without out_sum and batch statistics (MPNN_E_ARG otherwise); the
 *                                 pixel tiles are laid over the list's slots, a slot beyond *cnt is computed on zeros
 *                                 and stored nowhere
 *   mpnn_msconv_dgrad_horz_gen == mpnn_msconv_dgrad_horz; w_pack = w_horz [kh][kw][Cout][Cg]
 *   mpnn_msconv_dgrad_vert_gen == mpnn_msconv_dgrad_vert; w_pack = w_vert [kvh][kvw][Cout][Cg], H x W = coarse size
 *   mpnn_msconv_wgrad_gen      == mpnn_msconv_wgrad; dwa / dwv are HWIO like the weights; any n_split >= 1 (splits
 *                                 beyond mpnn_msconv_gen_tiles write zeros)
 * g_ctx is not offered (MPNN_E_ARG): the caller runs mpnn_bn_bwd_apply on g first.  Limits (mpnn_msconv_gen_check, host
 * only): square maps H == W of 4 or a multiple of 8 up to 256; filters 1..7 on each side; Cin 1, 3 or a multiple of 16,
 * Cv 0 or a multiple of 16, Cout a multiple of 16, all <= 512 (Cin is the output of dgrad-horz, Cv the output of
 * dgrad-vert: multiples of 16).  Returns 0 or MPNN_E_SHAPE.  Deterministic: no fp32 atomics (the BatchNorm sums are fp64
 * slot atomics, as everywhere). */
int mpnn_msconv_gen_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw);
int mpnn_msconv_gen_tiles(int n, int H, int W);      /* 64-pixel tiles of an n x H x W map, or MPNN_E_SHAPE */
int mpnn_msconv_fwd_gen(const mpnn_conv_fwd_args *args, int kh, int kw, int kvh, int kvw, void *stream);
int mpnn_msconv_dgrad_horz_gen(const mpnn_dgrad_horz_args *args, int kh, int kw, void *stream);
int mpnn_msconv_dgrad_vert_gen(const mpnn_dgrad_vert_args *args, int kvh, int kvw, void *stream);
int mpnn_msconv_wgrad_gen(const mpnn_wgrad_args *args, int kh, int kw, int kvh, int kvw, void *stream);

/* ---- the same four contractions on maps of ANY size (csrc/conv_gen.hip, the same kernels) ------------------------------
 * The _gen forms keep their limits; these take the same records and arguments with 1 <= H, W <= 256 INDEPENDENTLY
 * (rectangular maps, odd sides, maps one pixel wide; mpnn_msconv_hw_check: channels and filters as
 * mpnn_msconv_gen_check).  The pixel tiles are 8 or 4 pixels per axis (8 on an axis longer than 4) and may hang over the
 * bottom / right edge: pixels beyond the map are stored nowhere and add nothing to the BatchNorm sums, to dW or to db
 * (a.cnt / the statistics' count stay n * H * W).  mpnn_msconv_fwd_hw with pool_out needs even H and W (MPNN_E_SHAPE
 * otherwise) and takes sample lists as mpnn_msconv_fwd_gen does, overhanging tiles included; the fine map of
 * mpnn_msconv_dgrad_vert_hw is 2H x 2W.  On a shape both families accept, _hw and _gen
 * write the same bits.  mpnn_msconv_hw_tiles == mpnn_msconv_gen_tiles wherever the latter is defined. */
int mpnn_msconv_hw_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw);
int mpnn_msconv_hw_tiles(int n, int H, int W);       /* 64-pixel tiles of an n x H x W map, or MPNN_E_SHAPE */
int mpnn_msconv_fwd_hw(const mpnn_conv_fwd_args *args, int kh, int kw, int kvh, int kvw, void *stream);
int mpnn_msconv_dgrad_horz_hw(const mpnn_dgrad_horz_args *args, int kh, int kw, void *stream);
int mpnn_msconv_dgrad_vert_hw(const mpnn_dgrad_vert_args *args, int kvh, int kvw, void *stream);
int mpnn_msconv_wgrad_hw(const mpnn_wgrad_args *args, int kh, int kw, int kvh, int kvw, void *stream);

/* ---- the same four contractions with ANY channel counts (csrc/conv_gen_ch.hip over the same kernel template) ----------
 * The _gen and _hw forms keep their limits; these take the same records and arguments on the maps and filters of
 * mpnn_msconv_hw_check with 1 <= Cin, Cout <= 512 and Cv = 0 (no vertical operand) or 1 <= Cv <= 512
 * (mpnn_msconv_ch_check; the outputs of the two input-gradient forms are not held to multiples of 16 either).  Channel
 * tails are staged as zeros and stored nowhere.  The forward and input-gradient launches FIT the output tile to the
 * layer: 16 NT output channels per workgroup with NT = 1 (Cout <= 16), 2 (Cout <= 32) or 4, so a narrow layer does not pay
 * for a wide one; the order of the contraction of an output element does not depend on NT, and on a shape both families
 * accept _ch and _hw write the same bits.  mpnn_msconv_fwd_ch takes sample lists as mpnn_msconv_fwd_hw does.
 * mpnn_msconv_wgrad_ch loads g by scalars where Cout % 4 != 0.  Tiles per map: mpnn_msconv_hw_tiles. */
int mpnn_msconv_ch_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw);
int mpnn_msconv_fwd_ch(const mpnn_conv_fwd_args *args, int kh, int kw, int kvh, int kvw, void *stream);
int mpnn_msconv_dgrad_horz_ch(const mpnn_dgrad_horz_args *args, int kh, int kw, void *stream);
int mpnn_msconv_dgrad_vert_ch(const mpnn_dgrad_vert_args *args, int kvh, int kvw, void *stream);
int mpnn_msconv_wgrad_ch(const mpnn_wgrad_args *args, int kh, int kw, int kvh, int kvw, void *stream);

/* ---- single-scale Conv (scripts/lib/layer_types.py:55-74) ---------------------
 * y = b + conv2d_same(act(x), w) with supp x supp filters, supp = 3 (the direct 3x3 MFMA body of
 * the multiscale path) or supp = 1 (a GEMM over pixels, [n*H*W, Cin] x [Cin, Cout]).
 *   fwd  : w = the forward pack (supp 3, mpnn_pack_weights) or the HWIO tensor itself = [Cin][Cout] (supp 1)
 *   dgrad: dx = conv^T(g, w) [* (relu_src > 0): the producer's Rect]; w = the backward pack (supp 3) or
 *          [Cin][Cout] (supp 1); `scratch` (supp 3 with relu_src): 2*Cin doubles, overwritten
 *   wgrad: dw = act(x)^T (*) g, db = sum g.  supp 3: as mpnn_msconv_wgrad (n_split > 1: dw / db point into
 *          a slab, split_stride apart, then mpnn_slab_reduce); supp 1: ADDED into (caller-zeroed) dw / db.
 * Limits: supp 3 as the multiscale entry points; supp 1: Cin, Cout <= 256. */
typedef struct {
    mpnn_act a;  const float *w;  const float *bias;  float *out;
    int n, H, W, Cout;  int supp;
} mpnn_conv_nhwc_fwd_args;
int mpnn_conv_nhwc_fwd(const mpnn_conv_nhwc_fwd_args *args, void *stream);
typedef struct {
    const float *g;  int Cg;  const float *w;
    const float *relu_src;               /* [n,H,W,Cin] pre-activation of the producer, or NULL     */
    double *scratch;
    float *dx;
    int n, H, W, Cin;  int supp;
} mpnn_conv_nhwc_dgrad_args;
int mpnn_conv_nhwc_dgrad(const mpnn_conv_nhwc_dgrad_args *args, void *stream);
typedef struct {
    mpnn_act a;  const float *g;  float *dw;  float *db;
    long split_stride;  int n_split;
    int n, H, W, Cout;  int supp;
} mpnn_conv_nhwc_wgrad_args;
int mpnn_conv_nhwc_wgrad(const mpnn_conv_nhwc_wgrad_args *args, void *stream);

/* ---- exit head + router, first affine map ----------------------------------
 * y_k = flatten(act(a)) @ w_k + b_k [+ alpha_cpt * k_cpt[n] * w_k[K]] for up to
 * two weight sets sharing the input: the LogReg head's LinTrans and the
 * router's first LinTrans (layer_types.py:39-53 after Select(-1),
 * arch_and_hypers.py:45-49,66-70; the k_cpt column is net_types.py:149-160).
 *
 * The exit-path entry points are TABLE DRIVEN: `dev_table` is a DEVICE array
 * of `count` argument records (uploaded once per plan); one launch serves every
 * exit of the routing tree (the conv trunk does not depend on them). */
typedef struct {
    mpnn_act a;  int HW;                 /* input [n, HW, C] flattened to K=HW*C   */
    const float *w[2];  const float *b[2];  float *y[2];  int M[2];   /* M <= 16   */
    const float *k_cpt;  float alpha_cpt;  int extra_col[2];
    int n;
    /* Scratch of mpnn_lin_fwd_ks (both NULL: the record is never sliced; ignored by mpnn_lin_fwd):
     *   kpart: ceil(n/16) * MPNN_LIN_KSLICES * 512 floats, any contents
     *   kcnt : ceil(n/16) ints, ZERO before the first launch (left zero by every launch) */
    float *kpart;  int *kcnt;
} mpnn_lin_fwd_args;
#define MPNN_LIN_KSLICES 8
int mpnn_lin_fwd(const mpnn_lin_fwd_args *dev_table, int count, int n_max, void *stream);
/* The same map for SMALL batches (the training step: 8 row groups), K-sliced: a record with scratch and
 * K >= 512 is split over S = min(MPNN_LIN_KSLICES, K / 256) 256-thread workgroups per 16 rows; each leaves
 * its partial tile in kpart, and the LAST to arrive (ticket counter kcnt, which it resets) adds the S
 * partials in slice order -- the result does not depend on which workgroup that is (bit-identical from
 * launch to launch); it differs from mpnn_lin_fwd's in the last bits (another summation tree).
 * k_max >= HW*C of every record (sizes the grid). */
int mpnn_lin_fwd_ks(const mpnn_lin_fwd_args *dev_table, int count, int n_max, int k_max, void *stream);

typedef struct {
    mpnn_act a;  int HW;
    const float *w[2];  const float *dy[2];  int M[2];
    float *dw[2];  float *db[2];         /* written (sums over all n rows, fixed order) */
    float *dx;                           /* [n, HW*C] written, or NULL             */
    const float *k_cpt;  float alpha_cpt;  int extra_col[2];
    int n;
    /* Optional fusion of mpnn_bn_bwd_reduce for an exit whose block has no child (its dX is the
     * only gradient of that map): when dz_out is set (a.mode must be a BatchNorm mode), the kernel
     * also writes dz = dX where relu(bn(x)) > 0 else 0 to dz_out [n, HW*C] and adds
     * [sum dz, sum dz * xhat] per channel to red_out (fp64 [red_nslot][2C], caller-zeroed). */
    float *dz_out;  double *red_out;  int red_nslot;
    /* Scratch of mpnn_lin_bwd_rs (ignored by mpnn_lin_bwd):
     *   kpart: ceil((K+1)/64) * MPNN_LIN_RSPLIT * MPNN_LIN_RS_TILE floats, any contents
     *   kcnt : ceil((K+1)/64) ints, ZERO before the first launch (left zero by every launch) */
    float *kpart;  int *kcnt;
    /* ActivityError on the map (layer_types.py: ActivityError in front of the head's LinTrans): c_mod[s] = act_alpha *
     * sum_k act(x)[s][k]^2 over the K = HW*C features of the map -- not the k_cpt column -- weighted per sample by
     * act_w [n] (the leaf's w_cerr: dL/dc_mod = dL/dc_err).  Its gradient joins the input gradient where that is made:
     *   dX[s][k] += 2 act_alpha act_w[s] act(x)[s][k]
     * in dx and, through the same mask (a masked element has act(x) == 0), in dz_out / red_out.  act_alpha == 0 (a
     * zero-initialised record): neither field is read and every output has the bits it had without them.  Uniform
     * over a record; a table may mix records with and without. */
    float act_alpha;  const float *act_w;
} mpnn_lin_bwd_args;
#define MPNN_LIN_RSPLIT 8
#define MPNN_LIN_RS_TILE 2080            /* 64 features x 32 outputs of dW + 32 of db */
int mpnn_lin_bwd(const mpnn_lin_bwd_args *dev_table, int count, int n_max, int k_max,
                 void *stream);
/* The same for SMALL batches, ROW-SPLIT: min(MPNN_LIN_RSPLIT, ceil(n_max / 64)) workgroups share the rows
 * of a 64-feature block; their dW / db partial tiles meet in kpart, added in row-group order by the last
 * to arrive (ticket counter kcnt) -- bit-identical from launch to launch.  Every record needs scratch. */
int mpnn_lin_bwd_rs(const mpnn_lin_bwd_args *dev_table, int count, int n_max, int k_max,
                    void *stream);

/* ---- exit tail: everything after the first affine map ----------------------
 * Head: Softmax + CrossEntropyError (layer_types.py:81-84, 262-272).
 * Router: BN -> ReLU -> LinTrans(R) -> BN -> ReLU -> LinTrans(n_sinks)
 * (arch_and_hypers.py:47-49; BatchNorm over the batch, layer_types.py:219-239).
 * One workgroup per exit owns the whole batch (batch statistics need every
 * sample; the batch is held in LDS).  Limits: n <= 128 per launch, n_cls <= 16,
 * R <= 16, n_sinks <= 4 (MPNN_E_SHAPE beyond). */
typedef struct {
    /* head (z == NULL: no head at this exit) */
    const float *z;  const float *y;  int n_cls;  float eps_ce;
    float *c_err;  float *d_cor;                      /* [n] each               */
    /* router (h1 == NULL: node has no router) */
    const float *h1;  int R;  int n_sinks;            /* [n,R] pre-BN           */
    const float *g1, *b1;  float *m1, *v1;            /* BN1 gamma/beta/avgs    */
    const float *w2, *bias2;                          /* [R,R], [R]             */
    const float *g2, *b2;  float *m2, *v2;
    const float *w3, *bias3;                          /* [R,n_sinks], [n_sinks] */
    float *h2;  float *r;  int r_stride;              /* [n,R] pre-BN2, [n,r_stride] */
    float *bn_save;                                   /* [4*R] batch m1,rstd1,m2,rstd2 */
    float bn_eps, bn_decay;
    int mode;                                         /* MPNN_ACT_BN_BATCH / _MOVING */
    int n;
    /* Optional: accumulators of the launch that FOLLOWS (mpnn_route adds the TALR node statistics and the loss
     * sums with atomics): this record's head workgroup clears clear_f[0 .. n_clear_f) and clear_d[0 .. n_clear_d) --
     * for EVERY record of a table that carries them (a co-trained group's table: one set per net).
     * A training step then needs no clearing launch (the BatchNorm slot sums are cleared by their last reader,
     * mpnn_backward_finish / mpnn_bn_finalize). */
    float *clear_f;  int n_clear_f;  double *clear_d;  int n_clear_d;
    /* Width of the SECOND hidden layer (0: the same as R).  w2 is [R, R2], bias2 / g2 / b2 / m2 / v2 [R2], w3
     * [R2, n_sinks], h2 [n, R2], bn_save [2 R + 2 R2] = m1, rstd1, m2, rstd2.  The tuned kernels need R2 == R <= 16
     * and n_cls <= 16; the any-width forms below (mpnn_*_gen) take anything up to mpnn_exit_gen_check's limits. */
    int R2;
    /* Optional (K training steps in ONE hipGraph, lib/_plan.py:run_steps): this record's head workgroup copies the
     * MPNN_HYP_N schedule values hyp_src[0 .. MPNN_HYP_N) to hyp_dst -- the buffer mpnn_route and the optimizer of THIS
     * step read -- so that step j of the graph runs with the values staged in slot j, without a launch of its own. */
    const float *hyp_src;  float *hyp_dst;
    /* The SECOND router BatchNorm's own hyper-parameters (bn_eps / bn_decay above are the first one's: the two are
     * separate BatchNorm(d, eps) layers in the router chain, arch_and_hypers.py:47-49).  Always read: set both. */
    float bn_eps2, bn_decay2;
    /* The head's error layer, MPNN_LOSS_* (0, a zero-initialised record: Softmax + CrossEntropyError as above).  With
     * x = softmax(z) for MPNN_LOSS_SQ and x = z itself (no softmax) for MPNN_LOSS_SQ_LIN, SquaredError
     * (layer_types.py:255-260) is
     *   c_err[s] = sum_k (x[s][k] - y[s][k])^2,   d_cor[s] = [arg-max x[s] == arg-max y[s]]  (first index on ties),
     * y any float row (one-hot or real-valued targets); eps_ce is not read.  dL/dz with w = w_cerr[s]:
     *   MPNN_LOSS_SQ    : w x_k (g_k - sum_j g_j x_j),  g = 2 (x - y)
     *   MPNN_LOSS_SQ_LIN: 2 w (z_k - y_k)
     * Sums run in the order of the cross-entropy's; no atomics.  Uniform over a record; a table may mix the kinds. */
    int loss;
} mpnn_exit_tail_args;
#define MPNN_LOSS_CE 0
#define MPNN_LOSS_SQ 1
#define MPNN_LOSS_SQ_LIN 2
int mpnn_exit_tail_fwd(const mpnn_exit_tail_args *dev_table, int count, int n_max,
                       void *stream);

typedef struct {
    mpnn_exit_tail_args f;
    const float *w_cerr;                 /* [n] dL/dc_err                          */
    const float *dr;                     /* [n,r_stride] dL/dr                     */
    float *dz;                           /* [n,n_cls] dL/dz (head logits)          */
    float *dh1;                          /* [n,R] dL/dh1                           */
    float *dg1, *db1, *dw2, *dbias2, *dg2, *db2, *dw3, *dbias3;   /* written      */
    float *dh2;                          /* [n,R2] scratch (mpnn_exit_tail_bwd_gen: dL/dh2; the tuned kernel ignores it) */
    /* ActivityError on the head's logits and on its softmax outputs (layer_types.py: ActivityError behind the LinTrans,
     * behind the Softmax): c_mod[s] = act_z sum_k z[s][k]^2 + act_p sum_k p[s][k]^2, p = softmax(z).  Backward only (no
     * entry point reports c_mod), so the fields stand at the end of THIS record and mpnn_exit_tail_args is what it was: with
     * w = w_cerr[s], mpnn_exit_tail_bwd / _gen add to the loss's own dz
     *   2 w act_z z_k  +  2 w act_p p_k (p_k - sum_j p_j^2)        (the sum in class order, as the loss's dot product)
     * Both 0 (a zero-initialised record): dz has the bits it had without the fields.  act_p is not read with
     * MPNN_LOSS_SQ_LIN, a head without Softmax: the caller refuses that combination.  Any finite value, negative ones
     * included; uniform over a record. */
    float act_z, act_p;
} mpnn_exit_tail_bwd_args;
int mpnn_exit_tail_bwd(const mpnn_exit_tail_bwd_args *dev_table, int count, int n_max,
                       void *stream);

/* ---- one exit in evaluation mode, with routing ------------------------------
 * Head + router of one tree node in 'ev' mode (moving-average BatchNorm:
 * layer_types.py:237-238), any batch size, and the node's hard routing decision
 * pi_ev = one-hot(arg-max r) (net_types.py:127-129, first index on ties) turned
 * into per-child sample lists:
 *   z = flatten(act(a)) @ w_head + b_head -> softmax -> c_err, d_cor   (as mpnn_exit_tail_fwd)
 *   r = router MLP (as mpnn_lin_fwd + mpnn_exit_tail_fwd with MPNN_ACT_BN_MOVING)
 *   sample s (image idx[s]) is APPENDED to child_idx[i] (count child_cnt[i], atomically) for
 *   i = arg-max r, when sink i has a list (a child block); sinks without one (the exit's own
 *   classifier leaf) need none.
 * The sample list idx[0..*cnt) is the node's own (NULL: all n samples); c_err, d_cor and r are
 * indexed by IMAGE (r: [image][r_stride]), entries of samples that do not reach the node are
 * not touched (the caller clears them once per batch).  Table driven like the other exit-path
 * entry points; the grid is sized for n_max samples, counts are read on the device.
 * Limits (mpnn_exit_ev_check, host records): n_cls <= 16, R <= 16, n_sinks <= 4, C <= 128,
 * HW*C % 16 == 0. */
typedef struct {
    mpnn_act a;  int HW;                 /* the block's coarsest scale, pre-BN: [images, HW, C] */
    const float *w_head, *b_head;  int n_cls;         /* NULL: no classifier at this node */
    const float *y;  float eps_ce;  float *c_err, *d_cor;
    const float *w1, *b1;  int R;  int n_sinks;       /* NULL: no router */
    int extra_col;  const float *k_cpt;  float alpha_cpt;   /* dyn_k_cpt column (net_types.py:149-160) */
    const float *g1, *be1, *m1, *v1;  const float *w2, *bias2;
    const float *g2, *be2, *m2, *v2;  const float *w3, *bias3;
    float bn_eps;
    float *r;  int r_stride;
    const int *idx;  const int *cnt;  int n;           /* this node's sample list / capacity */
    int *child_idx[MPNN_MAX_SINKS];  int *child_cnt[MPNN_MAX_SINKS];
    int R2;                              /* width of the second hidden layer (0: R); see mpnn_exit_tail_args */
    float *z, *h1;                       /* scratch of mpnn_exit_ev_gen: [n, n_cls] head logits, [n, R] first router map
                                          * (rows by IMAGE; the tuned mpnn_exit_ev keeps both in LDS and ignores them) */
    float bn_eps2;                       /* epsilon of the SECOND router BatchNorm (bn_eps: the first one's); always read */
    /* The head's PREDICTION, by image (optional, both or neither): cls = arg-max class of the softmax -- the very index
     * d_cor compares with the label's, first index on ties -- and conf = its probability; p_cls (needs cls): the whole
     * softmax row [image][p_stride], p_stride >= n_cls.  Written for every sample of the node's list, nothing else.
     * LABEL-FREE head: y == NULL (then cls must be set): the cross-entropy and the label arg-max are skipped, c_err /
     * d_cor are not touched and may be NULL.  A labelled and a label-free launch on the same inputs satisfy
     * d_cor == (cls == arg-max y) exactly. */
    int *cls;  float *conf;
    float *p_cls;  int p_stride;
    /* The head's error layer, MPNN_LOSS_* as in mpnn_exit_tail_args (0: cross-entropy; mpnn_exit_ev_check refuses any
     * value but the three with MPNN_E_SHAPE -- the records are in device memory, so no launcher can: a caller of
     * mpnn_exit_ev_gen, which has no record check of its own, passes one of the three).  For the squared forms c_err / d_cor are SquaredError's on x = softmax(z)
     * (MPNN_LOSS_SQ) or x = z (MPNN_LOSS_SQ_LIN); cls = arg-max x, conf = x[cls], p_cls = the row x -- for
     * MPNN_LOSS_SQ_LIN these are RAW OUTPUTS, not probabilities (conf may be negative).  d_cor == (cls == arg-max y)
     * between a labelled and a label-free launch holds for every kind. */
    int loss;
} mpnn_exit_ev_args;
int mpnn_exit_ev(const mpnn_exit_ev_args *dev_table, int count, int n_max, void *stream);
int mpnn_exit_ev_check(const mpnn_exit_ev_args *host_record);

/* The routed evaluation's dense prefix made routed after the fact (csrc/exit_ev.hip): the exits of the blocks whose
 * convs run on every sample anyway (the first d0 tree depths) are evaluated densely in ONE mpnn_exit_ev launch; this
 * launch then walks every sample through the prefix's switches (arg-max of the router outputs, first index on ties:
 * net_types.py:127-129), clears r / c_err / d_cor of the prefix nodes the sample does not reach and appends it to the
 * sample list of the frontier block it arrives at.  Same results as the exit-by-exit routed pass, (d0 - 1) serial
 * launches fewer.  Records in topological order; parent[j] = record of the nearest switch above record j (-1: every
 * sample reaches it), parent_sink[j] = the sink of that switch that leads to j; n_sinks[j] = 0: no router at j;
 * c_err[j] / d_cor[j] NULL: no head at j.  front_*: the lists to fill.  host_rec is validated, dev_rec (the same
 * record in device memory) is what the kernel reads. */
#define MPNN_PREFIX_MAX 64
typedef struct {
    int n, count, n_front, pad_;
    int parent[MPNN_PREFIX_MAX], parent_sink[MPNN_PREFIX_MAX], n_sinks[MPNN_PREFIX_MAX], r_stride[MPNN_PREFIX_MAX];
    float *r[MPNN_PREFIX_MAX];
    float *c_err[MPNN_PREFIX_MAX];
    float *d_cor[MPNN_PREFIX_MAX];
    int front_parent[MPNN_PREFIX_MAX], front_sink[MPNN_PREFIX_MAX];
    int *front_idx[MPNN_PREFIX_MAX];
    int *front_cnt[MPNN_PREFIX_MAX];
} mpnn_ev_prefix_args;
int mpnn_ev_prefix_walk(const mpnn_ev_prefix_args *host_rec, const mpnn_ev_prefix_args *dev_rec, void *stream);

/* The answer of a label-free evaluation (csrc/ev_select.hip), after mpnn_route: in a dense pass and in the dense prefix
 * of a routed one the exits also run on samples that never reach them, so the sample's exit is chosen by p_ev.  One
 * thread per sample walks the leaves in order (leaf_node[l] = node id of leaf l); the FIRST leaf with p_ev == 1 is the
 * sample's (a statically forked net reaches several).  Written, by sample:
 *   leaf  that leaf's index (-1: none reached; then cls = -1, conf = 0, the probs row 0)
 *   cls, conf = leaf_cls / leaf_conf [leaf][leaf_stride] of that leaf (what mpnn_exit_ev stored there)
 *   probs [n][n_cls] (optional) = the leaf's row of leaf_p [leaf][leaf_stride][p_stride]
 *   ops   sum over ALL nodes with p_ev == 1 of node_ops[node] (block + router operations, exact integers)
 * The record goes to the kernel by value; it is validated on the host: 1 <= n_nodes <= MPNN_MAX_NODES,
 * 1 <= n_leaves <= n_nodes, leaf_stride >= n, probs needs leaf_p, n_cls >= 1 and p_stride >= n_cls.
 * CALLER'S OBLIGATION (leaf_node is a device table, the host cannot read it): 0 <= leaf_node[l] < n_nodes for every l. */
typedef struct {
    int n, n_nodes, n_leaves, n_cls;
    const float *p_ev;                   /* [n_nodes][n] (mpnn_route)              */
    const long long *node_ops;           /* [n_nodes]                              */
    const int *leaf_node;                /* [n_leaves], each in [0, n_nodes)       */
    const int *leaf_cls;  const float *leaf_conf;     /* [n_leaves][leaf_stride]   */
    const float *leaf_p;                 /* [n_leaves][leaf_stride][p_stride] or NULL */
    int leaf_stride, p_stride;
    int *leaf, *cls;  float *conf;       /* [n] written                            */
    float *probs;                        /* [n][n_cls] written, or NULL            */
    long long *ops;                      /* [n] written                            */
} mpnn_ev_select_args;
int mpnn_ev_select(const mpnn_ev_select_args *args, void *stream);

/* The confidence-threshold exit policy of a label-free evaluation (csrc/conf_gate.hip; Net.predict(exit_conf=)): leave at
 * the first exit whose head's confidence reaches a threshold.  The launch stands behind the mpnn_exit_ev / _gen launch
 * that stored `conf` and `r`, and in front of every reader of r (mpnn_ev_prefix_walk, mpnn_route, mpnn_ev_select; none of
 * them changes).  Table driven like mpnn_exit_ev: the records live in device memory, `count` records per launch, the grid
 * sized for n_max samples (one thread per sample, workgroups of 256), counts read on the device.  For every sample
 * s < min(*cnt, n) -- every s < n without cnt -- with img = idx ? idx[s] : s:
 *   d = exit_sink                                if conf[img] >= *tau  (plain fp32 comparison: a NaN on either side is "no")
 *   d = arg-max of r[img][i] over i != exit_sink otherwise             (first index on ties, the rule of mpnn_exit_ev and
 *                                                                       mpnn_ev_prefix_walk: the learnt router still chooses
 *                                                                       among the child blocks)
 *   r[img][i] = (i == d) ? 1 : 0  for i < n_sinks  (a finite one-hot row: every later reader reproduces d by its own plain
 *                                                   arg-max, and mpnn_route's softmax(r / tau) stays finite)
 *   img is appended to child_idx[d] where that list exists (wave ballot + popcount prefix, one atomicAdd per wave and
 *   sink; positions at or beyond n are not written, so a count that the caller did not clear cannot write past a list).
 * Rows of images that are not on the list are not touched; entries of a row at or beyond n_sinks neither.  Nothing depends
 * on a list's order.  tau is ONE float in device memory: a sweep rewrites a float, and a captured launch replays for any
 * value.  Asynchronous, allocates nothing, capturable.  count <= 0 or n_max <= 0: no launch, returns 0; a NULL table:
 * MPNN_E_ARG; more than 65 535 records: MPNN_E_SHAPE.
 * CALLER'S OBLIGATION (the records are in device memory): mpnn_conf_gate_check on every host record first -- MPNN_E_ARG:
 * NULL conf, tau or r, r_stride < n_sinks, idx without cnt, a child list with only one of its two pointers; MPNN_E_SHAPE:
 * n_sinks outside 2..MPNN_MAX_SINKS, exit_sink outside 0..n_sinks - 1 -- and n <= n_max, every idx[s] a valid image. */
typedef struct {
    const float *conf;                   /* [images] the head's confidence, by image (what mpnn_exit_ev / _gen stored) */
    const float *tau;                    /* ONE float in device memory: the threshold                                  */
    float *r;  int r_stride;             /* the switch's router outputs [image][r_stride], rewritten                    */
    int n_sinks, exit_sink;              /* 2..MPNN_MAX_SINKS; the sink that is this block's own classifier leaf        */
    const int *idx;  const int *cnt;  int n;      /* the node's sample list / capacity, as in mpnn_exit_ev_args         */
    int *child_idx[MPNN_MAX_SINKS];  int *child_cnt[MPNN_MAX_SINKS];   /* as in mpnn_exit_ev_args; NULL: no list        */
} mpnn_conf_gate_args;
int mpnn_conf_gate(const mpnn_conf_gate_args *dev_table, int count, int n_max, void *stream);
int mpnn_conf_gate_check(const mpnn_conf_gate_args *host_record);

/* The accuracy-versus-operations curve of confidence-threshold exits (csrc/exit_curve.hip; Net.exit_conf_curve): what every
 * image of a labelled batch does under each of n_points threshold rows, summed.  The launch stands behind a DENSE labelled
 * evaluation whose exit records carried labels and predictions together (mpnn_exit_ev_args: y, c_err, d_cor AND cls, conf),
 * so that every head's conf and d_cor and every switch's r are resident by image; nothing is evaluated again.
 *
 * The tree is a device table of one mpnn_curve_node per node.  Node 0 is the root and every child has a larger id than
 * its parent (the order of a depth-first walk).  For every image and point t the walk starts at node 0 and repeats:
 *   n_sinks == 0   the image exits at leaf_id
 *   n_sinks == 1   go to sink[0]
 *   switch_id >= 0 (a router; n_sinks >= 2), e = exit_sink, tau = taus[t][leaf_id of sink[e]]:
 *                  e >= 0 and tau not NaN: go to sink[e] if conf[that leaf][img] >= tau, else to the arg-max of
 *                  r[switch_id][img][i] over i != e;  otherwise (no e, or a NaN tau: the learnt policy) to the arg-max over
 *                  all i < n_sinks.  Comparison and arg-max are mpnn_conf_gate's: plain fp32, a NaN confidence is "no",
 *                  first index on ties.
 *   switch_id < 0, n_sinks == 2 (a static fork: sink[exit_sink] a leaf, the other sink not):
 *                  go to sink[exit_sink] if tau is not NaN and conf >= tau, else to the other sink.
 * Added, with integer atomics, into arrays the CALLER ZEROED (a second launch on another chunk keeps adding; the sums are
 * exact and independent of any order):
 *   correct[t]     images whose exit leaf has d_cor == 1
 *   ops[t]         sum over the images of node_ops[j] over the visited nodes j (the router of a gated switch counts: it
 *                  ran -- the `ops` of mpnn_ev_select behind mpnn_conf_gate)
 *   hist[t][leaf]  images that exit at `leaf`
 * taus: [n_points][n_leaves] with tau_per_leaf != 0, or the broadcast form [n_points] (tau_per_leaf == 0: one value per
 * point for every exit).  The record goes to the kernel by value; one thread per image, workgroups of 256, the points split
 * over the grid's y axis while the grid is small.  Asynchronous, allocates nothing, capturable.  n == 0:
 * no launch, returns 0.  The launcher refuses NULL pointers (MPNN_E_ARG; r may be NULL without switches), conf_stride or
 * dcor_stride below n (MPNN_E_ARG), and counts outside 1 <= n_nodes <= MPNN_MAX_NODES, 1 <= n_leaves <= n_nodes,
 * 0 <= n_switches <= MPNN_MAX_NODES / 2, n_points >= 1, n >= 0 (MPNN_E_SHAPE).
 * CALLER'S OBLIGATION (the tree is in device memory): mpnn_exit_curve_check(record, host copy of the tree) first.  On top of
 * the launcher's refusals it returns MPNN_E_SHAPE for a node with n_sinks outside 0..MPNN_MAX_SINKS, a sink id not above
 * the node's own or not below n_nodes, a leaf without a leaf_id of its own in 0..n_leaves - 1 (or an inner node with one),
 * a switch_id at or beyond n_switches or on a node with fewer than 2 sinks, an exit_sink outside its sinks or one that is
 * no leaf, and a static node with 2 or more sinks that is not "one leaf (its exit_sink) + one other node"; MPNN_E_ARG for
 * r_stride below a switch's n_sinks or r_switch_stride below n * r_stride.  A kernel that meets an id out of range all the
 * same ends that image's walk without counting it; it reads nothing out of bounds. */
typedef struct {
    int n_sinks;  int sink[MPNN_MAX_SINKS];      /* children (node ids)                                              */
    int switch_id;                               /* row of r, or -1: no router here                                   */
    int leaf_id;                                 /* of a leaf, else -1                                                */
    int exit_sink;                               /* the sink that is a classifier leaf directly below, or -1          */
} mpnn_curve_node;
typedef struct {
    int n, n_nodes, n_leaves, n_switches, n_points, tau_per_leaf;
    const mpnn_curve_node *tree;         /* [n_nodes], device memory                                                  */
    const long long *node_ops;           /* [n_nodes] (the table of mpnn_ev_select)                                   */
    const float *conf;  int conf_stride; /* [n_leaves][conf_stride >= n]                                              */
    const float *d_cor; int dcor_stride; /* [n_leaves][dcor_stride >= n]                                              */
    const float *r;  int r_stride;       /* [n_switches][r_switch_stride]: rows [image][r_stride], as mpnn_route reads */
    long long r_switch_stride;           /* floats between two switches (mpnn_route: n * max_sinks)                   */
    const float *taus;                   /* [n_points][n_leaves] or [n_points]                                        */
    long long *correct, *ops, *hist;     /* [n_points], [n_points], [n_points][n_leaves]: added to                    */
} mpnn_exit_curve_args;
int mpnn_exit_curve(const mpnn_exit_curve_args *args, void *stream);
int mpnn_exit_curve_check(const mpnn_exit_curve_args *host_record, const mpnn_curve_node *host_tree);

/* 8-bit pixels to the floats a net is trained on (csrc/decode.hip; the reference decodes on the host, once, in
 * scripts/prep-data:45-49 and :93-102): dst[i] = lut[src[i]] for 0 <= i < count, lut = 256 floats in DEVICE memory.  A
 * pure table lookup: bit-exact for any table, whatever NaNs or infinities it holds.  src may have any alignment, dst
 * and lut that of a float; 16-byte loads and float4 stores are used where one head of < 16 elements aligns both
 * pointers (src = dst modulo 4 elements), a scalar kernel otherwise.  Nothing outside [src, src + count) is read and
 * nothing outside [dst, dst + count) written.  count == 0: no launch, returns 0.  MPNN_E_ARG: a NULL pointer, count < 0,
 * dst or lut not 4-byte aligned. */
int mpnn_decode_u8(const unsigned char *src, float *dst, const float *lut, long count, void *stream);

/* MultiscaleLLN (csrc/lln.hip; reference layer_types.py:127-147): local luminance normalisation of every scale of the
 * input pyramid, in front of block 0.  With s = radius = ceil(2 sigma), g(u) = tap[u + s] and x_i[r][c] = x[r << i][c << i]
 * (ToPyramid's strided pick, layer_types.py:118-125; the pyramid is never materialised), for every scale i < n_scales
 * of h = H >> i by w = W >> i pixels:
 *   Y      = 0.2126 x_i[..][0] + 0.7152 x_i[..][1] + 0.0722 x_i[..][2]
 *   lum    = sum over u, v in [-s, s] of g(u) g(v) Y[r + u][c + v], zeros outside the map (:141-143; the reference's
 *            explicit pad and crop are redundant with SAME padding of radius s)
 *   dens   = the same sum over an image of ones (:144-146) = (sum of g(u), r + u inside) * (sum of g(v), c + v inside)
 *   out[i] = x_i / (lum / dens + eps), the one luminance channel broadcast over the three image channels (:147)
 * The taps are the caller's: g(u) = exp(-u^2 / (2 sigma^2)) computed in double and rounded to float; the constant
 * 1 / (2 pi sigma^2) of the reference's filter cancels in lum / dens.  There is no exp on the device.  Two 1-D passes
 * through LDS, fmaf in tap order, IEEE division: lum / dens + eps == 0 gives inf or nan as TensorFlow would, nothing
 * is clamped.  No atomics: a pixel's value depends on its own image alone (not on n, n_max, the record's place in
 * the table or the tiling), bit for bit.
 * One launch serves `count` records (one per net: a co-trained group concatenates them) of up to n_max samples each;
 * the geometry is the launch's, read on the host.  x is [n][H][W][3]; out[i] is [n][H >> i][W >> i][3] for i < n_scales
 * (the other entries are not read), and nothing outside out[i][0 .. n * h * w * 3) is written.  Asynchronous, allocates
 * nothing, capturable.  Refused before anything is launched -- MPNN_E_ARG: dev_table or geom NULL, count < 1,
 * n_max < 1; MPNN_E_SHAPE: radius outside 1..MPNN_LLN_MAX_RADIUS, n_scales outside 1..MPNN_LLN_MAX_SCALES, H or W
 * outside 1..256 or no multiple of 2^(n_scales - 1) (only then is every scale a strided pick).
 * CALLER'S OBLIGATION (the records are in device memory): x and out[i < n_scales] valid, 0 <= n <= n_max. */
#define MPNN_LLN_MAX_SCALES 8
#define MPNN_LLN_MAX_RADIUS 16
typedef struct {
    const float *x;                      /* [n][H][W][3]                           */
    float *out[MPNN_LLN_MAX_SCALES];     /* [n][H >> i][W >> i][3], i < n_scales   */
    int n;
    float eps;
} mpnn_lln_args;
typedef struct {
    int n_max, H, W, n_scales, radius;
    float tap[2 * MPNN_LLN_MAX_RADIUS + 1];          /* g(u), u = -radius .. radius, in tap[0 .. 2 radius] */
} mpnn_lln_geom;
int mpnn_lln_fwd(const mpnn_lln_args *dev_table, int count, const mpnn_lln_geom *geom, void *stream);

/* The labels of exits with a label space of their own (csrc/label_map.hip; reference layer_types.py:274-285,
 * SuperclassCrossEntropyError: y_sup = tf.matmul(y, w_cls)).  The exit kernels then read y_sup where they read y, with
 * the record's n_cls = n_sup: c_err, d_cor and the gradient are theirs.
 *   y_sup[r][s] = acc after  acc = 0.0f; for c in 0 .. n_cls - 1: acc = fmaf(y[r][c], w_cls[c][s], acc)
 * bit for bit: an element depends on neither the tiling, n, n_max nor the record's place in the table.  Nothing is skipped
 * or clamped (a zero label times an infinite weight is nan, as in a matmul).  No atomics.
 * One launch serves `count` records (one per distinct map of a net: a co-trained group concatenates its nets') of up to
 * n_max rows and n_sup_max columns each; the grid is sized from those two and n is read on the device.  Nothing outside
 * y_sup[0 .. n * n_sup) is written; a record with n == 0 writes nothing.  Asynchronous, allocates nothing, capturable.
 * Refused before anything is launched -- MPNN_E_ARG: dev_table NULL, count < 1, n_max < 1; MPNN_E_SHAPE: n_sup_max outside
 * 1..MPNN_LABEL_MAP_MAX_SUP (or more than 65 535 records).
 * CALLER'S OBLIGATION (the records are in device memory): mpnn_label_map_check on every host record first -- MPNN_E_ARG:
 * a NULL pointer (the record's or one of its three), n < 0; MPNN_E_SHAPE: n_cls outside 1..MPNN_LABEL_MAP_MAX_CLS, n_sup
 * outside 1..MPNN_LABEL_MAP_MAX_SUP -- and n <= n_max, n_sup <= n_sup_max (rows and columns beyond are not computed). */
#define MPNN_LABEL_MAP_MAX_CLS 1024
#define MPNN_LABEL_MAP_MAX_SUP 1024
typedef struct {
    const float *y;      /* [n][n_cls]                          */
    const float *w_cls;  /* [n_cls][n_sup] row-major, DEVICE    */
    float *y_sup;        /* [n][n_sup] written                  */
    int n, n_cls, n_sup;
} mpnn_label_map_args;
int mpnn_label_map(const mpnn_label_map_args *dev_table, int count, int n_max, int n_sup_max, void *stream);
int mpnn_label_map_check(const mpnn_label_map_args *host_record);

/* Dropout in front of an exit's classifier (csrc/dropout.hip; reference layer_types.py:212-217, tf.nn.dropout(x, λ) of
 * TF 0.12: x / keep_prob * floor(keep_prob + u)), training programs only.  The mask is drawn, never stored: element
 * (s, k) -- row s of the batch, feature k = (h W + w) C + c of the NHWC-flattened map -- is kept iff word k & 3 of
 *   Philox4x32-10(counter = (k >> 2, s, leaf, t), key = (seed_lo, seed_hi))  is  >= thresh,
 * thresh = ceil((1 - λ) 2^32) as the host computes it, t = *step read on the DEVICE (a captured graph replays with a new
 * step counter).  The mask depends on (seed, t, leaf, s, k) alone: not on the grid, n_max, k_max, the record's place in
 * the table or the other records.
 *   mpnn_dropout_fwd:  xd[s][k] = keep ? act(x[s][k]) * inv_keep : +0.0f -- act as mpnn_bn_relu_fwd materialises it
 *                      (a.mode MPNN_ACT_BN_BATCH: the same coefficients, the same expression) or the identity
 *                      (MPNN_ACT_IDENTITY); with thresh == 0 and inv_keep == 1 bit for bit mpnn_bn_relu_fwd's output;
 *   mpnn_dropout_bwd:  dx[s][k] = (accumulate ? dx[s][k] : +0.0f) + (keep ? dxd[s][k] * inv_keep : 0) -- the mask drawn
 *                      again from the counter; a dropped element of an accumulating dx keeps its bits.
 * One launch serves `count` records of up to n_max rows and k_max features each (both only size the grid: every record
 * is walked to its own n and HW * a.C by a grid-stride loop).  16-byte accesses where HW * a.C % 4 == 0.  No atomics, no
 * LDS.  Asynchronous, allocates nothing, capturable.  Refused before anything is launched -- MPNN_E_ARG: dev_table
 * NULL, count, n_max or k_max < 1; MPNN_E_SHAPE: more than 65 535 records, n_max * k_max >= 2^30.
 * CALLER'S OBLIGATION (the records are in device memory): mpnn_dropout_check on every host record first -- MPNN_E_ARG:
 * a NULL record or step, n < 1, HW < 1, inv_keep not finite or below 1, accumulate not 0 or 1, neither a forward half (a.x
 * with xd) nor a backward half (dxd with dx), a.mode other than the two above or a batch-statistics record without its
 * sums and coefficients; MPNN_E_SHAPE: a.shift != 0, a.C outside 1..512, n * HW * a.C >= 2^30. */
typedef struct {
    mpnn_act a;  int HW;  int n;          /* the block's coarsest map, as mpnn_lin_fwd_args sees it (shift == 0) */
    unsigned seed_lo, seed_hi, leaf, thresh;  float inv_keep;
    const unsigned *step;                 /* DEVICE: the step counter t this launch draws with */
    float *xd;                            /* fwd: [n, HW*C] written */
    const float *dxd;  float *dx;  int accumulate;   /* bwd: [n, HW*C] read / written (read as well with accumulate) */
} mpnn_dropout_args;
int mpnn_dropout_fwd(const mpnn_dropout_args *dev_table, int count, int n_max, int k_max, void *stream);
int mpnn_dropout_bwd(const mpnn_dropout_args *dev_table, int count, int n_max, int k_max, void *stream);
int mpnn_dropout_check(const mpnn_dropout_args *host_record);
/* The generator of the two launches as a host function: out[4] = Philox4x32-10(counter[4], key[2]). */
int mpnn_philox4x32_10(const unsigned *counter, const unsigned *key, unsigned *out);

/* ---- any-WIDTH forms of the exit path (csrc/exit_gen.hip) -------------------
 * LinTrans takes any n_chan (layer_types.py:39-53) and the router MLP any hidden width (arch_and_hypers.py:14,45-49);
 * the tuned kernels above hold n_cls <= 16 and two EQUAL hidden layers of <= 16 units.  The same argument records go
 * to these kernels (any batch size; the backward tail needs the dh2 scratch map) for n_cls <= 1024, R, R2 <= 256,
 * C <= 256, HW * C <= 65536.  mpnn_exit_gen_check holds those limits; the caller runs it on EVERY record before the
 * record's table is launched: it also keeps the widest column-tile count seen in the process, which sizes the grid of
 * mpnn_lin_fwd_gen and mpnn_exit_ev_gen (the records live in device memory, the launchers cannot read them).
 *   mpnn_lin_fwd_gen        == mpnn_lin_fwd
 *   mpnn_lin_bwd_gen        == mpnn_lin_bwd with dx (or NULL); the dz_out fusion is not offered: the caller runs
 *                              mpnn_bn_bwd_reduce on dx instead
 *   mpnn_exit_tail_fwd_gen  == mpnn_exit_tail_fwd (batch statistics or, with mode MPNN_ACT_BN_MOVING, the averages)
 *   mpnn_exit_tail_bwd_gen  == mpnn_exit_tail_bwd
 *   mpnn_exit_ev_gen        == mpnn_exit_ev (children's lists: one atomic reservation per workgroup and sink) */
int mpnn_lin_fwd_gen(const mpnn_lin_fwd_args *dev_table, int count, int n_max, void *stream);
int mpnn_lin_bwd_gen(const mpnn_lin_bwd_args *dev_table, int count, int n_max, int k_max, void *stream);
int mpnn_exit_tail_fwd_gen(const mpnn_exit_tail_args *dev_table, int count, int n_max, void *stream);
int mpnn_exit_tail_bwd_gen(const mpnn_exit_tail_bwd_args *dev_table, int count, int n_max, void *stream);
int mpnn_exit_ev_gen(const mpnn_exit_ev_args *dev_table, int count, int n_max, void *stream);
int mpnn_exit_gen_check(int C, int K, int n_cls, int R, int R2, int n_sinks);

/* ---- the router: routing probabilities, costs and their gradients ----------
 * Replaces ActorNet._route/_route_sinks_dyn + cost assembly
 * (net_types.py:108-131,165-177), CriticNet's (net_types.py:193-243,273-280)
 * and SRNet's loss (net_types.py:93-95).  One thread per sample walks the
 * routing tree given as a device table `nodes` (8 ints per node, DFS preorder:
 * parent, sink_index, n_sinks, switch_id (-1: none), leaf_id (-1: none),
 * n_leaves, depth (root = 0), rank of the node when all nodes are sorted by
 * (depth, preorder index) -- the kernel walks the tree one LEVEL at a time), `sw_children` [n_switches][max_sinks] node
 * ids, and `node_ops` (n_ops + router.n_ops per node).
 *   outputs: p_tr, p_ev [n_nodes][n]; w_cerr [n_leaves][n] = dL/dc_err;
 *            dr [n_switches][n][max_sinks] = dL/dr; node_stat [n_nodes][2] =
 *            sum p_tr, sum p_tr^2 (TALR, net_types.py:25-27), accumulated;
 *            loss[4] accumulated sums: c_err, c_cpt, c_dec|c_cre, sample count.
 * hyp = device floats indexed by MPNN_HYP_*. */
#define MPNN_NET_SR     0
#define MPNN_NET_ACTOR  1
#define MPNN_NET_CRITIC 2
#define MPNN_HYP_LR   0
#define MPNN_HYP_MU   1
#define MPNN_HYP_TAU  2
#define MPNN_HYP_EPS  3
#define MPNN_HYP_KCPT 4
#define MPNN_HYP_KDEC 5
#define MPNN_HYP_KCRE 6
#define MPNN_HYP_ARTR 7
#define MPNN_HYP_N    16
typedef struct {
    int net_type;  int n_nodes, n_leaves, n_switches, max_sinks;
    int optimistic, use_cls_err, want_grad;
    const int *nodes;  const int *sw_children;  const float *node_ops;
    const float *hyp;
    const float *k_cpt_vec;              /* [n] per-sample k_cpt or NULL           */
    const float *r;                      /* [n_switches][n][max_sinks]             */
    const float *c_err;  const float *d_cor;          /* [n_leaves][n]             */
    float *p_tr, *p_ev;                  /* [n_nodes][n]                           */
    float *w_cerr;                       /* [n_leaves][n]                          */
    float *dr;                           /* [n_switches][n][max_sinks]             */
    float *node_stat;                    /* [n_nodes][2] accumulated               */
    double *loss;                        /* [4] accumulated                        */
    int n;  int n_total;                 /* n_total: samples the mean is over      */
    /* node_stat with MORE THAN TWO workgroups (two fp32 atomics onto a cleared sum commute; three do not): every
     * workgroup stores its partial sums in stat_part (floats [workgroups][n_nodes][2], then doubles [workgroups][4] for
     * the loss sums; room for ceil(n / 16) workgroups: ceil(n / 16) * (2 * n_nodes + 8) floats, 8-byte aligned), the last
     * one to finish (stat_ticket: one int, zero between launches) adds them up in workgroup order -- the TALR statistics,
     * and with them the whole step, are the same bits from run to run.  NULL: atomics (evaluation; small batches). */
    float *stat_part;  int *stat_ticket;
} mpnn_route_args;
int mpnn_route(const mpnn_route_args *args, void *stream);
/* mpnn_route of `count` co-trained nets with the same tree shape and batch size as one launch (host_table sizes it,
 * dev_table = the same records in device memory). */
int mpnn_route_multi(const mpnn_route_args *host_table, const mpnn_route_args *dev_table, int count, void *stream);

/* On-device compaction of the 'ev' sub-batch that reaches a node: indices of
 * samples with p_ev > 0, in order (wave64 ballot + prefix sum), and their
 * count -- consumed by later launches without a host sync. */
int mpnn_compact_by_branch(const float *p_ev, int n, int *idx_out, int *count_out,
                           void *stream);

/* ---- BatchNorm epilogue of a training step ----------------------------------
 * Moving averages (layer_types.py:233-234) from the forward sums and
 * dgamma / dbeta from the backward reductions, for every conv BatchNorm in one
 * launch.  table: 8 ints per BN: sum_off (doubles; same offset in `reds`; each
 * a [SLOTS][2*C] block of which table[7] slots are in use),
 * mavg_off, vavg_off (floats in `state`), C, pixels per image, gamma_goff,
 * beta_goff (floats in `grads`), nslot.  gamma_goff = -1 marks a BatchNorm whose output
 * nobody consumes: no gradients and -- as in the reference, whose tf.assign of the
 * averages only executes when the output is needed -- no moving-average update.
 * sums_keep (NULL: off): this launch is the LAST reader of the step's slot sums; with sums_keep set it copies
 * the forward sums there (same layout: the step's batch statistics stay inspectable) and leaves `sums` and
 * `reds` CLEARED, so that the next training step needs no clearing launch. */
int mpnn_bn_finalize(double *sums, double *reds, float *state, float *grads,
                     const int *table, int n_bn, float decay, int n_img, double *sums_keep, void *stream);

/* ---- TALR + L2 + momentum (net_types.py:24-37, tf.train.MomentumOptimizer) --
 * For every trainable element: g = grad + 2*k_l2*pbar_node*(w - w_eq)  (w_eq: the identity part of a
 * `res` layer, layer_types.py:46,52,65-72: seg[5] = offset of the tensor's w_eq in `w_eq`, or -1 = zero);
 * g *= s_node (* alpha_rtr for router params), s_node = 1/sqrt(mean p_tr^2);
 * accum = mu*accum + g; w -= lr*accum.  seg table: MPNN_SEG_INTS ints per work item
 * (offset, count, node, is_router, l2_bits (float as int), w_eq offset or -1,
 *  then for 3x3 conv weights: offset of the tensor in `params`, Cin, Cout, forward-pack offset,
 *  backward-pack offset (-1: none) in `packs`; Cin = 0 for every other tensor; reserved).
 * packs != NULL: every updated conv weight is also written to its slots of the weight packs
 * (mpnn_pack_weights' layout), so the next step needs no packing launch.
 * grad_scale multiplies the raw gradients (1/world_size after an all-reduce
 * sum); inv_n = 1 / (samples behind node_stat). */
int mpnn_talr_momentum_step(float *params, float *accum, const float *grads,
                            const int *seg, int n_seg, const float *node_stat,
                            const float *hyp, int talr, float inv_n, float grad_scale,
                            const float *w_eq, float *packs, void *stream);
#define MPNN_SEG_INTS 12

/* ---- training-batch assembly (scripts/lib/data.py:10-34) -------------------
 * x_out[i] = rand_shift(rand_flip(x_src[j_i])), y_out[i] = y_src[j_i] for a dataset resident in
 * device memory ([N,H,W,C] and [N,n_cls] fp32, C <= 4).  `draw` is a device array [n][4] of ints
 * (j, flip, du, dv) drawn on the host with the reference's call sequence on numpy's global
 * stream (randint(0, N); rand() < 0.5 for symmetric classes; randint(-r, r + 1, 2)).
 * out[u][v] = a[u + du][v + dv] where that exists, else the image's per-channel mean (computed
 * in fp64); flip mirrors v.  y_src / y_out may be NULL. */
int mpnn_augment_batch(const float *x_src, const float *y_src, const int *draw,
                       float *x_out, float *y_out, int n, int H, int W, int C, int n_cls,
                       void *stream);
/* The batches of `count` consumers (co-trained nets) from one dataset in ONE launch: consumer r's record buffer and
 * destinations in dev_table[r] (device memory), n images each. */
typedef struct { const int *draw;  float *x_out;  float *y_out; } mpnn_augment_dst;
int mpnn_augment_batch_multi(const float *x_src, const float *y_src, const mpnn_augment_dst *dev_table, int count,
                             int n, int H, int W, int C, int n_cls, void *stream);

/* mpnn_slab_reduce and mpnn_bn_finalize in ONE launch (same arguments and semantics; the two are
 * independent of each other and both end the backward pass). */
int mpnn_backward_finish(const float *slabs, float *grads, const int *slab_table, int n_items,
                         double *sums, double *reds, float *state, const int *bn_table,
                         int n_bn, float decay, int n_img, double *sums_keep, void *stream);

/* mpnn_backward_finish AND mpnn_talr_momentum_step in ONE launch (single-process training: nothing sits between the
 * gradients and their use; under data parallelism the all-reduce does, and the two stay separate).  Every slab item's
 * workgroup applies the update to the elements it has just reduced (item_seg: one MPNN_SEG_INTS row per slab item, same
 * fields as the optimizer's work items, count <= MPNN_SLAB_ITEM), every BatchNorm's workgroup to its gamma / beta
 * (bn_opt: 4 ints per record of bn_table: tree node, l2 bits of gamma, l2 bits of beta, reserved), and n_plain further
 * workgroups run the optimizer work items plain_seg whose gradients are already final in `grads`.  Element for element
 * the arithmetic of the two launches it replaces. */
int mpnn_backward_finish_opt(const float *slabs, const int *slab_table, int n_items, const int *item_seg,
                             double *sums, double *reds, float *state, const int *bn_table, int n_bn,
                             const int *bn_opt, float decay, int n_img, double *sums_keep,
                             float *params, float *accum, float *grads, const float *node_stat,
                             const float *hyp, int talr, float inv_n, float grad_scale, const float *w_eq,
                             float *packs, const int *plain_seg, int n_plain, void *stream);

/* mpnn_backward_finish_opt of `count` co-trained nets as one launch: one record per net (the arguments of the single-net
 * call), in host memory to size the launch and in device memory for the kernel. */
typedef struct {
    const float *slabs;  const int *slab_table;  int n_items;  const int *item_seg;
    double *sums, *reds;  float *state;  const int *bn_table;  int n_bn;  const int *bn_opt;  int n_img;  double *sums_keep;
    float *params, *accum, *grads;  const float *node_stat, *hyp;  int talr;  float inv_n, grad_scale;
    const float *w_eq;  float *packs;  const int *plain_seg;  int n_plain;
} mpnn_finish_net;
int mpnn_backward_finish_opt_multi(const mpnn_finish_net *host_table, const mpnn_finish_net *dev_table, int count,
                                   float decay, void *stream);

/* Workgroups of the mpnn_msconv_bwd_scale kernel (the variant for this shape, with or without a
 * dgrad-vert body) for an H x W x Cout scale that are resident on the
 * device at once (occupancy x compute units; needs a GPU).  The caller gives the weight-gradient
 * split (n_split x channel chunks x cout groups workgroups) about half of them, so that the dgrad
 * and wgrad workgroups of the launch all start together.  dgrad_items = 64-pixel tiles x 16-channel rows of the
 * two input-gradient bodies (the most workgroups they can use; 64-channel layers whose input gradients cannot fill
 * one workgroup per CU are limited to two workgroups per CU).  Negative = MPNN_E_*. */
int mpnn_msconv_bwd_scale_slots(int H, int W, int Cout, int has_dgrad, int has_vert, int dgrad_items);

/* Profiling aid (no reference counterpart).  Installs (or, with NULL, removes) a device buffer of
 * MPNN_TRACE_SLOTS (12) uint64 per workgroup of the largest grid to be traced: thread 0 of every
 * workgroup of the conv / dgrad / wgrad kernels stamps the 100 MHz device clock at its phase
 * boundaries (entry, tables ready, first tile staged, first unit done, loop done, exit; slot 6 = body
 * kind, slot 7 = units; slots 8-10: first unit's MFMAs done, next unit staged, epilogue done).  tools/trace_phases.py prints the timeline.  Synchronises the device. */
int mpnn_debug_set_trace(unsigned long long *buf);

/* ---- MaxPool / GlobalMaxPool of the single-scale layer family (scripts/lib/layer_types.py:86-100; no shipped spec
 * uses them) on NHWC fp32 maps.  MaxPool: tf.nn.max_pool(..., 'SAME') with window `win` and step `step` -- the
 * reference passes its hypers as (strides, k_shape), i.e. window = hypers.stride, step = hypers.supp (:90-94);
 * out = ceil(H / step) x ceil(W / step); backward: each window's gradient goes to its FIRST maximum in row-major order,
 * overlapping windows add (a gather per input element: no atomics).  global != 0: tf.reduce_max over H x W ->
 * y [n][C], cnt [n][C] = number of maxima (forward output), backward dx = [x == y] * dy / cnt.  The caller pools
 * PRE-activation maps (max-pool commutes with the ReLU its consumers apply on load). */
int mpnn_maxpool_fwd(const float *x, float *y, float *cnt, int n, int H, int W, int C, int win, int step,
                     int global, void *stream);
int mpnn_maxpool_bwd(const float *x, const float *y, const float *cnt, const float *dy, float *dx, int n, int H,
                     int W, int C, int win, int step, int global, void *stream);

/* Host function (no device work, no stream): the augmentation draws of scripts/lib/data.py:24-34 -- per sample
 * randint(0, n_src); rand() < 0.5 if sym[j] (sym == NULL: every class is symmetric); randint(-r_shift, r_shift + 1, 2)
 * -- replayed over consecutive 32-bit outputs of numpy's legacy MT19937 stream with numpy's own bounded-integer and
 * random_sample algorithms.  draw: [n][4] = (j, flip, du, dv), the record mpnn_augment_batch reads.  RESUMABLE so that
 * the stream is never over-drawn: `state` (4 longs; [0..2] zero to start a batch, [3] = 1 if the caller vouches that
 * every sym[] entry is set, which tightens the lower bound) carries the position inside the batch; a
 * call consumes ALL n_raw words it is given and returns the minimum number of words the remaining draws need (0: the
 * batch is complete); the caller hands over exactly that many next time (first call: n_raw = 0).  MPNN_E_ARG for bad
 * arguments or more words than the minimum. */
long mpnn_draw_augmentation(const unsigned int *raw, long n_raw, int n, long n_src, const unsigned char *sym,
                            int r_shift, int *draw, long *state);

/* The same draws from a PRIVATE MT19937 state in numpy's legacy layout (key[624], *pos in 0..624: the fields of
 * numpy.random.RandomState.get_state()), the generator stepped here: `batches` batches of n samples per call, written
 * to draw as [batches][n][4] -- or, with draw == NULL, only skipped.  A net trained beside others (lib/_co.py, train-nets
 * --shard-nets) gets the batches of the reference's serial experiment loop (scripts/train-nets:159-164: ONE global
 * stream, net after net) by advancing the experiment's stream over the iterations of the nets in front of it.  key / pos
 * are updated in place.  0, or MPNN_E_ARG. */
long mpnn_draw_augmentation_mt(unsigned int *key, int *pos, long batches, int n, long n_src, const unsigned char *sym,
                               int r_shift, int *draw);

/* Data parallelism (new here: the reference is single-process, scripts/train-nets:159-164).  Compute units every
 * persistent grid launched AFTER this call leaves free (0: none, the default): RCCL's all-reduce kernels run beside
 * the backward launches of the bucket sections (lib/_plan.py), and a grid fitted to every resident workgroup slot
 * then holds workgroups that only start when others exit.  Affects the grids the launchers choose and the slot counts
 * mpnn_msconv_bwd_scale_slots / mpnn_msconv_bwd_level_slots report.  Host-side state, not stream-ordered.  Returns the
 * previous value; a negative argument only queries. */
int mpnn_set_reserved_cus(int cus);

/* Measurement aids (no reference counterpart).  mpnn_debug_spin: `wgs` workgroups of `threads` threads that do nothing
 * but hold their slots for `us` microseconds (100 MHz device clock) -- a stand-in for a co-running collective kernel
 * in tools/dp_corunner_probe.py.  mpnn_debug_noop: one wave that returns at once -- the launch floor in bench.py. */
int mpnn_debug_spin(int wgs, int threads, float us, void *stream);
int mpnn_debug_noop(void *stream);

const char *mpnn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPNN_HIP_H */
