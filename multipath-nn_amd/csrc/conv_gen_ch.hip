// The any-channel family of the general multiscale conv entry points: mpnn_msconv_fwd_ch / _dgrad_horz_ch /
// _dgrad_vert_ch / _wgrad_ch take the records of the _hw forms on the maps and filters of mpnn_msconv_hw_check with ANY
// channel count from 1 to 512 on every operand (mpnn_msconv_ch_check), as the reference's MultiscaleConvMax takes any
// n_chan (scripts/lib/layer_types.py:149-194).  The host side is conv_gen.hip's (one set of record checks for the three
// families); this translation unit holds what only this family launches:
//
//   * the forward / input-gradient kernel (conv_gen_k.h) with FITTED output tiles -- NT = 1 or 2 16-channel tiles per wave
//     for layers of <= 16 / <= 32 output channels, grid.y = ceil(Cout / (16 NT)) -- so that a narrow layer does not stage
//     and multiply three or two tiles of masked zeros; wider layers run conv_gen.hip's NT = 4 kernels.  The contraction
//     order of an output element does not depend on NT: on a shape the _hw forms take, the bits are theirs.
//   * the forward kernel of both widths on a sample list (routed evaluation);
//   * the weight-gradient kernel with scalar loads of the g tile, for Cout % 4 != 0.
#include "conv_gen_k.h"

template <int NT>
static int ch_launch(int epi, bool list, const GenP &p, dim3 grid, hipStream_t stream) {
    switch (epi) {
    case GEN_FWD:
        if (list) hipLaunchKernelGGL((gen_conv_k<GEN_FWD, true, NT>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((gen_conv_k<GEN_FWD, false, NT>), grid, dim3(256), 0, stream, p);
        break;
    case GEN_DGH_BN:  hipLaunchKernelGGL((gen_conv_k<GEN_DGH_BN, false, NT>), grid, dim3(256), 0, stream, p);  break;
    case GEN_DGH_RAW: hipLaunchKernelGGL((gen_conv_k<GEN_DGH_RAW, false, NT>), grid, dim3(256), 0, stream, p);  break;
    case GEN_DGV:     hipLaunchKernelGGL((gen_conv_k<GEN_DGV, false, NT>), grid, dim3(256), 0, stream, p);  break;
    default: return MPNN_E_ARG;
    }
    MPNN_LAUNCH_CHECK();
    return 0;
}

int gen_ch_launch(int epi, bool list, int nt, const GenP &p, dim3 grid, hipStream_t stream) {
    if (nt == 1) return ch_launch<1>(epi, list, p, grid, stream);
    if (nt == 2) return ch_launch<2>(epi, list, p, grid, stream);
    return MPNN_E_ARG;
}

int gen_ch_wgrad_launch(const GenWP &p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL(gen_wgrad_k<true>, grid, dim3(256), 0, stream, p);
    MPNN_LAUNCH_CHECK();
    return 0;
}

// Maps and filters as mpnn_msconv_hw_check; any Cin, Cout from 1 to 512, Cv = 0 (no vertical operand) or 1 to 512.
int gen_ch_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw) {
    if (H < 1 || H > 256 || W < 1 || W > 256) return MPNN_E_SHAPE;
    if (Cin < 1 || Cin > GEN_CMAX || Cout < 1 || Cout > GEN_CMAX || Cv < 0 || Cv > GEN_CMAX) return MPNN_E_SHAPE;
    if (kh < 1 || kh > GEN_KMAX || kw < 1 || kw > GEN_KMAX) return MPNN_E_SHAPE;
    if (Cv != 0 && (kvh < 1 || kvh > GEN_KMAX || kvw < 1 || kvw > GEN_KMAX)) return MPNN_E_SHAPE;
    return 0;
}

extern "C" int mpnn_msconv_ch_check(int H, int W, int Cin, int Cv, int Cout, int kh, int kw, int kvh, int kvw) {
    return gen_ch_check(H, W, Cin, Cv, Cout, kh, kw, kvh, kvw);
}
extern "C" int mpnn_msconv_fwd_ch(const mpnn_conv_fwd_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    return gen_fwd(GEN_FAM_CH, a, kh, kw, kvh, kvw, stream);
}
extern "C" int mpnn_msconv_dgrad_horz_ch(const mpnn_dgrad_horz_args *a, int kh, int kw, void *stream) {
    return gen_dgrad_horz(GEN_FAM_CH, a, kh, kw, stream);
}
extern "C" int mpnn_msconv_dgrad_vert_ch(const mpnn_dgrad_vert_args *a, int kvh, int kvw, void *stream) {
    return gen_dgrad_vert(GEN_FAM_CH, a, kvh, kvw, stream);
}
extern "C" int mpnn_msconv_wgrad_ch(const mpnn_wgrad_args *a, int kh, int kw, int kvh, int kvw, void *stream) {
    return gen_wgrad(GEN_FAM_CH, a, kh, kw, kvh, kvw, stream);
}
