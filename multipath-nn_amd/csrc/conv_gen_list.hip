// mpnn_msconv_fwd_gen / mpnn_msconv_fwd_hw on a sample list (mpnn_conv_fwd_args.idx / cnt: routed evaluation): the IDX
// instantiation of the general forward conv kernel (conv_gen_k.h), launched by gen_fwd of conv_gen.hip.
#include "conv_gen_k.h"

int gen_fwd_list_launch(const GenP &p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((gen_conv_k<GEN_FWD, true>), grid, dim3(256), 0, stream, p);
    MPNN_LAUNCH_CHECK();
    return 0;
}
