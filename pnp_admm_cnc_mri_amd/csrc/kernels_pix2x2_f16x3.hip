// DRUNet's scale changes in the split-half ("f16x3") arithmetic of kernels_conv_f16x3.hip: pix2x2_body.h's kernel with
// float32 in and out -- eight 16-byte loads per thread and chunk, each value split into a half pair on the way into LDS (pixel =
// [64 hi][64 lo] + 16 bytes, the conv kernel's layout), the chunk's weights pre-split in 16 KiB blocks, 48 v_mfma_f32_16x16x32_f16 per wave
// and chunk (2 K steps x 2 M tiles x 4 N tiles x 3 products).
#include "pix2x2_body.h"

namespace pnp {

template <bool UP, bool X2>
__global__ __launch_bounds__(CV_THREADS, 2) void k_pix2x2_h3(Pix2Args a, int nitems) { pix2x2_body<Pix2H3, UP, X2>(a, nitems); }

__global__ __launch_bounds__(256) void k_pix2_pack_w(const float* w, _Float16* wfrag, int C, int up) { pix2_pack_w_body<true>(w, wfrag, C, up); }

hipError_t launch_pix2x2_f16x3(hipStream_t s, const float* x, const float* x2, const float* w, float* y, int n, int C, int H, int W, int up) {
    static void (*const kern[2][2])(Pix2Args, int) = {{k_pix2x2_h3<false, false>, k_pix2x2_h3<false, true>}, {k_pix2x2_h3<true, false>, k_pix2x2_h3<true, true>}};
    return launch_pix2(s, kern, x, x2, w, y, n, C, H, W, up, 1);
}

hipError_t launch_pix2_pack_w_f16x3(hipStream_t s, const float* w, float* wfrag, int C, int up) {
    return launch_pix2_pack(s, k_pix2_pack_w, w, wfrag, C, up);
}

}  // namespace pnp
