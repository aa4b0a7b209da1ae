// DRUNet's scale changes in the half-precision ("f16") arithmetic of kernels_conv_f16.hip: pix2x2_body.h's kernel with
// halves in and out -- four 16-byte loads per thread and chunk instead of eight, nothing to split (an added x2: the sum is formed in
// float32 and rounded to half once, as the operand), 8 KiB blocks of weights, 16 v_mfma_f32_16x16x32_f16 per wave and chunk instead of 48,
// results rounded once on store (or left float32: y_f32).
#include "pix2x2_body.h"

namespace pnp {

template <bool UP, bool X2>
__global__ __launch_bounds__(CV_THREADS, 2) void k_pix2x2_f16(Pix2Args a, int nitems) { pix2x2_body<Pix2F16, UP, X2>(a, nitems); }

__global__ __launch_bounds__(256) void k_pix2_pack_w_f16(const float* w, _Float16* wfrag, int C, int up) { pix2_pack_w_body<false>(w, wfrag, C, up); }

hipError_t launch_pix2x2_f16(hipStream_t s, const void* x, const void* x2, const void* w, void* y, int n, int C, int H, int W, int up, int y_f32) {
    static void (*const kern[2][2])(Pix2Args, int) = {{k_pix2x2_f16<false, false>, k_pix2x2_f16<false, true>}, {k_pix2x2_f16<true, false>, k_pix2x2_f16<true, true>}};
    return launch_pix2(s, kern, x, x2, w, y, n, C, H, W, up, y_f32);
}

hipError_t launch_pix2_pack_w_f16(hipStream_t s, const float* w, void* wfrag, int C, int up) {
    return launch_pix2_pack(s, k_pix2_pack_w_f16, w, wfrag, C, up);
}

}  // namespace pnp
