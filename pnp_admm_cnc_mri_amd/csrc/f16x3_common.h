// Shared by the split-half ("f16x3") matrix-core kernels: kernels_conv_f16x3.hip (conv3x3 C -> C) and kernels_pix2x2_f16x3.hip
// (DRUNet's 2 x 2 stride-2 and transposed convolutions).  DESIGN.md 4.8.
#pragma once
#include "conv_common.h"

namespace pnp {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

constexpr float H3_SCALE = 2048.f, H3_RSCALE = 1.f / 2048.f;
constexpr int H3_STR = 68;                       // floats between the staging rows of the epilogue
constexpr int H3_TAP16 = 1024;                   // 16-byte units of one 64 x 64 block of weights: [K step 2][N tile 4][hi, lo][lane 64]

// x = hi + lo / 2048,  hi = half(x),  lo = half((x - hi) * 2048)
__device__ __forceinline__ void split4(const f32x4& v, h4& hi, h4& lo) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        // two values at a time: ONE packed conversion for the hi halves; (x - h) * 2048 as fma(h, -2048, x * 2048) on the half as it is
        // (v_fma_mixlo / mixhi_f16) -- both forms are exact: the residual has at most 13 significant bits
        const f32x2 x = {v[2 * k], v[2 * k + 1]};
        const h2 h = __builtin_convertvector(x, h2);
        hi[2 * k] = h[0]; hi[2 * k + 1] = h[1];
        lo[2 * k] = (_Float16)__builtin_fmaf((float)h[0], -H3_SCALE, x[0] * H3_SCALE);
        lo[2 * k + 1] = (_Float16)__builtin_fmaf((float)h[1], -H3_SCALE, x[1] * H3_SCALE);
    }
}

// Packed weights, both families (the pack kernels run once per model): a 64 x 64 block is [K step s][N tile nt][lane 64][8 values j], lane
// (n, kb) of fragment (s, nt) holding rows k = 32 s + 8 kb + j of column 16 nt + n -- v_mfma_f32_16x16x32_f16: lane l supplies
// B[k = 8 (l >> 4) + j][column l & 15]; the A side reads input channels in the same order.  Thread o of a pack kernel owns value
// o = (((blk * 2 + s) * 4 + nt) * 64 + lane) * 8 + j.  SPLIT (f16x3): the fragment is a hi fragment followed by its lo fragment, 16 KiB per
// block, as many bytes as the float32 weights; else (f16) one fragment of halves rounded to nearest even, 8 KiB.
struct FragPos { long long blk; int s, nt, lane, j; };
__device__ __forceinline__ FragPos frag_pos(long long o) {
    return FragPos{o >> 12, (int)(o >> 11) & 1, (int)(o >> 9) & 3, (int)(o >> 3) & 63, (int)o & 7};
}
template <bool SPLIT>
__device__ __forceinline__ void frag_write(_Float16* wfrag, long long o, const FragPos& p, float v) {
    const _Float16 hi = (_Float16)v;
    if (SPLIT) {
        const size_t frag = ((size_t)p.blk * 2 + p.s) * 8 + p.nt * 2;
        wfrag[(frag * 64 + p.lane) * 8 + p.j] = hi;
        wfrag[((frag + 1) * 64 + p.lane) * 8 + p.j] = (_Float16)((v - (float)hi) * H3_SCALE);
    } else {
        wfrag[o] = hi;
    }
}
// torch.nn.Conv2d weight [C out][C in][3][3] -> blocks [cb][chunk cc][tap]: value (s, nt, lane (n, kb), j) is
// W[out = 64 cb + 16 nt + n][in = 64 cc + 32 s + 8 kb + j][tap]
template <bool SPLIT>
__device__ __forceinline__ void conv_pack_w_body(const float* w_oihw, _Float16* wfrag, int C) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;      // one value per thread
    if (o >= 9LL * C * C) return;
    const int NC = C >> 6;
    const FragPos p = frag_pos(o);                                // blk = (cb * NC + cc) * 9 + tap
    const int tap = (int)(p.blk % 9), cc = (int)((p.blk / 9) % NC), cb = (int)(p.blk / (9 * NC));
    const int out = 64 * cb + 16 * p.nt + (p.lane & 15), in = 64 * cc + 32 * p.s + 8 * (p.lane >> 4) + p.j;
    frag_write<SPLIT>(wfrag, o, p, w_oihw[((size_t)out * C + in) * 9 + tap]);
}

// The operand tile in LDS (kernels_conv_f16x3.hip): a pixel is 256 bytes of halves + 16 bytes of padding (CV_PS floats), in sixteen
// 16-byte chunks.  Chunk (kb, s2, part) = [hi | lo] halves of input channels 32 s2 + 8 kb .. + 7 -- lane (i, kb) of a wave reads it as the
// A fragment of K step s2 -- sits at h3_chunk_pos: the chunks of kb and kb ^ 1 lie 128 bytes apart, and the wave's M-tile row i is tile
// column h3_row_pixel(i) (columns 0-3 and 4-7 exchanged).  Why: ds_read_b128 serves the lanes in the groups {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS table), i.e. rows {0-3, 12-15} of kb = 0 together with rows 4-11 of kb = 1.  In the
// straightforward order (chunk = 4 s2 + kb, row i = column i: rounds 4's layout) those sixteen 16-byte accesses fall on 15 distinct
// bank quads -- every A read takes 8 LDS cycles instead of 4, a quarter of the kernel's LDS cycles (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE
// = 0.23).  With the pair 128 bytes apart and the two column quads exchanged the sixteen accesses of every group cover the 64 banks
// exactly once -- same bytes of LDS, the same immediate offsets per tap, no address arithmetic added.
__device__ __forceinline__ constexpr int h3_chunk_pos(int kb, int s2, int part) { return ((kb & 1) * 8 + (kb >> 1) * 4 + s2 * 2 + part) * 16; }
__device__ __forceinline__ int h3_row_pixel(int i) { return (i & 8) ? i : (i ^ 4); }

// The SPLIT activation format: what the f16x3 kernels hand to each other between layers instead of float32.  Same shape, same bytes --
// [n][H][W][C] with 256 bytes per pixel and block of 64 channels -- but a block is [64 hi halves][64 lo halves] of its 64 values
// (the operand layout of the kernels' LDS tiles): the producing layer splits each output value ONCE in its epilogue, and a consuming
// layer copies 16-byte runs of halves into its tile instead of splitting every value of every tile (halo included) again for every
// block of output channels.  A value read back is hi + lo / 2048: the float32 result rounded to 2^-22 relative -- the precision the
// consumer's operands had anyway.
__device__ __forceinline__ float unsplit(const _Float16 hi, const _Float16 lo) { return fmaf((float)lo, H3_RSCALE, (float)hi); }

}  // namespace pnp
