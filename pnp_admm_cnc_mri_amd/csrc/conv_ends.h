// The stacks' first and last layers, what the arithmetic families share of them:
//   * the first layer (k_conv3x3_head in kernels_conv.hip, k_conv3x3_head_f16 in kernels_conv_f16.hip): ONE body, float32 arithmetic
//     on the float32 network input, storing float32 or halves;
//   * the last layer on the matrix cores (k_conv3x3_tail_h3 in kernels_conv_f16x3.hip, k_conv3x3_tail_f16 in kernels_conv_f16.hip):
//     arguments, launcher, the weights' order in LDS and the epilogue.  Staging and the tap loops stay with each family: the LDS layouts
//     differ on purpose, and so does the handling of x2.
#pragma once
#include "f16_common.h"

namespace pnp {

// ------------------------------------------------------------------------------------------
// First layer of the plain stacks (models/network_dncnn.py:52-62, models/network_ffdnet.py:50-56): few input channels -- no matrix-core
// shape, and bound by the 64-channel tensor it writes.  A direct convolution on the vector units, one 256-thread workgroup per 8 x 16
// pixel tile, 16 lanes per group of 8 consecutive pixels:
//   x [n][CIN][H][W] (NCHW, CIN <= 8)  ->  y [n][H][W][64] (NHWC), + bias, ReLU: lane cq of a group computes channels 4 cq .. 4 cq + 3
//   of its 8 pixels (acc 32 registers); inputs and weights from LDS (broadcast reads)
// ------------------------------------------------------------------------------------------
constexpr int HD_HX = Geo<1>::HX, HD_HY = Geo<1>::HY, HD_MAXC = CP_MAX_CIN;
struct HeadArgs {
    const float* x; const float* w; const float* bias; void* y;
    int n, cin, H, W, tiles_x, tiles_y, relu;
    // FFDNet's input stage folded into the staging loop (models/network_ffdnet.py:58-68): x is the FULL-resolution image [n][1][src_h][src_w];
    // channels 0..3 of the layer's input are its pixel-unshuffled quarters (channel 2 dy + dx at (y, x) = x[2 y + dy][2 x + dx], replicate-padded
    // to even size = index clamped), channel 4 the noise level sigma[img * sigma_stride]; H = ceil(src_h / 2), W = ceil(src_w / 2)
    int ffdnet, src_h, src_w, sigma_stride;
    const float* sigma;
};
template <bool HALF>                                              // y is half (rounded once, on store) instead of float32
__device__ __forceinline__ void conv3x3_head_body(const HeadArgs& a) {
    __shared__ float xin[HD_MAXC * HD_HY * HD_HX];                 // [ci][row 10][col 18]
    __shared__ __attribute__((aligned(16))) float wl[HD_MAXC * 9 * CV_C];   // [ci * 9 + tap][64 out]
    const int tid = threadIdx.x;
    const int per_img = a.tiles_x * a.tiles_y;
    const int img = blockIdx.x / per_img, trem = blockIdx.x - img * per_img, ty = trem / a.tiles_x;
    const int y0 = ty * CV_TY, x0 = (trem - ty * a.tiles_x) * CV_TX;
    const size_t plane = (size_t)a.H * a.W;
    const float* xb = a.ffdnet ? a.x + (size_t)img * a.src_h * a.src_w : a.x + (size_t)img * a.cin * plane;
    const float sig = a.ffdnet ? a.sigma[(size_t)img * a.sigma_stride] : 0.f;
    if (a.ffdnet) {
        // the full-resolution patch, 2 HD_HY rows x 2 HD_HX columns, read row by row (consecutive threads, consecutive pixels) and
        // de-interleaved into the four channel planes on the way into LDS
        for (int e = tid; e < 4 * HD_HY * HD_HX; e += 256) {
            const int pr = e / (2 * HD_HX), pc = e - pr * (2 * HD_HX), r = pr >> 1, c = pc >> 1, ci = 2 * (pr & 1) + (pc & 1);
            const int gy = y0 - 1 + r, gx = x0 - 1 + c;
            const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            const int sy = min(2 * (in ? gy : 0) + (pr & 1), a.src_h - 1), sx = min(2 * (in ? gx : 0) + (pc & 1), a.src_w - 1);
            const float v = xb[(size_t)sy * a.src_w + sx];
            xin[(ci * HD_HY + r) * HD_HX + c] = in ? v : 0.f;
        }
        for (int p = tid; p < HD_HY * HD_HX; p += 256) {           // the convolution zero-pads the noise-level channel too
            const int r = p / HD_HX, c = p - r * HD_HX, gy = y0 - 1 + r, gx = x0 - 1 + c;
            xin[4 * HD_HY * HD_HX + p] = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? sig : 0.f;
        }
    } else {
        for (int e = tid; e < a.cin * HD_HY * HD_HX; e += 256) {
            const int ci = e / (HD_HY * HD_HX), p = e - ci * (HD_HY * HD_HX), r = p / HD_HX, c = p - r * HD_HX;
            const int gy = y0 - 1 + r, gx = x0 - 1 + c;
            const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            const float v = xb[(size_t)ci * plane + (size_t)(in ? gy : 0) * a.W + (in ? gx : 0)];
            xin[e] = in ? v : 0.f;
        }
    }
    for (int e = tid; e < a.cin * 9 * CV_C; e += 256) {            // w_oihw [64][cin][3][3] -> [ci * 9 + tap][out]
        const int out = e & 63, k = e >> 6;                        // k = ci * 9 + tap
        wl[e] = a.w[(size_t)out * a.cin * 9 + k];
    }
    __syncthreads();
    const int cq = tid & 15, pg = tid >> 4, row = pg >> 1, col0 = (pg & 1) * 8;
    f32x4 acc[8];
    const f32x4 b4 = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + 4 * cq) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int px = 0; px < 8; ++px) acc[px] = b4;
#pragma unroll 1
    for (int ci = 0; ci < a.cin; ++ci) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            float in[10];
            const float* rp = xin + (ci * HD_HY + row + ky) * HD_HX + col0;
#pragma unroll
            for (int k = 0; k < 10; ++k) in[k] = rp[k];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wl + (ci * 9 + ky * 3 + kx) * CV_C + 4 * cq);
#pragma unroll
                for (int px = 0; px < 8; ++px) {
                    acc[px][0] = fmaf(in[px + kx], w4[0], acc[px][0]); acc[px][1] = fmaf(in[px + kx], w4[1], acc[px][1]);
                    acc[px][2] = fmaf(in[px + kx], w4[2], acc[px][2]); acc[px][3] = fmaf(in[px + kx], w4[3], acc[px][3]);
                }
            }
        }
    }
    constexpr int PIX = CV_C * (HALF ? 2 : 4);                    // bytes of a pixel of y
    const __amdgpu_buffer_rsrc_t ry = bytes_rsrc(a.y, (size_t)img * plane * PIX, (unsigned)plane * (unsigned)PIX);
    const int gy = y0 + row;
#pragma unroll
    for (int px = 0; px < 8; ++px) {
        const int gx = x0 + col0 + px;
        f32x4 v = acc[px];
        if (a.relu) { v[0] = relu_keep_nan(v[0]); v[1] = relu_keep_nan(v[1]); v[2] = relu_keep_nan(v[2]); v[3] = relu_keep_nan(v[3]); }
        const int off = (gx < a.W) ? (gy * a.W + gx) * PIX + cq * (PIX / 16) : -16;        // rows below the image: out of range, dropped
        if (HALF) {
            const h4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, hv), ry, off, 0, 0);
        } else {
            const u32x4v o = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
            __builtin_amdgcn_raw_buffer_store_b128(o, ry, off, 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Last layer of the stacks on the matrix cores (64 -> COUT <= 4 channels, NHWC in, float32 NCHW out, + bias; models/network_ffdnet.py:56,
// network_dncnn.py:62): a 16-column matrix product of which COUT columns are used, per wave two M tiles (its two tile rows) x one N tile,
// 18 K steps of 32.  Persistent, two workgroups per compute unit; bound by reading its input.
// ------------------------------------------------------------------------------------------
struct TailMmaArgs {
    const void* x; const void* x2; const float* w; const float* bias; float* y;      // x2: null, or a tensor of x's shape added to it (the U-Net's last skip sum)
    int n, cout, H, W, tiles_x, tiles_y;
    // FFDNet's output stage folded into the stores (models/network_ffdnet.py:70-73): cout = 4, and channel 2 dy + dx of pixel (y, x) is pixel
    // (2 y + dy, 2 x + dx) of the ONE-channel full-resolution result y [n][1][out_h][out_w] (pixel shuffle + the crop of the padded row / column)
    int shuffle, out_h, out_w;
};
constexpr int TAIL_WL = 9 * 2 * 4 * 4 * 8;                        // weights a workgroup keeps in LDS: [tap][K step s2][kb][n < 4][8 values j]
// value e of that order: w_oihw [cout][64][3][3] at out = n, in = 32 s2 + 8 kb + j (columns >= cout: zeros)
__device__ __forceinline__ float tail_mma_weight(const TailMmaArgs& t, int e) {
    const int j = e & 7, n = (e >> 3) & 3, kq = (e >> 5) & 3, s2 = (e >> 7) & 1, tap = e >> 8;
    return n < t.cout ? t.w[((size_t)n * 64 + 32 * s2 + 8 * kq + j) * 9 + tap] : 0.f;
}
// The epilogue of tile q.  Lane (i, kb) holds output channel i (`col`: i < cout; b: its bias) of the pixels (tile row 2 w + mt, column
// col0 + r): value[mt][r] -- col0 = 4 kb, or where the family's M-tile rows map to (f16x3: h3_row_pixel(4 kb)).  Every wave is past its
// taps (the caller's barrier): `blk`, the start of the input tile, may be reused.
__device__ __forceinline__ void tail_mma_store(const TailMmaArgs& t, const TilePos& q, float* blk, int tid, int wv, int i, int col0, bool col, float b, const f32x4 (&value)[2]) {
    if (t.shuffle) {
        // FFDNet: the tile's 8 x 16 x 4 values are a 16 x 32 block of the full-resolution result; it is assembled in LDS and leaves as
        // whole rows, two consecutive pixels per thread
        if (col) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    blk[(2 * (2 * wv + mt) + (i >> 1)) * 32 + 2 * (col0 + r) + (i & 1)] = value[mt][r] + b;
        }
        __syncthreads();
        const int orow = tid >> 4, ocol = 2 * (tid & 15), oy = 2 * q.y0 + orow, ox = 2 * q.x0 + ocol;
        if (oy < t.out_h) {
            float* dst = t.y + ((size_t)q.img * t.out_h + oy) * t.out_w + ox;
            if (ox < t.out_w) dst[0] = blk[orow * 32 + ocol];
            if (ox + 1 < t.out_w) dst[1] = blk[orow * 32 + ocol + 1];
        }
        __syncthreads();                                      // the assembled block is read: the next tile may be written
    } else if (col) {
        const size_t plane = (size_t)t.H * t.W;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int gy = q.y0 + 2 * wv + mt;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gx = q.x0 + col0 + r;
                if (gy < t.H && gx < t.W) t.y[((size_t)q.img * t.cout + i) * plane + (size_t)gy * t.W + gx] = value[mt][r] + b;
            }
        }
    }
}
static hipError_t launch_tail_mma(hipStream_t s, void (*kern)(TailMmaArgs, int), const void* x_nhwc, const void* x2_nhwc, const float* w_oihw, const float* bias,
                                  float* y, int n, int cout, int H, int W, int shuffle_h, int shuffle_w) {
    if (cp_check_tail(n, cout, H, W, shuffle_h, shuffle_w)) return hipErrorInvalidValue;
    const ConvTiling tl = cp_tiling(n, H, W, CP_NARROW);
    TailMmaArgs t;
    t.shuffle = shuffle_h ? 1 : 0; t.out_h = shuffle_h; t.out_w = shuffle_w;
    t.x = x_nhwc; t.x2 = x2_nhwc; t.w = w_oihw; t.bias = bias; t.y = y; t.n = n; t.cout = cout; t.H = H; t.W = W;
    t.tiles_x = tl.tiles_x; t.tiles_y = tl.tiles_y;
    const int cus = conv_compute_units();
    if (cus <= 0) return hipGetLastError();
    // persistent, two workgroups per compute unit; every loop ends: tile < ntiles
    hipLaunchKernelGGL(kern, dim3((unsigned)cp_grid(tl.items, 2, cus)), dim3(CV_THREADS), 0, s, t, (int)tl.items);
    return hipGetLastError();
}

}  // namespace pnp
