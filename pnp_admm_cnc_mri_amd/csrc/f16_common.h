// Shared by the half-precision ("f16") matrix-core kernels: kernels_conv_f16.hip (conv3x3 C -> C, the stacks' first and last layers)
// and kernels_pix2x2_f16.hip (DRUNet's 2 x 2 stride-2 and transposed convolutions).  DESIGN.md 4.12.
//
// Activations between layers are IEEE halves, NHWC: 128 bytes per pixel and block of 64 channels.  A layer multiplies half operands on
// v_mfma_f32_16x16x32_f16 (exact products), accumulates in float32, adds bias and skip in float32 and rounds ONCE, on store.
#pragma once
#include "f16x3_common.h"                       // h8 / h4, H3_STR, relu_keep_nan, tile geometry (conv_common.h)

namespace pnp {

// which tensors of a launch are float32 instead of half (include/pnp_mri.h: PNP_F16_*_F32)
constexpr int HF_FMT_X32 = 1, HF_FMT_SKIP32 = 2, HF_FMT_Y32 = 4;

// The operand tile in LDS: a pixel is 128 bytes of halves + 32 bytes of padding; chunk 4 s2 + kb (16 bytes) = input channels 32 s2 + 8 kb
// .. + 7 -- lane (i, kb) of a wave reads it as the A fragment of K step s2 with one ds_read_b128.  ds_read_b128 serves the lanes in the
// groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...: rows {0-3, 12-15} of kb = 0 together with rows 4-11 of kb = 1.  With 160 bytes
// = 40 banks between pixels the eight rows of either set start on the eight multiples of 8 banks, and the chunk of kb = 1 lies four
// banks behind: the sixteen accesses of a group cover the 64 banks exactly once.  (144 bytes, the next smaller stride that keeps 16-byte
// alignment, would need the chunks of kb and kb ^ 1 a multiple of 128 bytes apart -- the pixel has no room for that.)
constexpr int HF_PS = 160;
constexpr int HF_TAP16 = 512;                    // 16-byte units of one 64 x 64 block of half weights: [K step 2][N tile 4][lane 64]

template <int DIL> struct GeoF {
    static constexpr int HX = Geo<DIL>::HX, HY = Geo<DIL>::HY;
    static constexpr int XU = (HY * HX * 8 + CV_THREADS - 1) / CV_THREADS;      // 16-byte chunks (8 halves) of the tile per thread: 6 at dilation 1
    static constexpr int XINB = HY * HX * HF_PS;                                // bytes of the tile
};

typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));

// `bytes` from `base + off`, as a raw buffer
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bytes_rsrc(const void* base, size_t off, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(base) + off), 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ h8 round8(const f32x4& a, const f32x4& b) {
    return h8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3], (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
}
__device__ __forceinline__ f32x4 as_f32x4(const u32x4v& w) {
    return f32x4{__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w)};
}

// Input staging: chunk u of thread tid is channels 8 (tid & 7) .. + 7 of tile pixel p = (tid >> 3) + 32 u = (row r, column c);
// pk[u] = (r W + c) * pix | c -- pix (bytes between pixels of the tensor) is a multiple of 128 and c < 32: the low seven bits are free
// for the column, the only coordinate that needs a test (rows fall out of the buffer's range by themselves: conv_plan.h keeps
// (H + CP_SPARE_ROWS) W pix below 2^31, so the 32-bit offset of a halo or overhang row cannot wrap back into range) -- or -1: no such chunk.
template <int DIL> struct StagingF { int pk[GeoF<DIL>::XU]; };
template <int DIL>
__device__ __forceinline__ void staging_init_f(int W, int tid, StagingF<DIL>& st, const int pix) {
    constexpr int HX = GeoF<DIL>::HX, HY = GeoF<DIL>::HY;
#pragma unroll
    for (int u = 0; u < GeoF<DIL>::XU; ++u) {
        const int p = (tid >> 3) + 32 * u, r = p / HX, c = p - r * HX;
        st.pk[u] = (p < HY * HX) ? (((r * W + c) * pix) | c) : -1;
    }
}
// what the pieces of one tile's request share.  X32: the tensor is float32 (a chunk is two 16-byte loads), else half (one)
struct FetchF { __amdgpu_buffer_rsrc_t rs; int origin, xlo, xhi; };
template <int DIL, bool X32>
__device__ __forceinline__ FetchF fetch_begin_f(const void* x, int H, int W, const TilePos& q, int tid, const int pix, const int coff_bytes, const bool any = true) {
    FetchF f;
    // any = false: a descriptor of zero bytes -- every piece is still ISSUED (the counted waits rely on their number) but none reaches memory
    const unsigned bytes = any ? (unsigned)H * (unsigned)W * (unsigned)pix - (unsigned)coff_bytes : 0u;
    f.rs = bytes_rsrc(x, (size_t)q.img * H * W * pix + (any ? coff_bytes : 0), bytes);
    f.origin = ((q.y0 - DIL) * W + (q.x0 - DIL)) * pix + (X32 ? 32 : 16) * (tid & 7);      // may be negative: out of range as unsigned
    f.xlo = DIL - q.x0; f.xhi = W + DIL - q.x0;                                            // valid tile columns: xlo <= c < xhi
    return f;
}
template <int DIL, bool X32> struct XRegs { u32x4v v[GeoF<DIL>::XU * (X32 ? 2 : 1)]; };
template <int DIL, bool X32, int U0, int U1>
__device__ __forceinline__ void fetch_piece_f(const FetchF& f, const StagingF<DIL>& st, XRegs<DIL, X32>& x) {
#pragma unroll
    for (int u = U0; u < U1 && u < GeoF<DIL>::XU; ++u) {
        const int c = st.pk[u] & 127;
        const bool in = st.pk[u] >= 0 && c >= f.xlo && c < f.xhi;
        const int off = in ? f.origin + (st.pk[u] & ~127) : -32;
        if constexpr (X32) {
            x.v[2 * u] = __builtin_amdgcn_raw_buffer_load_b128(f.rs, off, 0, 0);
            x.v[2 * u + 1] = __builtin_amdgcn_raw_buffer_load_b128(f.rs, in ? off + 16 : -16, 0, 0);
        } else {
            x.v[u] = __builtin_amdgcn_raw_buffer_load_b128(f.rs, off, 0, 0);
        }
    }
}
// registers -> LDS tile; float32 values are rounded to half here (round to nearest even, beyond +-65504: inf).  The eight lanes of a
// pixel write its 128 bytes: ds_write_b128 serves 8 contiguous lanes per cycle, 32 distinct banks.
template <int DIL, bool X32>
__device__ __forceinline__ void put_input_f(char* xin, int tid, const XRegs<DIL, X32>& x) {
    char* px = xin + (tid >> 3) * HF_PS + (tid & 7) * 16;
#pragma unroll
    for (int u = 0; u < GeoF<DIL>::XU; ++u)
        if ((tid >> 3) + 32 * u < GeoF<DIL>::HY * GeoF<DIL>::HX) {
            if constexpr (X32) *reinterpret_cast<h8*>(px + u * (32 * HF_PS)) = round8(as_f32x4(x.v[2 * u]), as_f32x4(x.v[2 * u + 1]));
            else *reinterpret_cast<u32x4v*>(px + u * (32 * HF_PS)) = x.v[u];
        }
}

}  // namespace pnp
