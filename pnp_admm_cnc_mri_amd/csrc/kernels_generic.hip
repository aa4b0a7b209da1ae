// Generic c2c kernels of libpnpmri.so for gfx950: any H, W in {256, 512}.
//
// These implement, transform by transform, what np.fft.fft2 / np.fft.ifft2 and the surrounding
// NumPy lines of the reference do (S4:119-124 etc.; see include/pnp_mri.h).  They are the
// operator API (fft2, A, A^H, Df, synthesis, init) and the fallback of the iteration for shapes
// the fused 256x256 kernels (kernels_fused256.hip) do not cover.
//
// FFT: autosort (Stockham) radix-4 stages (+ one radix-2 stage for 512) in LDS, ping-pong
// buffers, twiddles from an fp64-generated fp32 table W_N^m = exp(-2 pi i m / N) staged in LDS.
//   rows   : one wavefront (64 lanes) per row, 4 rows per 256-thread workgroup
//   columns: a tile of 16 columns x N rows per workgroup, transposed into LDS on load so the
//            same row routine runs on it (16 lanes per column); global accesses are 128-B row
//            segments; the LDS pitch N+1 keeps the transposing writes conflict-free.
// What a row launch (RowIn, inverse, RowEpi) and a column launch (pre, ColMid, post) read, compute per element and write, the legal
// triples and the complex helpers: c2c_roles.h, shared with kernels_anysize.hip.
#include "internal.h"
#include "fft16.h"
#include <math.h>
#include <stdint.h>
#include <initializer_list>

namespace pnp {

__device__ float2 g_tw256[256];
__device__ float2 g_tw512[512];
__device__ double2 g_tw256d[256];      // fp64 validation context
__device__ double2 g_tw512d[512];

hipError_t upload_twiddles() {
    static thread_local float2 h[512];
    static thread_local double2 hd[512];
    for (int N : {256, 512}) {
        for (int m = 0; m < N; ++m) {
            const double a = -2.0 * M_PI * (double)m / (double)N;
            hd[m] = make_double2(cos(a), sin(a));
            h[m] = make_float2((float)hd[m].x, (float)hd[m].y);
        }
        hipError_t e = (N == 256) ? hipMemcpyToSymbol(HIP_SYMBOL(g_tw256), h, sizeof(float2) * 256)
                                  : hipMemcpyToSymbol(HIP_SYMBOL(g_tw512), h, sizeof(float2) * 512);
        if (e != hipSuccess) return e;
        e = (N == 256) ? hipMemcpyToSymbol(HIP_SYMBOL(g_tw256d), hd, sizeof(double2) * 256)
                       : hipMemcpyToSymbol(HIP_SYMBOL(g_tw512d), hd, sizeof(double2) * 512);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename R> struct Tw;
template <> struct Tw<float>  { __device__ static const float2*  get(int N) { return N == 256 ? g_tw256 : g_tw512; } };
template <> struct Tw<double> { __device__ static const double2* get(int N) { return N == 256 ? g_tw256d : g_tw512d; } };

// The T threads of one transform are lanes of ONE wavefront (T <= 64, groups aligned to T): a wave's LDS instructions
// execute in order, so the stages need no workgroup barrier -- only the compiler has to keep the order.  (Until round 3
// every stage ended in __syncthreads(): 9-10 workgroup barriers per transform held every column of a tile to the pace of
// the slowest wave; the column kernel ran at 0.18 of the HBM roofline.)
__device__ __forceinline__ void stage_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Length-N transform of the contiguous LDS array `a` by T cooperating lanes of one wave (t in [0,T)), scratch `b`.
// No workgroup barrier inside: the caller orders its own cross-wave accesses around the call.
// Returns the buffer holding the result (natural order).
template <int N, int T, bool INV, typename C>
__device__ __forceinline__ C* fft_lds(C* a, C* b, const C* tw, int t) {
    static_assert(N == 256 || N == 512, "N");
    static_assert(T <= 64 && 64 % T == 0, "the lanes of a transform must share a wavefront");
    int Ns = 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        for (int j = t; j < N / 4; j += T) {
            const int k = j & (Ns - 1);
            const int ti = k * (N / (Ns * 4));
            C v0 = a[j], v1 = a[j + N / 4], v2 = a[j + N / 2], v3 = a[j + 3 * N / 4];
            if (s > 0) {
                const C w1 = tw[ti], w2 = tw[2 * ti], w3 = tw[3 * ti];
                if (INV) { v1 = cmulc(v1, w1); v2 = cmulc(v2, w2); v3 = cmulc(v3, w3); }
                else     { v1 = cmul(v1, w1);  v2 = cmul(v2, w2);  v3 = cmul(v3, w3); }
            }
            const C t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3);
            const C d = csub(v1, v3);
            const C t3 = INV ? mkc<C>(-d.y, d.x) : mkc<C>(d.y, -d.x);   // (+/-) i * d
            const int j0 = ((j - k) << 2) + k;
            b[j0] = cadd(t0, t2);
            b[j0 + Ns] = cadd(t1, t3);
            b[j0 + 2 * Ns] = csub(t0, t2);
            b[j0 + 3 * Ns] = csub(t1, t3);
        }
        stage_sync();
        C* tmp = a; a = b; b = tmp;
        Ns *= 4;
    }
    if (N == 512) {                                   // final radix-2 stage, Ns = 256
        for (int j = t; j < N / 2; j += T) {
            const int k = j & 255;
            C v0 = a[j], v1 = a[j + N / 2];
            v1 = INV ? cmulc(v1, tw[k]) : cmul(v1, tw[k]);
            const int j0 = ((j - k) << 1) + k;
            b[j0] = cadd(v0, v1);
            b[j0 + 256] = csub(v0, v1);
        }
        stage_sync();
        C* tmp = a; a = b; b = tmp;
    }
    return a;
}

// ------------------------------------------------------------------------------------------
// rows: one wavefront per row; 4 rows per workgroup (2 in fp64: same LDS footprint)
// ------------------------------------------------------------------------------------------
template <typename R> struct RowCfg { static constexpr int ROWS = sizeof(R) == 8 ? 2 : 4; };

template <int N, int IN, bool INV, int EPI, typename R>
__global__ __launch_bounds__(256) void k_rows(RowArgsT<R> p) {
    using C = typename CxOf<R>::type;
    constexpr int T = 64, ROWS = RowCfg<R>::ROWS;
    __shared__ C sA[ROWS * N];
    __shared__ C sB[ROWS * N];
    __shared__ C sTw[N];
    const int tid = threadIdx.x, lane = tid & 63, rw = tid >> 6;
    const C* gtw = Tw<R>::get(N);
    for (int i = tid; i < N; i += ROWS * 64) sTw[i] = gtw[i];
    const int row = blockIdx.x * ROWS + rw;                    // nrows is a multiple of ROWS
    const size_t base = (size_t)row * N;
    C* a = sA + rw * N;
    C* b = sB + rw * N;
#pragma unroll
    for (int i = 0; i < N / T; ++i) {
        const int n = lane + i * T;
        a[n] = row_load<IN>(p, base + n);
    }
    __syncthreads();
    C* r = fft_lds<N, T, INV>(a, b, sTw, lane);
#pragma unroll
    for (int i = 0; i < N / T; ++i) {
        const int n = lane + i * T;
        row_store<EPI>(p, base + n, r[n]);
    }
}

template <int N, int IN, bool INV, int EPI, typename R>
static hipError_t launch_rows_t(hipStream_t s, const RowArgsT<R>& a) {
    constexpr int ROWS = RowCfg<R>::ROWS;
    hipLaunchKernelGGL((k_rows<N, IN, INV, EPI, R>), dim3(a.nrows / ROWS), dim3(ROWS * 64), 0, s, a);
    return hipGetLastError();
}

template <int N, typename R>
static hipError_t launch_rows_n(hipStream_t s, RowIn in, bool inv, RowEpi epi, const RowArgsT<R>& a) {
    return row_roles(in, inv, epi, hipErrorInvalidValue,
                     [&](auto IN, auto INV, auto EPI) { return launch_rows_t<N, IN(), INV(), EPI()>(s, a); });
}

template <typename R>
hipError_t launch_rows(hipStream_t s, int W, RowIn in, bool inv, RowEpi epi, const RowArgsT<R>& a) {
    if (a.nrows % RowCfg<R>::ROWS) return hipErrorInvalidValue;
    if (W == 256) return launch_rows_n<256>(s, in, inv, epi, a);
    if (W == 512) return launch_rows_n<512>(s, in, inv, epi, a);
    return hipErrorInvalidValue;
}
template hipError_t launch_rows<float>(hipStream_t, int, RowIn, bool, RowEpi, const RowArgsT<float>&);
template hipError_t launch_rows<double>(hipStream_t, int, RowIn, bool, RowEpi, const RowArgsT<double>&);

// ------------------------------------------------------------------------------------------
// columns: [optional forward] -> pointwise k-space op -> [optional inverse]
// tile = COLS columns x N rows, COLS = 16 (8 for fp64 at N = 512: LDS), 256/COLS lanes per column
// ------------------------------------------------------------------------------------------
template <int N, typename R> struct ColCfg { static constexpr int COLS = (sizeof(R) == 8 && N == 512) ? 8 : 16; };

template <int N, bool PRE, int MID, bool POST, typename R>
__global__ __launch_bounds__(256) void k_cols(ColArgsT<R> p, int W) {
    using C = typename CxOf<R>::type;
    constexpr int COLS = ColCfg<N, R>::COLS, T = 256 / COLS, P = N + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    C* sA = reinterpret_cast<C*>(smem_raw);     // [COLS][P]
    C* sB = sA + COLS * P;
    C* sTw = sA + 2 * COLS * P;
    const int tid = threadIdx.x;
    const C* gtw = Tw<R>::get(N);
    for (int i = tid; i < N; i += 256) sTw[i] = gtw[i];
    const int tiles = W / COLS;
    const int b = blockIdx.x / tiles;
    const int k0 = (blockIdx.x % tiles) * COLS;
    const size_t sbase = (size_t)b * N * W;
    for (int idx = tid; idx < N * COLS; idx += 256) {
        const int r = idx / COLS, c = idx % COLS;
        sA[c * P + r] = p.in[sbase + (size_t)r * W + k0 + c];
    }
    __syncthreads();
    const int c_f = tid / T, t_f = tid % T;
    C* cur = sA;
    C* oth = sB;
    if (PRE) {
        C* r = fft_lds<N, T, false>(sA + c_f * P, sB + c_f * P, sTw, t_f);
        if (r != sA + c_f * P) { cur = sB; oth = sA; }
    }
    if (MID != MID_NONE) {
        __syncthreads();                                  // the pointwise pass walks the tile row-major: other waves' columns
        const int mid = p.mask_id ? p.mask_id[b] : 0;
        const uint8_t* mask = p.mask_bank + (size_t)mid * N * W;
        const C* yb = p.y + ((MID == MID_MASK_ADD && !p.y_per_slice) ? 0 : sbase);
        for (int idx = tid; idx < N * COLS; idx += 256) {
            const int r = idx / COLS, c = idx % COLS;
            const size_t g = (size_t)r * W + k0 + c;
            cur[c * P + r] = col_mid<MID>(cur[c * P + r], mask[g] != 0, &yb[g], p.c);
        }
        __syncthreads();
    }
    if (POST) {
        C* r = fft_lds<N, T, true>(cur + c_f * P, oth + c_f * P, sTw, t_f);
        if (r != cur + c_f * P) { C* tmp = cur; cur = oth; oth = tmp; }
    }
    __syncthreads();
    for (int idx = tid; idx < N * COLS; idx += 256) {
        const int r = idx / COLS, c = idx % COLS;
        p.out[sbase + (size_t)r * W + k0 + c] = cur[c * P + r];
    }
}

template <int N, bool PRE, int MID, bool POST, typename R>
static hipError_t launch_cols_t(hipStream_t s, int W, const ColArgsT<R>& a) {
    using C = typename CxOf<R>::type;
    constexpr int COLS = ColCfg<N, R>::COLS;
    const size_t lds = sizeof(C) * (2 * COLS * (N + 1) + N);
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_cols<N, PRE, MID, POST, R>, done, lds, lds)) return e;
    hipLaunchKernelGGL((k_cols<N, PRE, MID, POST, R>), dim3(a.B * (W / COLS)), dim3(256), lds, s, a, W);
    return hipGetLastError();
}

template <int N, typename R>
static hipError_t launch_cols_n(hipStream_t s, int W, bool pre, ColMid mid, bool post, const ColArgsT<R>& a) {
    return col_roles(pre, mid, post, hipErrorInvalidValue,
                     [&](auto PRE, auto MID, auto POST) { return launch_cols_t<N, PRE(), MID(), POST()>(s, W, a); });
}

// ------------------------------------------------------------------------------------------
// columns of 256-row float arrays: the register transform of fft16.h (16 lanes x 16 points, ONE exchange through LDS)
// instead of four LDS stages.  Same tile (16 columns x 256 rows, 128-byte row segments in global memory), same
// pointwise pass; the Stockham kernel above stays for 512 rows and for double.
// (k_cols<256, true, 1, true, float> ran 526-536 us at 512 slices = 1.48 TB/s, bound by the latency of eight dependent
// LDS stages at two workgroups per compute unit; this one holds 40 KB of LDS: four workgroups per compute unit.)
// Tile pitch 273 complex: = 1 mod 16, so the transposing tile writes of 16 lanes (one row, 16 columns) hit 16 distinct
// bank pairs, and = 17 mod 32, so the b64 column reads of a 32-lane group (two columns x 16 lanes) overlap in one pair only.
// ------------------------------------------------------------------------------------------
constexpr int C16_P = 273;

template <bool INV>
__device__ __forceinline__ void col16_fft(c32 (&a)[16], const c32* twl, c32* col, int t) {
    {
        c32 tw[16];                                 // the lane's row of the table, fetched per transform (not held across the kernel)
#pragma unroll
        for (int k = 0; k < 16; ++k) tw[k] = twl[17 * t + k];
        fft256_head<INV>(a, tw);
    }
    stage_sync();                                   // every lane of the column holds its inputs: the column's slot is free
#pragma unroll
    for (int k = 0; k < 16; ++k) col[k * 17 + t] = a[k];
    stage_sync();
#pragma unroll
    for (int n = 0; n < 16; ++n) a[n] = col[t * 17 + n];
    stage_sync();
    fft256_tail<INV>(a);
}

// The operands of the pointwise pass (measurements / noise, mask bytes) are requested at the START of the kernel, in the
// row-major order that pass walks (coalesced 128-byte row segments), and are consumed after the forward transform: their
// memory latency hides behind the tile load and the transform.  (Until round 4 they were fetched inside the pass, where
// every wave of the workgroup waited a full memory latency between two barriers: k_cols16<true, 1, true> 233 us at 512
// slices = 3.3 TB/s.)  y travels in 32 registers (3 workgroups per compute unit instead of 4); the mask tile (16 bytes per
// row) goes through 4 KiB of LDS as four dword loads per thread instead of sixteen byte loads.
template <bool PRE, int MID, bool POST>
__global__ __launch_bounds__(256, (MID != MID_NONE ? 3 : 4)) void k_cols16(ColArgsT<float> p, int W) {
    __shared__ __attribute__((aligned(16))) c32 tile[16 * C16_P];
    __shared__ c32 twl[16 * 17];
    __shared__ uint32_t mtile[MID != MID_NONE ? 1024 : 1];           // [row 256][4 dwords = 16 mask bytes]
    const int tid = threadIdx.x;
    {
        const float2 wv = g_tw256[((tid >> 4) * (tid & 15)) & 255];
        twl[17 * (tid >> 4) + (tid & 15)] = mk<float>(wv.x, wv.y);          // [t][k] = W256^(t k)
    }
    const int tiles = W / 16;
    const int b = blockIdx.x / tiles;
    const int k0 = (blockIdx.x % tiles) * 16;
    const size_t sbase = (size_t)b * 256 * W;
    const c32* in = reinterpret_cast<const c32*>(p.in);
    c32* out = reinterpret_cast<c32*>(p.out);
    c32 tin[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = tid + 256 * i, r = idx >> 4, c = idx & 15;
        tin[i] = in[sbase + (size_t)r * W + k0 + c];
    }
    uint32_t mq[4];
    c32 yv[16] = {};                                  // MID_MASK never fills it; col_mid takes its element by value
    if (MID != MID_NONE) {
        const int mid = p.mask_id ? p.mask_id[b] : 0;
        const uint32_t* mask4 = reinterpret_cast<const uint32_t*>(p.mask_bank + (size_t)mid * 256 * W + k0);   // k0 % 16 == 0: aligned
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = tid + 256 * u;                                      // row d >> 2, columns 4 (d & 3) .. + 3 of the tile
            mq[u] = mask4[(size_t)(d >> 2) * (W / 4) + (d & 3)];
        }
        if (MID != MID_MASK) {
            const c32* yb = reinterpret_cast<const c32*>(p.y) + ((MID == MID_MASK_ADD && !p.y_per_slice) ? 0 : sbase);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int idx = tid + 256 * i, r = idx >> 4, cc = idx & 15;
                yv[i] = yb[(size_t)r * W + k0 + cc];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = tid + 256 * i, r = idx >> 4, c = idx & 15;
        tile[c * C16_P + r] = tin[i];
    }
    if (MID != MID_NONE) {
#pragma unroll
        for (int u = 0; u < 4; ++u) mtile[tid + 256 * u] = mq[u];
    }
    __syncthreads();
    const int c = tid >> 4, t = tid & 15;
    c32* col = tile + c * C16_P;
    c32 a[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = col[t + 16 * j];
    if (PRE) col16_fft<false>(a, twl, col, t);
    if (MID != MID_NONE) {
        stage_sync();
#pragma unroll
        for (int j = 0; j < 16; ++j) col[t + 16 * j] = a[j];
        __syncthreads();                                  // the pointwise pass walks the tile row-major (the order its operands were fetched in)
        const uint8_t* mbytes = reinterpret_cast<const uint8_t*>(mtile);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int idx = tid + 256 * i, r = idx >> 4, cc = idx & 15;
            tile[cc * C16_P + r] = col_mid<MID>(tile[cc * C16_P + r], mbytes[16 * r + cc] != 0, yv[i], p.c);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = col[t + 16 * j];
    }
    if (POST) col16_fft<true>(a, twl, col, t);
    stage_sync();
#pragma unroll
    for (int j = 0; j < 16; ++j) col[t + 16 * j] = a[j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = tid + 256 * i, r = idx >> 4, cc = idx & 15;
        out[sbase + (size_t)r * W + k0 + cc] = tile[cc * C16_P + r];
    }
}

template <bool PRE, int MID, bool POST>
static hipError_t launch_cols16(hipStream_t s, int W, const ColArgsT<float>& a) {
    hipLaunchKernelGGL((k_cols16<PRE, MID, POST>), dim3(a.B * (W / 16)), dim3(256), 0, s, a, W);
    return hipGetLastError();
}
static hipError_t launch_cols16_any(hipStream_t s, int W, bool pre, ColMid mid, bool post, const ColArgsT<float>& a) {
    return col_roles(pre, mid, post, hipErrorInvalidValue,
                     [&](auto PRE, auto MID, auto POST) { return launch_cols16<PRE(), MID(), POST()>(s, W, a); });
}
// ------------------------------------------------------------------------------------------
// the same for 512-row float arrays: 32 lanes x 16 points per column (fft16.h: structure A forward, t-layout -> k-layout;
// structure B inverse, k-layout -> t-layout), 16 columns x 512 rows per 512-thread workgroup.
//   t-layout: lane t, register j <-> row t + 32 j;   k-layout: lane 2 k2 + h, register q <-> row k2 + 16 q + 256 h
// Column slot pitch 545 (= 1 mod 16: conflict-free transposing tile writes; >= 544 = the exchange region of 16 runs of 34).
// ------------------------------------------------------------------------------------------
constexpr int C32_P = 545;
__device__ __forceinline__ float lane_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true));
}
__device__ __forceinline__ void col32_fwd(c32 (&a)[16], const c32* twl, c32* col, int t) {       // t-layout -> k-layout
    const int k2 = t >> 1, h = t & 1;
    fft512_a1<false>(a, twl + 17 * t);
    stage_sync();
#pragma unroll
    for (int k = 0; k < 16; ++k) col[k * 34 + t] = a[k];
    stage_sync();
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = col[k2 * 34 + 2 * i + h];
    stage_sync();
    fft512_a2<false>(a, h);
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = bfly2(a[q], mk<float>(lane_xor1(a[q].x), lane_xor1(a[q].y)), h);
}
__device__ __forceinline__ void col32_inv(c32 (&a)[16], const c32* twl, c32* col, int t) {       // k-layout -> t-layout
    const int k2 = t >> 1, h = t & 1;
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = bfly2(a[q], mk<float>(lane_xor1(a[q].x), lane_xor1(a[q].y)), h);
    fft512_b1<true>(a, h);
    stage_sync();
#pragma unroll
    for (int i = 0; i < 16; ++i) col[k2 * 34 + 2 * i + h] = a[i];
    stage_sync();
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = col[k * 34 + t];
    stage_sync();
    fft512_b2<true>(a, twl + 17 * t);
}

template <bool PRE, int MID, bool POST>
__global__ __launch_bounds__(512, 4) void k_cols32(ColArgsT<float> p, int W) {      // 4 waves per SIMD = two workgroups per compute unit (74 KB of LDS each)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw32[];
    c32* tile = reinterpret_cast<c32*>(smem_raw32);            // [16][C32_P]
    c32* twl = tile + 16 * C32_P;                              // [32][17] = W512^(t k)
    const int tid = threadIdx.x;
    {
        const float2 wv = g_tw512[((tid >> 4) * (tid & 15)) & 511];
        twl[17 * (tid >> 4) + (tid & 15)] = mk<float>(wv.x, wv.y);
    }
    const int tiles = W / 16;
    const int b = blockIdx.x / tiles;
    const int k0 = (blockIdx.x % tiles) * 16;
    const size_t sbase = (size_t)b * 512 * W;
    const c32* in = reinterpret_cast<const c32*>(p.in);
    c32* out = reinterpret_cast<c32*>(p.out);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = tid + 512 * i, r = idx >> 4, c = idx & 15;
        tile[c * C32_P + r] = in[sbase + (size_t)r * W + k0 + c];
    }
    __syncthreads();
    const int c = tid >> 5, t = tid & 31, k2 = t >> 1, h = t & 1;
    c32* col = tile + c * C32_P;
    c32 a[16];
    if (PRE) {
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = col[t + 32 * j];
        col32_fwd(a, twl, col, t);
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) a[q] = col[k2 + 16 * q + 256 * h];
    }
    // a is in k-layout here
    if (MID != MID_NONE) {
        stage_sync();
#pragma unroll
        for (int q = 0; q < 16; ++q) col[k2 + 16 * q + 256 * h] = a[q];
        __syncthreads();                                  // the pointwise pass walks the tile row-major (coalesced y / mask reads)
        const int mid = p.mask_id ? p.mask_id[b] : 0;
        const uint8_t* mask = p.mask_bank + (size_t)mid * 512 * W;
        const c32* yb = reinterpret_cast<const c32*>(p.y) + ((MID == MID_MASK_ADD && !p.y_per_slice) ? 0 : sbase);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int idx = tid + 512 * i, r = idx >> 4, cc = idx & 15;
            const size_t g = (size_t)r * W + k0 + cc;
            tile[cc * C32_P + r] = col_mid<MID>(tile[cc * C32_P + r], mask[g] != 0, &yb[g], p.c);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) a[q] = col[k2 + 16 * q + 256 * h];
    }
    stage_sync();
    if (POST) {
        col32_inv(a, twl, col, t);
        stage_sync();
#pragma unroll
        for (int j = 0; j < 16; ++j) col[t + 32 * j] = a[j];
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) col[k2 + 16 * q + 256 * h] = a[q];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = tid + 512 * i, r = idx >> 4, cc = idx & 15;
        out[sbase + (size_t)r * W + k0 + cc] = tile[cc * C32_P + r];
    }
}

template <bool PRE, int MID, bool POST>
static hipError_t launch_cols32(hipStream_t s, int W, const ColArgsT<float>& a) {
    const size_t lds = sizeof(c32) * (16 * C32_P + 32 * 17);
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_cols32<PRE, MID, POST>, done, lds, lds)) return e;
    hipLaunchKernelGGL((k_cols32<PRE, MID, POST>), dim3(a.B * (W / 16)), dim3(512), lds, s, a, W);
    return hipGetLastError();
}
static hipError_t launch_cols32_any(hipStream_t s, int W, bool pre, ColMid mid, bool post, const ColArgsT<float>& a) {
    return col_roles(pre, mid, post, hipErrorInvalidValue,
                     [&](auto PRE, auto MID, auto POST) { return launch_cols32<PRE(), MID(), POST()>(s, W, a); });
}
// A/B knob of experiment builds (-DPNP_EXPERIMENT_KNOBS): PNP_GENERIC_STOCKHAM selects the four-stage LDS kernel for float too
static inline bool generic_stockham() {
#ifdef PNP_EXPERIMENT_KNOBS
    static const bool on = getenv("PNP_GENERIC_STOCKHAM") != nullptr;
    return on;
#else
    return false;
#endif
}
// float columns take the register transforms (k_cols16 / k_cols32); double, and float under the knob, the four-stage LDS kernel
template <int N, typename R>
static hipError_t cols_reg_or_stockham(hipStream_t s, int W, bool pre, ColMid mid, bool post, const ColArgsT<R>& a) {
    if constexpr (std::is_same<R, float>::value) {
        if (!generic_stockham()) return N == 256 ? launch_cols16_any(s, W, pre, mid, post, a) : launch_cols32_any(s, W, pre, mid, post, a);
    }
    return launch_cols_n<N>(s, W, pre, mid, post, a);
}

template <typename R>
hipError_t launch_cols(hipStream_t s, int H, int W, bool pre, ColMid mid, bool post, const ColArgsT<R>& a) {
    if (W % 16) return hipErrorInvalidValue;
    if (H == 256) return cols_reg_or_stockham<256>(s, W, pre, mid, post, a);
    if (H == 512) return cols_reg_or_stockham<512>(s, W, pre, mid, post, a);
    return hipErrorInvalidValue;
}
template hipError_t launch_cols<float>(hipStream_t, int, int, bool, ColMid, bool, const ColArgsT<float>&);
template hipError_t launch_cols<double>(hipStream_t, int, int, bool, ColMid, bool, const ColArgsT<double>&);

// ------------------------------------------------------------------------------------------
// pointwise kernels on caller pointers (PnP path, S6:301-308): 4 floats per lane, grid-stride; a scalar tail when n % 4 != 0
// (any-size slices: B H W need not be a multiple of 4)
// ------------------------------------------------------------------------------------------
// torch's clamp_(0, 1) (S6:306-308): NaN in -> NaN out.  fminf / fmaxf alone are IEEE minNum / maxNum and return the OTHER operand for a
// NaN -- a non-finite denoiser output would turn into 0 here and the loop would carry on with plausible numbers.
__device__ __forceinline__ float clamp01(float v) { return v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f); }

template <bool CNC>
__global__ __launch_bounds__(256) void k_prox(const float4* x, float4* z, float4* w, ProxParams p, size_t n4, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 xv = x[i];
        float4 zv = z[i], wv = w[i];
        if (CNC) { prox_cnc(xv.x, zv.x, wv.x, p); prox_cnc(xv.y, zv.y, wv.y, p); prox_cnc(xv.z, zv.z, wv.z, p); prox_cnc(xv.w, zv.w, wv.w, p); }
        else     { prox_l1(xv.x, zv.x, wv.x, p);  prox_l1(xv.y, zv.y, wv.y, p);  prox_l1(xv.z, zv.z, wv.z, p);  prox_l1(xv.w, zv.w, wv.w, p); }
        z[i] = zv; w[i] = wv;
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float* zs = (float*)z; float* ws = (float*)w;
        if (CNC) prox_cnc(((const float*)x)[i], zs[i], ws[i], p); else prox_l1(((const float*)x)[i], zs[i], ws[i], p);
    }
}

__global__ __launch_bounds__(256) void k_combine(const float4* z, const float4* x, const float4* w, const float4* sd,
                                                 float4* t, float c1, float c2, float c3, size_t n4, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 zv = z[i], xv = x[i], wv = w[i], sv = sd[i];
        float4 o;
        // S6:301 evaluated left to right in float32 like the reference's torch expression
        o.x = c1 * zv.x + c2 * (xv.x + wv.x) + c3 * (zv.x - sv.x);
        o.y = c1 * zv.y + c2 * (xv.y + wv.y) + c3 * (zv.y - sv.y);
        o.z = c1 * zv.z + c2 * (xv.z + wv.z) + c3 * (zv.z - sv.z);
        o.w = c1 * zv.w + c2 * (xv.w + wv.w) + c3 * (zv.w - sv.w);
        t[i] = o;
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float zv = ((const float*)z)[i], xv = ((const float*)x)[i], wv = ((const float*)w)[i], sv = ((const float*)sd)[i];
        ((float*)t)[i] = c1 * zv + c2 * (xv + wv) + c3 * (zv - sv);
    }
}

__global__ __launch_bounds__(256) void k_add(const float4* a, const float4* b, float4* o, size_t n4, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 av = a[i], bv = b[i];
        o[i] = make_float4(av.x + bv.x, av.y + bv.y, av.z + bv.z, av.w + bv.w);
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        ((float*)o)[i] = ((const float*)a)[i] + ((const float*)b)[i];
}

__global__ __launch_bounds__(256) void k_dual_clamp(float4* x, float4* z, float4* w, size_t n4, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 xv = x[i], zv = z[i], wv = w[i];
        wv.x = wv.x + xv.x - zv.x; wv.y = wv.y + xv.y - zv.y; wv.z = wv.z + xv.z - zv.z; wv.w = wv.w + xv.w - zv.w;
        x[i] = make_float4(clamp01(xv.x), clamp01(xv.y), clamp01(xv.z), clamp01(xv.w));
        z[i] = make_float4(clamp01(zv.x), clamp01(zv.y), clamp01(zv.z), clamp01(zv.w));
        w[i] = make_float4(clamp01(wv.x), clamp01(wv.y), clamp01(wv.z), clamp01(wv.w));
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float* xs = (float*)x; float* zs = (float*)z; float* ws = (float*)w;
        const float xv = xs[i], zv = zs[i];
        const float wv = ws[i] + xv - zv;
        xs[i] = clamp01(xv); zs[i] = clamp01(zv); ws[i] = clamp01(wv);
    }
}

static inline unsigned pw_grid(size_t n4) {
    size_t g = (n4 + 255) / 256;
    return (unsigned)(g < 2048 ? (g ? g : 1) : 2048);
}

// The float4 body needs every array on a 16-byte boundary; the C ABI promises only float alignment.  One pointer off that boundary:
// n4 = 0, the scalar tail loop covers [0, n) with 4-byte accesses, and the grid is sized from n (same 2048-block cap).
struct PwShape { size_t n4; unsigned grid; };
static inline PwShape pw_shape(size_t n, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* q : ptrs) bits |= (uintptr_t)q;
    if (bits & 15) return { 0, pw_grid(n) };
    return { n / 4, pw_grid(n / 4) };
}

hipError_t launch_prox(hipStream_t s, bool cnc, const float* x, float* z, float* w, ProxParams p, size_t n) {
    const PwShape g = pw_shape(n, { x, z, w });
    if (cnc) hipLaunchKernelGGL(k_prox<true>, dim3(g.grid), dim3(256), 0, s, (const float4*)x, (float4*)z, (float4*)w, p, g.n4, n);
    else     hipLaunchKernelGGL(k_prox<false>, dim3(g.grid), dim3(256), 0, s, (const float4*)x, (float4*)z, (float4*)w, p, g.n4, n);
    return hipGetLastError();
}
hipError_t launch_combine(hipStream_t s, const float* z, const float* x, const float* w, const float* sd, float* t,
                          float c1, float c2, float c3, size_t n) {
    const PwShape g = pw_shape(n, { z, x, w, sd, t });
    hipLaunchKernelGGL(k_combine, dim3(g.grid), dim3(256), 0, s, (const float4*)z, (const float4*)x,
                       (const float4*)w, (const float4*)sd, (float4*)t, c1, c2, c3, g.n4, n);
    return hipGetLastError();
}
hipError_t launch_add(hipStream_t s, const float* a, const float* b, float* o, size_t n) {
    const PwShape g = pw_shape(n, { a, b, o });
    hipLaunchKernelGGL(k_add, dim3(g.grid), dim3(256), 0, s, (const float4*)a, (const float4*)b, (float4*)o, g.n4, n);
    return hipGetLastError();
}
hipError_t launch_dual_clamp(hipStream_t s, float* x, float* z, float* w, size_t n) {
    const PwShape g = pw_shape(n, { x, z, w });
    hipLaunchKernelGGL(k_dual_clamp, dim3(g.grid), dim3(256), 0, s, (float4*)x, (float4*)z, (float4*)w, g.n4, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// metrics: per slice sum((255 x - gt)^2) and sum(gt^2) in double        (utils_image.py:543-636)
// one workgroup per slice; wave shuffle reduction then LDS across the 4 waves
// ------------------------------------------------------------------------------------------
template <typename X>
__global__ __launch_bounds__(256) void k_metrics(const X* x, const uint8_t* gt, double* acc, int N) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const X* xb = x + (size_t)b * N;
    const uint8_t* gb = gt + (size_t)b * N;
    double se = 0.0, sg = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double g = (double)gb[i];
        const double d = (double)xb[i] * 255.0 - g;
        se += d * d;
        sg += g * g;
    }
    for (int o = 32; o > 0; o >>= 1) { se += __shfl_down(se, o); sg += __shfl_down(sg, o); }
    __shared__ double s1[4], s2[4];
    if ((tid & 63) == 0) { s1[tid >> 6] = se; s2[tid >> 6] = sg; }
    __syncthreads();
    if (tid == 0) { acc[2 * b] = s1[0] + s1[1] + s1[2] + s1[3]; acc[2 * b + 1] = s2[0] + s2[1] + s2[2] + s2[3]; }
}

template <typename X>
hipError_t launch_metrics(hipStream_t s, const X* x, const uint8_t* gt, double* acc, int B, int N) {
    hipLaunchKernelGGL(k_metrics<X>, dim3(B), dim3(256), 0, s, x, gt, acc, N);
    return hipGetLastError();
}
template hipError_t launch_metrics<float>(hipStream_t, const float*, const uint8_t*, double*, int, int);
template hipError_t launch_metrics<double>(hipStream_t, const double*, const uint8_t*, double*, int, int);

// ------------------------------------------------------------------------------------------
// SSIM (utils/utils_image.py:593-615): 11-tap Gaussian (sigma 1.5) on the valid region, in double.
// One workgroup per 16x16 tile of the (H-10)x(W-10) SSIM map: 26x26 patches of img_E = 255 x and
// of the ground truth in LDS, separable filter of the five moment planes, per-tile partial sum
// (host adds the tiles: deterministic, no float atomics).
// ------------------------------------------------------------------------------------------
__constant__ double c_gauss[11];

hipError_t upload_gauss() {
    double g[11], s = 0.0;
    for (int i = 0; i < 11; ++i) { g[i] = exp(-((i - 5.0) * (i - 5.0)) / (2.0 * 1.5 * 1.5)); s += g[i]; }
    for (int i = 0; i < 11; ++i) g[i] /= s;
    return hipMemcpyToSymbol(HIP_SYMBOL(c_gauss), g, sizeof(g));
}

template <typename X>
__global__ __launch_bounds__(256) void k_ssim(const X* x, const uint8_t* gt, double* partial, int H, int W, int tiles_x, int tiles_y) {
    __shared__ double sx[26][26], sg[26][26];
    __shared__ double hp[5][26][16];
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * 16, tx0 = (blockIdx.x % tiles_x) * 16;
    const int VH = H - 10, VW = W - 10;
    const X* xb = x + (size_t)b * H * W;
    const uint8_t* gb = gt + (size_t)b * H * W;
    for (int i = tid; i < 26 * 26; i += 256) {
        const int r = i / 26, c = i % 26;
        const int yy = min(ty0 + r, H - 1), xx = min(tx0 + c, W - 1);
        sx[r][c] = (double)xb[yy * W + xx] * 255.0;
        sg[r][c] = (double)gb[yy * W + xx];
    }
    __syncthreads();
    for (int i = tid; i < 26 * 16; i += 256) {                  // horizontal pass
        const int r = i / 16, c = i % 16;
        double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const double a = sx[r][c + k], g = sg[r][c + k], wgt = c_gauss[k];
            m1 += wgt * a; m2 += wgt * g; s11 += wgt * a * a; s22 += wgt * g * g; s12 += wgt * a * g;
        }
        hp[0][r][c] = m1; hp[1][r][c] = m2; hp[2][r][c] = s11; hp[3][r][c] = s22; hp[4][r][c] = s12;
    }
    __syncthreads();
    const int r = tid >> 4, c = tid & 15;
    double v = 0.0;
    if (ty0 + r < VH && tx0 + c < VW) {
        double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const double wgt = c_gauss[k];
            m1 += wgt * hp[0][r + k][c]; m2 += wgt * hp[1][r + k][c];
            s11 += wgt * hp[2][r + k][c]; s22 += wgt * hp[3][r + k][c]; s12 += wgt * hp[4][r + k][c];
        }
        const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
        const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        v = ((2 * m12 + C1) * (2 * (s12 - m12) + C2)) / ((m11 + m22 + C1) * ((s11 - m11) + (s22 - m22) + C2));
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) partial[(size_t)b * tiles_x * tiles_y + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

template <typename X>
hipError_t launch_ssim(hipStream_t s, const X* x, const uint8_t* gt, double* partial, int B, int H, int W) {
    const int tx = (W - 10 + 15) / 16, ty = (H - 10 + 15) / 16;
    hipLaunchKernelGGL(k_ssim<X>, dim3(tx * ty, B), dim3(256), 0, s, x, gt, partial, H, W, tx, ty);
    return hipGetLastError();
}
template hipError_t launch_ssim<float>(hipStream_t, const float*, const uint8_t*, double*, int, int, int);
template hipError_t launch_ssim<double>(hipStream_t, const double*, const uint8_t*, double*, int, int, int);

// float -> double widening of the image handed to the double-precision synthesis (exact)
__global__ __launch_bounds__(256) void k_widen(const float4* in, double4* out, size_t n4, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = in[i];
        out[i] = make_double4((double)v.x, (double)v.y, (double)v.z, (double)v.w);
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        ((double*)out)[i] = (double)((const float*)in)[i];
}
hipError_t launch_widen(hipStream_t s, const float* in, double* out, size_t n) {
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(k_widen, dim3(pw_grid(n4)), dim3(256), 0, s, (const float4*)in, (double4*)out, n4, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Calibration (pnp_calibrate_stream, include/pnp_mri.h): the slice-resident kernel's ACCESS SHAPE without its arithmetic (profiles/micro/
// slice_stride.hip, round 3, moved into the library in round 6 so that bench.py can print what THIS card's memory system gives such a
// kernel next to the kernel's own rate).  One 512-thread workgroup per 256-KiB slice; per pass: read z, w and a table, write z, w back in
// place, 16 bytes per lane, eight accesses of each array in flight per wave.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_calibrate_stream(float4* z, float4* w, const float4* y, int passes) {
    const size_t base = (size_t)blockIdx.x * 16384;
    float4* zs = z + base;
    float4* ws = w + base;
    const float4* ys = y + base;
    const int tid = threadIdx.x;
    for (int it = 0; it < passes; ++it)
        for (int g = 0; g < 4; ++g) {
            float4 a[8], b[8], c[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int i = tid + 512 * (8 * g + u); a[u] = zs[i]; b[u] = ws[i]; c[u] = ys[i]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = tid + 512 * (8 * g + u);
                zs[i] = make_float4(a[u].x + c[u].x * 1e-9f, a[u].y + c[u].y * 1e-9f, a[u].z + c[u].z * 1e-9f, a[u].w + c[u].w * 1e-9f);
                ws[i] = make_float4(b[u].x - c[u].x * 1e-9f, b[u].y - c[u].y * 1e-9f, b[u].z - c[u].z * 1e-9f, b[u].w - c[u].w * 1e-9f);
            }
        }
}

hipError_t launch_calibrate_stream(hipStream_t s, float* z, float* w, const float* y, int slices, int passes) {
    hipLaunchKernelGGL(k_calibrate_stream, dim3((unsigned)slices), dim3(512), 0, s, reinterpret_cast<float4*>(z), reinterpret_cast<float4*>(w),
                       reinterpret_cast<const float4*>(y), passes);
    return hipGetLastError();
}

}  // namespace pnp
