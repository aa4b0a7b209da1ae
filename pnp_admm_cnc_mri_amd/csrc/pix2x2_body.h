// DRUNet's scale changes, the ONE kernel body behind kernels_pix2x2_f16x3.hip (k_pix2x2_h3) and kernels_pix2x2_f16.hip
// (k_pix2x2_f16):
//
//     down   torch.nn.Conv2d(C, 2C, 2, 2, 0, bias=False)            models/network_unet.py:95-99,  models/basicblock.py:415-421
//     up     torch.nn.ConvTranspose2d(C, C/2, 2, 2, 0, bias=False)  models/network_unet.py:103-107, models/basicblock.py:439-445
//
// Neither has a halo: both are plain matrix products over pixels,
//     down   y[(oy, ox)][co]               = sum_{dy, dx, ci} x[(2 oy + dy, 2 ox + dx)][ci] W[co][ci][dy][dx]      K = 4 C,  N = 2 C
//     up     y[(2 iy + dy, 2 ix + dx)][co] = sum_ci x[(iy, ix)][ci] W[ci][co][dy][dx]                              K = C,    N = 4 (C / 2)
// so one kernel serves the two: a workgroup item is 8 x 16 pixels of the TILE GRID (output pixels for `down`, input pixels for `up`) x
// one block of 64 matrix columns; its K loop runs over chunks of 64 input channels.  Per chunk the 128 pixels x 64 channels of A are
// loaded two chunks ahead into registers and put into LDS in the family's operand layout (an operand fragment is one ds_read_b128), the
// chunk's 64 x 64 weights arrive packed by LDS-DMA into the other of two buffers.  Unlike the 3 x 3 kernels every chunk brings a new A
// tile: two barriers per chunk, and the big instances (64 <-> 128 channels at full resolution) are bound by their memory traffic, not
// by the matrix pipe -- which is all this kernel has to reach: the six layers are 2.3 % of DRUNet's arithmetic and were 8 % of its time
// on MIOpen.
// `x2`: an optional second input ADDED to x while staging -- the U-Net's skip additions `m_up(x + x_skip)` (models/network_unet.py:
// 131-133) ride on the transposed convolution that consumes the sum; the sum itself never goes to memory.
//
// The arithmetic family is a POLICY (Pix2H3, Pix2F16 below): the element type of the loads, how a chunk goes from registers into LDS,
// the MFMA block, the value staged from the accumulators and the store.  Control flow, waits and barriers are the body's alone.
#pragma once
#include "f16_common.h"

namespace pnp {

struct Pix2Args {
    const void* x;       // [n][Hin][Win][Cin]
    const void* x2;      // null, or a tensor of x's shape added to it
    const void* w;       // packed: blocks [cb][kc] of P::WBLK bytes (pix2_pack_w_body)
    void* y;             // [n][Hout][Wout][Cout]
    int n, Hin, Win, Cin, Hout, Wout, Cout;
    int GH, GW, tiles_x, tiles_y;      // the tile grid (down: Hout x Wout; up: Hin x Win) and its 8 x 16 tiling
    int KC, NB;                         // chunks of 64 along K, blocks of 64 matrix columns
    int y32;                            // f16: y is float32, the accumulator result without the final rounding
};
constexpr int P2_ROWS = CP_PIX2.ty, P2_COLS = CP_PIX2.tx;      // the tile (conv_plan.h)
constexpr int P2_TILE = 4 * 32 * H3_STR * 4;                    // bytes: the epilogue's staging area (4 waves x 32 pixels x H3_STR floats); the A tile lies inside

// split halves (f16x3_common.h): float32 in and out, a value is hi + lo / 2048, three products per MFMA step.  A pixel of the A tile is
// [64 hi][64 lo] + 16 bytes, a block of weights [K step 2][N tile 4][hi, lo][lane 64] x 16 bytes
struct Pix2H3 {
    static constexpr int ELT = 4, PS = CV_PS * 4, WBLK = H3_TAP16 * 16;      // bytes: element of x / x2, pixel of the A tile, block of weights
    struct Acc { f32x4 mainv[2][4], corrv[2][4]; };
    template <bool X2>
    static __device__ __forceinline__ void put(char* px, const u32x4v& a, const u32x4v& b) {
        h4 hi, lo;
        split4(X2 ? as_f32x4(a) + as_f32x4(b) : as_f32x4(a), hi, lo);
        *reinterpret_cast<h4*>(px) = hi;
        *reinterpret_cast<h4*>(px + 128) = lo;
    }
    static __device__ __forceinline__ void mma(Acc& c, const char* a0, const char* bp) {      // 48 v_mfma_f32_16x16x32_f16: 2 K steps x 2 M tiles x 4 N tiles x 3
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            h8 ah[2], al[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                ah[mt] = *reinterpret_cast<const h8*>(a0 + mt * (P2_COLS * PS) + 64 * s2);
                al[mt] = *reinterpret_cast<const h8*>(a0 + mt * (P2_COLS * PS) + 64 * s2 + 128);
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const h8 bh = *reinterpret_cast<const h8*>(bp + 1024 * ((s2 * 4 + nt) * 2));
                const h8 bl = *reinterpret_cast<const h8*>(bp + 1024 * ((s2 * 4 + nt) * 2 + 1));
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    c.mainv[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], bh, c.mainv[mt][nt], 0, 0, 0);
                    c.corrv[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], bl, c.corrv[mt][nt], 0, 0, 0);
                    c.corrv[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mt], bh, c.corrv[mt][nt], 0, 0, 0);
                }
            }
        }
    }
    static __device__ __forceinline__ float value(const Acc& c, int mt, int nt, int r) { return fmaf(c.corrv[mt][nt][r], H3_RSCALE, c.mainv[mt][nt][r]); }
    static __device__ __forceinline__ int out_elt(int) { return 4; }
    // the lane's 16 / ELT channels of one pixel: `sp` in the staging area -> y at byte `off` (out of range for a pixel outside the grid: dropped)
    static __device__ __forceinline__ void store(const __amdgpu_buffer_rsrc_t& ry, int off, bool, const float* sp, int) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(sp);
        const u32x4v o = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
        __builtin_amdgcn_raw_buffer_store_b128(o, ry, off, 0, 0);
    }
};

// halves (f16_common.h): half in, half (or float32: y32) out, one product per MFMA step, results rounded once on store.  A pixel of the A
// tile is 128 bytes of halves + 32, a block of weights [K step 2][N tile 4][lane 64] x 16 bytes
struct Pix2F16 {
    static constexpr int ELT = 2, PS = HF_PS, WBLK = HF_TAP16 * 16;
    struct Acc { f32x4 acc[2][4]; };
    template <bool X2>
    static __device__ __forceinline__ void put(char* px, const u32x4v& a, const u32x4v& b) {
        u32x4v v = a;
        if (X2) {                                                 // the sum is formed in float32 and rounded to half once, as the operand
            const h8 p = __builtin_bit_cast(h8, a), r = __builtin_bit_cast(h8, b);
            h8 s;
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] = (_Float16)((float)p[e] + (float)r[e]);
            v = __builtin_bit_cast(u32x4v, s);
        }
        *reinterpret_cast<u32x4v*>(px) = v;
    }
    static __device__ __forceinline__ void mma(Acc& c, const char* a0, const char* bp) {      // 16 v_mfma_f32_16x16x32_f16: 2 K steps x 2 M tiles x 4 N tiles
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            h8 af[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) af[mt] = *reinterpret_cast<const h8*>(a0 + mt * (P2_COLS * PS) + 64 * s2);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const h8 bf = *reinterpret_cast<const h8*>(bp + 1024 * (s2 * 4 + nt));
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) c.acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf, c.acc[mt][nt], 0, 0, 0);
            }
        }
    }
    static __device__ __forceinline__ float value(const Acc& c, int mt, int nt, int r) { return c.acc[mt][nt][r]; }
    static __device__ __forceinline__ int out_elt(int y32) { return y32 ? 4 : 2; }
    static __device__ __forceinline__ void store(const __amdgpu_buffer_rsrc_t& ry, int off, bool in, const float* sp, int y32) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(sp), v1 = *reinterpret_cast<const f32x4*>(sp + 4);
        if (y32) {                                                // uniform
            const u32x4v o0 = {__float_as_uint(v0[0]), __float_as_uint(v0[1]), __float_as_uint(v0[2]), __float_as_uint(v0[3])};
            const u32x4v o1 = {__float_as_uint(v1[0]), __float_as_uint(v1[1]), __float_as_uint(v1[2]), __float_as_uint(v1[3])};
            __builtin_amdgcn_raw_buffer_store_b128(o0, ry, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(o1, ry, in ? off + 16 : -16, 0, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, round8(v0, v1)), ry, off, 0, 0);
        }
    }
};

template <class P, bool UP, bool X2>
__device__ __forceinline__ void pix2x2_body(const Pix2Args& a, int nitems) {
    constexpr int CPV = 16 / P::ELT;                             // channels in 16 bytes of x: one load, and one lane's share of a pixel in the epilogue
    constexpr int NQ = 64 / CPV;                                 // threads across a chunk's 64 channels
    constexpr int RS = CV_THREADS / (NQ * P2_COLS), U = P2_ROWS / RS;      // a thread stages tile rows sr + RS u, u < U (f16x3: 8 loads of row u; f16: 4 of rows sr + 2 u)
    constexpr int NDMA = P::WBLK / (CV_THREADS * 16);
    static_assert(P2_ROWS * P2_COLS * P::PS <= P2_TILE, "the A tile must fit the staging area");
    __shared__ __attribute__((aligned(16))) char lds[P2_TILE + 2 * P::WBLK];      // one array: A tile, then the two weight buffers
    char* const xin = lds;
    char* const wbuf = lds + P2_TILE;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kb = lane >> 4;
    const int NB = a.NB, KC = a.KC, ncc = a.Cin >> 6;
    int item = blockIdx.x;
    if (item >= nitems) return;
    const int cb = item % NB;                                   // gridDim.x is a multiple of NB: a workgroup keeps its block of columns
    const int esz = P::out_elt(a.y32), pixA = a.Cin * P::ELT, pixO = a.Cout * esz;
    const int per_img = a.tiles_x * a.tiles_y;
    // staging role of this thread: tile column sc, channels CPV sq .. of the chunk, tile rows sr + RS u
    const int sq = tid % NQ, sc = (tid / NQ) % P2_COLS, sr = tid / (NQ * P2_COLS);

    // A is requested TWO chunks ahead (a chunk's MFMAs are a fraction of a us, a memory round trip under load several times that): two
    // register sets, chunk kc lives in set kc & 1 (KC is even).  The second tensor (X2) has ONE set, requested one chunk ahead: its
    // values must stay apart from x's until the operand is formed (an addition at load time would wait for the loads on the spot), and
    // two more sets do not fit 256 registers.  `any` = false: a descriptor of zero bytes -- the loads are still ISSUED (the counted wait
    // below relies on their number) but reach no memory.
    u32x4v areg[2][U], breg[X2 ? U : 1];
    auto load_t = [&](const void* base, u32x4v* dst, int it_, int kc_, const bool any) __attribute__((always_inline)) {
        const int t = it_ / NB, img = t / per_img, trem = t - img * per_img, ty = trem / a.tiles_x;
        const int gy0 = ty * P2_ROWS + sr, gx = (trem - ty * a.tiles_x) * P2_COLS + sc;
        int dy = 0, dx = 0, cc = kc_;
        if (!UP) { const int q = kc_ / ncc; cc = kc_ - q * ncc; dy = q >> 1; dx = q & 1; }
        const unsigned bytes = any ? (unsigned)a.Hin * (unsigned)a.Win * (unsigned)pixA : 0u;
        const __amdgpu_buffer_rsrc_t rs = bytes_rsrc(base, (size_t)img * a.Hin * a.Win * pixA, bytes);
        const int ix = UP ? gx : 2 * gx + dx;
        const int col_off = ix * pixA + (64 * cc + CPV * sq) * P::ELT;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int gy = gy0 + RS * u, iy = UP ? gy : 2 * gy + dy;
            const int off = (gy < a.GH && gx < a.GW) ? iy * a.Win * pixA + col_off : -16;     // outside the grid: out of range, zeros
            dst[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
    };
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, NB * KC * P::WBLK, 0x00020000);
    const int wvoff = tid * 16;
    auto dma_w = [&](int buf, int kc_) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NDMA; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(wbuf + buf * P::WBLK + (wv * 64 + 256 * j) * 16), 16, wvoff,
                                                     (cb * KC + kc_) * P::WBLK + j * 4096, 0, 0);
    };

    load_t(a.x, areg[0], item, 0, true);
    if (X2) load_t(a.x2, breg, item, 0, true);
    dma_w(0, 0);
    load_t(a.x, areg[1], item, 1, true);                         // KC >= 2
    int par = 0;
    const char* const a0 = xin + (2 * wv * P2_COLS + i) * P::PS + kb * 16;
#pragma unroll 1
    for (; item < nitems; item += gridDim.x) {
        typename P::Acc acc = {};
        auto chunk = [&](const int kc, u32x4v (&areg)[U]) __attribute__((always_inline)) {
            // (1) this wave's share of the chunk's weights and its A registers have landed -- everything but the U loads of x for the
            //     chunk after this one, which were issued BEHIND this chunk's weight DMA (in-order completion; the order is pinned by the
            //     sched_barrier below and checked in the ISA by tools/isa_scan.py); every wave's reads of the A tile and of the other
            //     weight buffer for the chunk before have RETURNED (lgkmcnt(0): a raw s_barrier waits for no counter, and the
            //     sched_barrier behind the MFMA block keeps those reads and MFMAs in their chunk -- without the two, hipcc moved 12 of a
            //     chunk's 16 MFMAs and their reads behind this barrier, where other waves already overwrite the tile)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(U) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            {
                char* px = xin + (sr * P2_COLS + sc) * P::PS + 2 * CPV * sq;
#pragma unroll
                for (int u = 0; u < U; ++u) P::template put<X2>(px + u * (RS * P2_COLS * P::PS), areg[u], breg[X2 ? u : 0]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                          // (2) the A tile is complete
            asm volatile("" ::: "memory");
            // requests, in this order: x2 of the chunk after this one; its weights; then (behind them) x of the chunk after that -- of
            // this item or of the workgroup's next one
            const bool more = item + (int)gridDim.x < nitems;
            const bool last = kc + 1 == KC, last2 = kc + 2 >= KC;
            __builtin_amdgcn_sched_barrier(0);
            if (X2) load_t(a.x2, breg, last ? (more ? item + gridDim.x : item) : item, last ? 0 : kc + 1, !last || more);
            __builtin_amdgcn_sched_barrier(0);
            if (!last || more) dma_w(par ^ 1, last ? 0 : kc + 1);
            __builtin_amdgcn_sched_barrier(0);
            load_t(a.x, areg, last2 ? (more ? item + gridDim.x : item) : item, last2 ? kc + 2 - KC : kc + 2, !last2 || more);
            __builtin_amdgcn_sched_barrier(0);
            P::mma(acc, a0, wbuf + par * P::WBLK + lane * 16);
            __builtin_amdgcn_sched_barrier(0);                     // the chunk's LDS reads and MFMAs stay in front of the next chunk's barrier
            par ^= 1;
        };
#pragma unroll 1
        for (int kc = 0; kc < KC; kc += 2) {
            chunk(kc, areg[0]);
            chunk(kc + 1, areg[1]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                              // every wave is done with the A tile: it becomes the staging area
        asm volatile("" ::: "memory");
        // accumulator (reg r, lane (i, kb)) of tile (mt, nt) = pixel (tile row 2 w + mt, column 4 kb + r), column 16 nt + i of the block
        float* stage = reinterpret_cast<float*>(xin) + wv * (32 * H3_STR);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    stage[(16 * mt + 4 * kb + r) * H3_STR + 16 * nt + i] = P::value(acc, mt, nt, r);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            const int t = item / NB, img = t / per_img, trem = t - img * per_img, ty = trem / a.tiles_x;
            const int gy0 = ty * P2_ROWS + 2 * wv, gx0 = (trem - ty * a.tiles_x) * P2_COLS;
            int dy = 0, dx = 0, co0 = 64 * cb;
            if (UP) { const int nco = a.Cout >> 6, q = cb / nco; co0 = 64 * (cb - q * nco); dy = q >> 1; dx = q & 1; }
            const __amdgpu_buffer_rsrc_t ry = bytes_rsrc(a.y, (size_t)img * a.Hout * a.Wout * pixO, (unsigned)a.Hout * (unsigned)a.Wout * (unsigned)pixO);
            // a lane takes CPV consecutive channels (group lane % NQ) of pixel slot lane / NQ, 32 / CPV times: staged row m = CPV it + slot
            const int ps = lane / NQ, co = lane % NQ;
#pragma unroll
            for (int it = 0; it < 32 / CPV; ++it) {
                const int m = CPV * it + ps, gy = gy0 + (m >> 4), gx = gx0 + (m & 15);
                const int oy = UP ? 2 * gy + dy : gy, ox = UP ? 2 * gx + dx : gx;
                const bool in = gy < a.GH && gx < a.GW;
                const int off = in ? (oy * a.Wout + ox) * pixO + (co0 + CPV * co) * esz : -32;      // outside: dropped
                P::store(ry, off, in, stage + m * H3_STR + CPV * co, a.y32);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // no wave ends with an LDS-DMA in flight
}

// torch weights -> fragment order, blocks [cb][kc] (the conv kernels' block format, frag_write in f16x3_common.h): value j of lane
// (n, kb) of fragment (K step s, N tile nt) of block (cb, kc) is M[k = 64 kc + 32 s + 8 kb + j][column 64 cb + 16 nt + n] with
//     down  M[(2 dy + dx) C + ci][co]              = W[co][ci][dy][dx]      (Conv2d weight [2C][C][2][2])
//     up    M[ci][(2 dy + dx) (C / 2) + co]        = W[ci][co][dy][dx]      (ConvTranspose2d weight [C][C/2][2][2])
template <bool SPLIT>
__device__ __forceinline__ void pix2_pack_w_body(const float* w, _Float16* wfrag, int C, int up) {
    const int K = up ? C : 4 * C, N = 2 * C, KC = K >> 6;
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;      // one value per thread
    if (o >= (long long)K * N) return;
    const FragPos p = frag_pos(o);                                      // blk = cb * KC + kc
    const int kc = (int)(p.blk % KC), cb = (int)(p.blk / KC);
    const int k = 64 * kc + 32 * p.s + 8 * (p.lane >> 4) + p.j, col = 64 * cb + 16 * p.nt + (p.lane & 15);
    float v;
    if (up) {
        const int half = C >> 1, q = col / half, co = col - q * half;
        v = w[(((size_t)k * half + co) * 2 + (q >> 1)) * 2 + (q & 1)];
    } else {
        const int q = k / C, ci = k - q * C;
        v = w[(((size_t)col * C + ci) * 2 + (q >> 1)) * 2 + (q & 1)];
    }
    frag_write<SPLIT>(wfrag, o, p, v);
}

// kern[up][x2]: the unit's four instances of its named kernel
static hipError_t launch_pix2(hipStream_t s, void (*const (&kern)[2][2])(Pix2Args, int), const void* x, const void* x2, const void* w, void* y,
                              int n, int C, int H, int W, int up, int y_f32) {
    if (cp_check_pix2(n, C, H, W, up != 0)) return hipErrorInvalidValue;
    const Pix2Plan p = cp_pix2_plan(n, C, H, W, up != 0);
    Pix2Args a;
    a.x = x; a.x2 = x2; a.w = w; a.y = y; a.n = n; a.Hin = H; a.Win = W; a.Cin = C;
    a.Hout = p.Hout; a.Wout = p.Wout; a.Cout = p.Cout; a.GH = p.GH; a.GW = p.GW;
    a.tiles_x = p.t.tiles_x; a.tiles_y = p.t.tiles_y; a.KC = p.KC; a.NB = p.NB; a.y32 = y_f32 ? 1 : 0;
    const long long items = p.t.items;
    const int cus = conv_compute_units();
    if (cus <= 0) return hipGetLastError();
    const long long grid = cp_grid(items, 2, cus, p.NB);         // persistent workgroups, two per compute unit, a multiple of NB of them
    hipLaunchKernelGGL(kern[up != 0][x2 != nullptr], dim3((unsigned)grid), dim3(CV_THREADS), 0, s, a, (int)items);
    return hipGetLastError();
}

static hipError_t launch_pix2_pack(hipStream_t s, void (*kern)(const float*, _Float16*, int, int), const float* w, void* wfrag, int C, int up) {
    if (cp_check_pack2(C, up != 0)) return hipErrorInvalidValue;
    const long long n = (long long)(up ? C : 4 * C) * 2 * C;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, reinterpret_cast<_Float16*>(wfrag), C, up);
    return hipGetLastError();
}

}  // namespace pnp
