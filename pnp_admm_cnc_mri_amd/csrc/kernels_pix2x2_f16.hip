// DRUNet's scale changes in the half-precision ("f16") arithmetic of kernels_conv_f16.hip:
//
//     down   torch.nn.Conv2d(C, 2C, 2, 2, 0, bias=False)            models/network_unet.py:95-99,  models/basicblock.py:415-421
//     up     torch.nn.ConvTranspose2d(C, C/2, 2, 2, 0, bias=False)  models/network_unet.py:103-107, models/basicblock.py:439-445
//
// The structure is kernels_pix2x2_f16x3.hip's -- both layers are plain matrix products over pixels, one kernel serves the two: an item is
// 8 x 16 pixels of the tile grid (output pixels for `down`, input pixels for `up`) x one block of 64 matrix columns, its K loop runs over
// chunks of 64 input channels; the 128 pixels x 64 channels of A are loaded two chunks ahead into registers and copied into LDS, the
// chunk's 64 x 64 weights arrive by LDS-DMA into the other of two 8 KiB buffers -- with halves in and out: four 16-byte loads per thread
// and chunk instead of eight, nothing to split, 16 v_mfma_f32_16x16x32_f16 per wave and chunk instead of 48, results rounded once on store.
// `x2`: an optional second half tensor ADDED to x while staging (the U-Net's skip sums `m_up(x + x_skip)`): the sum is formed in float32
// and rounded to half once, as the operand; it never goes to memory.
#include "f16_common.h"

namespace pnp {

struct Pix2F16Args {
    const void* x;       // [n][Hin][Win][Cin] halves
    const void* x2;      // null, or a tensor of x's shape added to it
    const void* w;       // packed halves: blocks [cb][kc] of 8 KiB (k_pix2_pack_w_f16)
    void* y;             // [n][Hout][Wout][Cout] halves (float32 with y32: the accumulator result without the final rounding)
    int n, Hin, Win, Cin, Hout, Wout, Cout;
    int GH, GW, tiles_x, tiles_y;      // the tile grid (down: Hout x Wout; up: Hin x Win) and its 8 x 16 tiling
    int KC, NB;                         // chunks of 64 along K, blocks of 64 matrix columns
    int y32;
};
constexpr int P2F_ROWS = CP_PIX2.ty, P2F_COLS = CP_PIX2.tx, P2F_U = 4;     // the tile (conv_plan.h); 16-byte chunks of the A tile per thread
constexpr int P2F_TILE = 4 * 32 * H3_STR * 4;                     // bytes: the A tile (128 x 160) lies inside the epilogue's staging area (128 x 68 floats)
static_assert(P2F_ROWS * P2F_COLS * HF_PS <= P2F_TILE, "the A tile must fit the staging area");

template <bool UP, bool X2>
__global__ __launch_bounds__(CV_THREADS, 2) void k_pix2x2_f16(Pix2F16Args a, int nitems) {
    __shared__ __attribute__((aligned(16))) char lds[P2F_TILE + 2 * HF_TAP16 * 16];      // one array: A tile, then the two weight buffers
    char* const xin = lds;
    u32x4v (*const wbuf)[HF_TAP16] = reinterpret_cast<u32x4v (*)[HF_TAP16]>(lds + P2F_TILE);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kb = lane >> 4;
    const int NB = a.NB, KC = a.KC, ncc = a.Cin >> 6;
    int item = blockIdx.x;
    if (item >= nitems) return;
    const int cb = item % NB;                                   // gridDim.x is a multiple of NB: a workgroup keeps its block of columns
    const int pixA = a.Cin * 2, esz = a.y32 ? 4 : 2, pixO = a.Cout * esz;
    const int per_img = a.tiles_x * a.tiles_y;
    // staging role of this thread: tile column sc, channels 8 sq .. of the chunk, tile rows sr + 2 u
    const int sq = tid & 7, sc = (tid >> 3) & 15, sr = tid >> 7;

    // A is requested TWO chunks ahead: two register sets, chunk kc lives in set kc & 1 (KC is even).  The second tensor (X2) has ONE set,
    // requested one chunk ahead.  `any` = false: a descriptor of zero bytes -- the loads are still ISSUED (the counted wait below relies
    // on their number) but reach no memory.
    u32x4v areg[2][P2F_U], breg[X2 ? P2F_U : 1];
    auto load_t = [&](const void* base, u32x4v* dst, int it_, int kc_, const bool any) __attribute__((always_inline)) {
        const int t = it_ / NB, img = t / per_img, trem = t - img * per_img, ty = trem / a.tiles_x;
        const int gy0 = ty * P2F_ROWS + sr, gx = (trem - ty * a.tiles_x) * P2F_COLS + sc;
        int dy = 0, dx = 0, cc = kc_;
        if (!UP) { const int q = kc_ / ncc; cc = kc_ - q * ncc; dy = q >> 1; dx = q & 1; }
        const unsigned bytes = any ? (unsigned)a.Hin * (unsigned)a.Win * (unsigned)pixA : 0u;
        const __amdgpu_buffer_rsrc_t rs = bytes_rsrc(base, (size_t)img * a.Hin * a.Win * pixA, bytes);
        const int ix = UP ? gx : 2 * gx + dx;
        const int col_off = ix * pixA + (64 * cc + 8 * sq) * 2;
#pragma unroll
        for (int u = 0; u < P2F_U; ++u) {
            const int gy = gy0 + 2 * u, iy = UP ? gy : 2 * gy + dy;
            const int off = (gy < a.GH && gx < a.GW) ? iy * a.Win * pixA + col_off : -16;     // outside the grid: out of range, zeros
            dst[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
    };
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, NB * KC * (HF_TAP16 * 16), 0x00020000);
    const int wvoff = tid * 16;
    auto dma_w = [&](int buf, int kc_) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(&wbuf[buf][wv * 64 + 256 * j]), 16, wvoff,
                                                     (cb * KC + kc_) * (HF_TAP16 * 16) + j * 4096, 0, 0);
    };

    load_t(a.x, areg[0], item, 0, true);
    if (X2) load_t(a.x2, breg, item, 0, true);
    dma_w(0, 0);
    load_t(a.x, areg[1], item, 1, true);                         // KC >= 2
    int par = 0;
    const char* const a0 = xin + (2 * wv * P2F_COLS + i) * HF_PS + kb * 16;
#pragma unroll 1
    for (; item < nitems; item += gridDim.x) {
        f32x4 acc[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto chunk = [&](const int kc, u32x4v (&areg)[P2F_U]) __attribute__((always_inline)) {
            // (1) this wave's share of the chunk's weights and its A registers have landed -- everything but the P2F_U loads of x for the
            //     chunk after this one, which were issued BEHIND this chunk's weight DMA (in-order completion; the order is pinned by the
            //     sched_barrier below and checked in the ISA by tests/test_conv_f16_cpu.py); every wave's reads of the A tile and of the
            //     other weight buffer for the chunk before have RETURNED (lgkmcnt(0): a raw s_barrier waits for no counter, and the
            //     sched_barrier behind the MFMA block keeps those reads and MFMAs in their chunk -- without the two, hipcc moved 12 of a
            //     chunk's 16 MFMAs and their reads behind this barrier, where other waves already overwrite the tile)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(P2F_U) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            {
                char* px = xin + (sr * P2F_COLS + sc) * HF_PS + 16 * sq;
#pragma unroll
                for (int u = 0; u < P2F_U; ++u) {
                    u32x4v v = areg[u];
                    if (X2) {
                        const h8 p = __builtin_bit_cast(h8, areg[u]), r = __builtin_bit_cast(h8, breg[X2 ? u : 0]);
                        h8 s;
#pragma unroll
                        for (int e = 0; e < 8; ++e) s[e] = (_Float16)((float)p[e] + (float)r[e]);
                        v = __builtin_bit_cast(u32x4v, s);
                    }
                    *reinterpret_cast<u32x4v*>(px + u * (2 * P2F_COLS * HF_PS)) = v;
                }
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
            const char* bp = reinterpret_cast<const char*>(&wbuf[par][0]) + lane * 16;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                h8 af[2];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) af[mt] = *reinterpret_cast<const h8*>(a0 + mt * (P2F_COLS * HF_PS) + 64 * s2);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const h8 bf = *reinterpret_cast<const h8*>(bp + 1024 * (s2 * 4 + nt));
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf, acc[mt][nt], 0, 0, 0);
                }
            }
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
                    stage[(16 * mt + 4 * kb + r) * H3_STR + 16 * nt + i] = acc[mt][nt][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            const int t = item / NB, img = t / per_img, trem = t - img * per_img, ty = trem / a.tiles_x;
            const int gy0 = ty * P2F_ROWS + 2 * wv, gx0 = (trem - ty * a.tiles_x) * P2F_COLS;
            int dy = 0, dx = 0, co0 = 64 * cb;
            if (UP) { const int nco = a.Cout >> 6, q = cb / nco; co0 = 64 * (cb - q * nco); dy = q >> 1; dx = q & 1; }
            const __amdgpu_buffer_rsrc_t ry = bytes_rsrc(a.y, (size_t)img * a.Hout * a.Wout * pixO, (unsigned)a.Hout * (unsigned)a.Wout * (unsigned)pixO);
            // a lane takes eight consecutive channels (octet lane & 7) of pixel slot lane >> 3, four times: 16 bytes of halves (32 of float32)
            const int ps = lane >> 3, co = lane & 7;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int m = 8 * it + ps, gy = gy0 + (m >> 4), gx = gx0 + (m & 15);
                const int oy = UP ? 2 * gy + dy : gy, ox = UP ? 2 * gx + dx : gx;
                const bool in = gy < a.GH && gx < a.GW;
                const int off = in ? (oy * a.Wout + ox) * pixO + (co0 + 8 * co) * esz : -32;      // outside: dropped
                const float* sp = stage + m * H3_STR + 8 * co;
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(sp), v1 = *reinterpret_cast<const f32x4*>(sp + 4);
                if (a.y32) {                                       // uniform
                    const u32x4v o0 = {__float_as_uint(v0[0]), __float_as_uint(v0[1]), __float_as_uint(v0[2]), __float_as_uint(v0[3])};
                    const u32x4v o1 = {__float_as_uint(v1[0]), __float_as_uint(v1[1]), __float_as_uint(v1[2]), __float_as_uint(v1[3])};
                    __builtin_amdgcn_raw_buffer_store_b128(o0, ry, off, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(o1, ry, in ? off + 16 : -16, 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, round8(v0, v1)), ry, off, 0, 0);
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // no wave ends with an LDS-DMA in flight
}

// torch weights -> halves (round to nearest even) in fragment order, blocks [cb][kc] of 8 KiB: half j of lane (n, kb) of fragment
// (K step s, N tile nt) of block (cb, kc) is half(M[k = 64 kc + 32 s + 8 kb + j][column 64 cb + 16 nt + n]) with
//     down  M[(2 dy + dx) C + ci][co]              = W[co][ci][dy][dx]      (Conv2d weight [2C][C][2][2])
//     up    M[ci][(2 dy + dx) (C / 2) + co]        = W[ci][co][dy][dx]      (ConvTranspose2d weight [C][C/2][2][2])
__global__ __launch_bounds__(256) void k_pix2_pack_w_f16(const float* w, _Float16* wfrag, int C, int up) {
    const int K = up ? C : 4 * C, N = 2 * C, KC = K >> 6;
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;      // one half per thread
    if (o >= (long long)K * N) return;
    const int j = o & 7, lane = (o >> 3) & 63, nt = (o >> 9) & 3, s = (o >> 11) & 1;
    const long long blk = o >> 12;                                      // cb * KC + kc
    const int kc = (int)(blk % KC), cb = (int)(blk / KC);
    const int k = 64 * kc + 32 * s + 8 * (lane >> 4) + j, col = 64 * cb + 16 * nt + (lane & 15);
    float v;
    if (up) {
        const int half = C >> 1, q = col / half, co = col - q * half;
        v = w[(((size_t)k * half + co) * 2 + (q >> 1)) * 2 + (q & 1)];
    } else {
        const int q = k / C, ci = k - q * C;
        v = w[(((size_t)col * C + ci) * 2 + (q >> 1)) * 2 + (q & 1)];
    }
    wfrag[o] = (_Float16)v;
}

hipError_t launch_pix2x2_f16(hipStream_t s, const void* x, const void* x2, const void* w, void* y, int n, int C, int H, int W, int up, int y_f32) {
    if (cp_check_pix2(n, C, H, W, up != 0)) return hipErrorInvalidValue;
    const Pix2Plan p = cp_pix2_plan(n, C, H, W, up != 0);
    Pix2F16Args a;
    a.x = x; a.x2 = x2; a.w = w; a.y = y; a.n = n; a.Hin = H; a.Win = W; a.Cin = C;
    a.Hout = p.Hout; a.Wout = p.Wout; a.Cout = p.Cout; a.GH = p.GH; a.GW = p.GW;
    a.tiles_x = p.t.tiles_x; a.tiles_y = p.t.tiles_y; a.KC = p.KC; a.NB = p.NB; a.y32 = y_f32 ? 1 : 0;
    const long long items = p.t.items;
    const int cus = conv_compute_units();
    if (cus <= 0) return hipGetLastError();
    const long long grid = cp_grid(items, 2, cus, p.NB);         // persistent workgroups, two per compute unit, a multiple of NB of them
    if (up && x2)       hipLaunchKernelGGL((k_pix2x2_f16<true, true>), dim3((unsigned)grid), dim3(CV_THREADS), 0, s, a, (int)items);
    else if (up)        hipLaunchKernelGGL((k_pix2x2_f16<true, false>), dim3((unsigned)grid), dim3(CV_THREADS), 0, s, a, (int)items);
    else if (x2)        hipLaunchKernelGGL((k_pix2x2_f16<false, true>), dim3((unsigned)grid), dim3(CV_THREADS), 0, s, a, (int)items);
    else                hipLaunchKernelGGL((k_pix2x2_f16<false, false>), dim3((unsigned)grid), dim3(CV_THREADS), 0, s, a, (int)items);
    return hipGetLastError();
}

hipError_t launch_pix2_pack_w_f16(hipStream_t s, const float* w, void* wfrag, int C, int up) {
    if (cp_check_pack2(C, up != 0)) return hipErrorInvalidValue;
    const long long n = (long long)(up ? C : 4 * C) * 2 * C;
    hipLaunchKernelGGL(k_pix2_pack_w_f16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, reinterpret_cast<_Float16*>(wfrag), C, up);
    return hipGetLastError();
}

}  // namespace pnp
