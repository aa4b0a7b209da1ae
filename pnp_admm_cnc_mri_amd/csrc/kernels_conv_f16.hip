// The denoisers' convolution layers in HALF precision on the f16 matrix cores: "f16".  DESIGN.md 4.12.
//
// The f16x3 kernels (kernels_conv_f16x3.hip) spend three v_mfma_f32_16x16x32_f16 per float32 product and carry every activation as a
// hi / lo pair, 256 bytes per pixel and 64 channels.  Here activations between layers ARE halves (NHWC, 128 bytes per pixel and 64
// channels) and weights are rounded to half once, at pack time: one matrix instruction per product, half the bytes.  The arithmetic of
// a layer, which tests/test_gpu_conv_f16.py holds the kernels to:
//
//     y = round_half( relu?( sum_fp32( x_half * w_half ) + bias_fp32 + float(skip_half) ) )
//
// exact products, float32 accumulation, ONE rounding on store (a format mask can ask for float32 x / skip / y: a float32 x is rounded
// while it is staged, a float32 y is the unrounded accumulator result).  Beyond +-65504 the stored half is inf, NaN propagates.
//
// Structure of the 3 x 3 kernel = the narrow f16x3 kernel's: persistent 256-thread workgroups, THREE per compute unit at dilation 1 and two
// at dilations 2 .. 4 (50 .. 76 KiB of LDS; the f16x3 kernel: two and one), an item = 8 x 16 output pixels x 64 output channels, the input tile of 64 channels in LDS for nine taps
// (f16_common.h: 160 bytes per pixel, conflict-free ds_read_b128), a tap's 8 KiB of weights by LDS-DMA one tap ahead into one of two
// buffers, a counted s_waitcnt vmcnt and ONE raw s_barrier per tap, the next input tile requested in six pieces behind taps 0..5's
// DMA.  A wave = 2 M tiles (its two tile rows) x 4 N tiles, ONE accumulator set: 32 registers, 16 MFMAs per tap.
#include "conv_ends.h"
#include <type_traits>

namespace pnp {

struct ConvF16Args {
    const void* x;        // [n][H][W][C] half (float32 with HF_FMT_X32)
    const void* w;        // packed halves: blocks [cb][chunk][tap] of 8 KiB in fragment order (k_conv_pack_w_f16)
    const float* bias;    // [C] or null
    const void* skip;     // [n][H][W][C] half (float32 with HF_FMT_SKIP32) or null: added after the bias, before the ReLU
    void* y;              // [n][H][W][C] half (float32 with HF_FMT_Y32)
    int n, H, W, tiles_x, tiles_y, relu, C, fmt;
};
__device__ __forceinline__ TilePos tile_pos_f(int tiles_x, int tiles_y, int t) {
    const int per_img = tiles_x * tiles_y;
    TilePos q;
    q.img = t / per_img;
    const int trem = t - q.img * per_img, ty = trem / tiles_x;
    q.y0 = ty * CV_TY; q.x0 = (trem - ty * tiles_x) * CV_TX;
    return q;
}

template <int DIL> struct GeoFK {
    // the input tile doubles as the epilogue's staging area (4 waves x 32 pixels x H3_STR floats)
    static constexpr int TILE = GeoF<DIL>::XINB > 4 * 32 * H3_STR * 4 ? GeoF<DIL>::XINB : 4 * 32 * H3_STR * 4;
    static constexpr int LDS = TILE + 2 * HF_TAP16 * 16;          // 51 200 / 54 784 / 65 664 / 77 824 bytes at dilation 1 / 2 / 3 / 4
    // workgroups per compute unit: THREE at dilation 1 (153 600 of the 163 840 bytes; <= 168 registers), two at dilations 2 .. 4.  Measured at
    // [256, 64, 128, 128]: 0.380 ms with three against 0.418 with two (profiles/conv_f16_r07.txt) -- a tap is 16 MFMAs, too short for one
    // partner wave to cover the other's barrier and LDS latency
    static constexpr int WPS = 3 * LDS <= 160 * 1024 ? 3 : 2;
};

// The epilogue's second half.  The wave's 32 pixels x 64 channels lie in `stage` in pixel order, bias added; a lane takes EIGHT consecutive
// channels (octet co = lane & 7) of pixel slot lane >> 3, four times: staged row m = 8 it + (lane >> 3) = tile row 2 w + (m >> 4), column
// m & 15.  Eight channels are 16 bytes of a half pixel, 32 of a float32 one.  y = relu?(staged + skip), rounded once if y is half.
__device__ __forceinline__ void store_rows_f16(const ConvF16Args& a, const TilePos& q, const float* stage, int wv, int lane, const int cb) {
    const bool k32 = (a.fmt & HF_FMT_SKIP32) != 0, y32 = (a.fmt & HF_FMT_Y32) != 0;
    const int pixy = a.C * (y32 ? 4 : 2), pixk = a.C * (k32 ? 4 : 2);
    const int cby = 64 * cb * (y32 ? 4 : 2), cbk = 64 * cb * (k32 ? 4 : 2);
    const size_t hw = (size_t)a.H * a.W;
    const __amdgpu_buffer_rsrc_t ry = bytes_rsrc(a.y, q.img * hw * pixy + cby, (unsigned)hw * (unsigned)pixy - (unsigned)cby);
    const __amdgpu_buffer_rsrc_t rk = a.skip ? bytes_rsrc(a.skip, q.img * hw * pixk + cbk, (unsigned)hw * (unsigned)pixk - (unsigned)cbk) : ry;
    int ln = lane;                                               // (opaque copy: what derives from it is computed here, per item, not kept through the tap loop)
    asm volatile("" : "+v"(ln));
    const int ps = ln >> 3, co = ln & 7;
    int pidx[4];                                                 // the pixel's index in the image, or -1
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int m = 8 * it + ps, gx = q.x0 + (m & 15);
        pidx[it] = gx < a.W ? (q.y0 + 2 * wv + (m >> 4)) * a.W + gx : -1;      // rows below the image: beyond the buffer's range (no wrap: the launcher's bound)
    }
    u32x4v k0[4], k1[4];
    if (a.skip) {                                                // all requests first: one memory round trip
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int o = pidx[it] >= 0 ? pidx[it] * pixk + (k32 ? 32 : 16) * co : -32;
            k0[it] = __builtin_amdgcn_raw_buffer_load_b128(rk, o, 0, 0);
            if (k32) k1[it] = __builtin_amdgcn_raw_buffer_load_b128(rk, pidx[it] >= 0 ? o + 16 : -16, 0, 0);
        }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const float* sp = stage + (8 * it + ps) * H3_STR + 8 * co;
        f32x4 v0 = *reinterpret_cast<const f32x4*>(sp), v1 = *reinterpret_cast<const f32x4*>(sp + 4);
        if (a.skip) {
            if (k32) {
                v0 += as_f32x4(k0[it]); v1 += as_f32x4(k1[it]);
            } else {
                const h8 kh = __builtin_bit_cast(h8, k0[it]);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[e] += (float)kh[e]; v1[e] += (float)kh[4 + e]; }
            }
        }
        if (a.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { v0[e] = relu_keep_nan(v0[e]); v1[e] = relu_keep_nan(v1[e]); }
        }
        if (y32) {
            const int o = pidx[it] >= 0 ? pidx[it] * pixy + 32 * co : -32;
            const u32x4v o0 = {__float_as_uint(v0[0]), __float_as_uint(v0[1]), __float_as_uint(v0[2]), __float_as_uint(v0[3])};
            const u32x4v o1 = {__float_as_uint(v1[0]), __float_as_uint(v1[1]), __float_as_uint(v1[2]), __float_as_uint(v1[3])};
            __builtin_amdgcn_raw_buffer_store_b128(o0, ry, o, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(o1, ry, pidx[it] >= 0 ? o + 16 : -16, 0, 0);
        } else {
            const int o = pidx[it] >= 0 ? pidx[it] * pixy + 16 * co : -32;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, round8(v0, v1)), ry, o, 0, 0);
        }
    }
}

template <int DIL, bool X32>
__global__ __launch_bounds__(CV_THREADS, GeoFK<DIL>::WPS) void k_conv3x3_f16(ConvF16Args a, int nitems) {
    constexpr int HX = GeoF<DIL>::HX, XU = GeoF<DIL>::XU;
    // ONE LDS array (input tile, then the two weight buffers): with LDS-DMA in flight hipcc orders accesses to separate arrays conservatively
    __shared__ __attribute__((aligned(16))) char lds[GeoFK<DIL>::LDS];
    char* const xin = lds;
    u32x4v (*const wbuf)[HF_TAP16] = reinterpret_cast<u32x4v (*)[HF_TAP16]>(lds + GeoFK<DIL>::TILE);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // v_mfma_f32_16x16x32_f16: lane (i, kb) supplies A[row i][k = 8 kb ..] and B[k = 8 kb ..][column i]; the wave's 32 pixels are two
    // M tiles = its two tile rows (i = the pixel's column), its 64 output channels four N tiles
    const int i = lane & 15, kb = lane >> 4;
    // an ITEM is (tile, block cb of 64 output channels); item = tile * NC + cb and gridDim.x is a multiple of NC: a workgroup keeps its cb,
    // its weight stream -- [cb][chunk][tap] blocks of 8 KiB -- is periodic in 9 NC taps
    const int NC = a.C >> 6, pix = a.C * (X32 ? 4 : 2), period = 9 * NC, cstep = X32 ? 256 : 128;
    int item = blockIdx.x;
    if (item >= nitems) return;
    const int cb = item % NC;

    StagingF<DIL> st;
    staging_init_f<DIL>(a.W, tid, st, pix);
    XRegs<DIL, X32> xpre;
    {
        const FetchF f0 = fetch_begin_f<DIL, X32>(a.x, a.H, a.W, tile_pos_f(a.tiles_x, a.tiles_y, item / NC), tid, pix, 0);
        fetch_piece_f<DIL, X32, 0, XU>(f0, st, xpre);
    }
    // A tap's weights travel global memory -> LDS by LDS-DMA: thread t copies units t and t + 256 of the 512, one tap ahead of their use.
    // Completion is this wave's vmcnt; visibility to the other waves the barrier after the wait.
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 9 * a.C * a.C * 2, 0x00020000);
    const int wvoff = tid * 16, wbase = cb * period * (HF_TAP16 * 16);
#define HF_DMA(buf_, t_)                                                                                                   \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                           \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(&wbuf[buf_][wv * 64 + 256 * j]), 16, wvoff, \
                                                 wbase + (t_) * (HF_TAP16 * 16) + j * 4096, 0, 0);
    HF_DMA(0, 0)
    put_input_f<DIL, X32>(xin, tid, xpre);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int par = 0;                                                 // buffer of the current tap
    int t1 = 1 >= period ? 0 : 1;                                // stream position of the next tap's weights
    // a workgroup that arrived on an odd wave slot of its SIMD starts late, once (kernels_conv.hip): the partners stay out of phase
    if (__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4) & 1) __builtin_amdgcn_s_sleep(127);

#pragma unroll 1
    for (; item < nitems; item += gridDim.x) {
        const TilePos q = tile_pos_f(a.tiles_x, a.tiles_y, item / NC);
        f32x4 acc[2][4];                                         // [M tile = tile row of the wave][N tile of 16 channels]
        // One chunk = 64 input channels x 9 taps.  The first chunk of an item is its own instance of the code (FIRST): there the first
        // MFMA of every accumulator takes the constant 0 as its C operand.
        auto chunk = [&](const int cc, auto first_tag) __attribute__((always_inline)) {
            constexpr bool FIRST = decltype(first_tag)::value;
            // the input tile that follows this one -- the tile's next 64 input channels, or the first 64 of the next item -- is requested
            // now, in six pieces behind the weights of taps 0..5, and consumed after this chunk's nine taps
            const bool last = cc + 1 == NC;
            const bool more = !last || item + (int)gridDim.x < nitems;
            const FetchF nx = fetch_begin_f<DIL, X32>(a.x, a.H, a.W, last && more ? tile_pos_f(a.tiles_x, a.tiles_y, (item + gridDim.x) / NC) : q, tid, pix,
                                                      last ? 0 : cstep * (cc + 1), more);
            constexpr int PIECE = (XU + 5) / 6;
            // One tap = 2 K steps of 32 input channels = 4 half steps (a K step x two of the four N tiles) of 4 MFMAs.  The A operands of
            // K step 0 are read BEFORE the barrier (the input tile does not change inside a chunk), only the B reads of half step 0 stand
            // between the barrier and the first MFMA, and the request for the next tap's weights leaves behind half step 0's MFMAs.
            h8 af[2][2], bf[2][2];                                   // [slot][M tile] / [slot][N tile of the pair]
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#define HF_LOAD_A(slot, ap_, s2_)                                                                        \
            _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                                             \
                af[slot][mt] = *reinterpret_cast<const h8*>((ap_) + mt * (HX * HF_PS) + 64 * (s2_));
#define HF_LOAD_B(slot, h_)                                                                              \
            _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_)                                             \
                bf[slot][q_] = *reinterpret_cast<const h8*>(bp + 1024 * (((h_) >> 1) * 4 + 2 * ((h_) & 1) + q_));
#define HF_MFMA(h_)                                                                                      \
            __builtin_amdgcn_sched_barrier(0);                                                           \
            _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                                             \
            _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_) {                                           \
                const int nt_ = 2 * ((h_) & 1) + q_;                                                     \
                const bool z_ = FIRST && tap == 0 && (h_) < 2;         /* compile-time: the accumulators' first use */   \
                acc[mt][nt_] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[((h_) >> 1) & 1][mt], bf[(h_) & 1][q_], z_ ? zero4 : acc[mt][nt_], 0, 0, 0);  \
            }                                                                                            \
            __builtin_amdgcn_sched_barrier(0);
            // tap (0, 0), M tile 0: pixel (row 2 w, column i); + HX pixels: M tile 1; + 64 s2: K step
            const char* const a0 = xin + (2 * wv * HX + i) * HF_PS + 16 * kb;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - 3 * ky;
                const char* ap = a0 + (ky * DIL * HX + kx * DIL) * HF_PS;                            // input pixel of this tap
                const char* bp = reinterpret_cast<const char*>(&wbuf[par][0]) + lane * 16;          // + 1024 f: fragment f = s2 * 4 + nt
                // this wave's DMA of this tap's weights has landed (the loads of the input-prefetch piece issued behind it may still be in
                // flight: a counted wait), its LDS reads are back; then the barrier -- raw: __syncthreads() would drain vmcnt
#define HF_WAIT_BUT(n_) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(n_) : "memory");
#define HF_PIECE_LOADS(k_) ((X32 ? 2 : 1) * ((k_) * PIECE >= XU ? 0 : ((k_) + 1) * PIECE <= XU ? PIECE : XU - (k_) * PIECE))
                if (tap == 0 || tap >= 7) { HF_WAIT_BUT(0) }          // nothing was requested behind the tap before's DMA
                if (tap == 1) { HF_WAIT_BUT(HF_PIECE_LOADS(0)) }
                if (tap == 2) { HF_WAIT_BUT(HF_PIECE_LOADS(1)) }
                if (tap == 3) { HF_WAIT_BUT(HF_PIECE_LOADS(2)) }
                if (tap == 4) { HF_WAIT_BUT(HF_PIECE_LOADS(3)) }
                if (tap == 5) { HF_WAIT_BUT(HF_PIECE_LOADS(4)) }
                if (tap == 6) { HF_WAIT_BUT(HF_PIECE_LOADS(5)) }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (tap == 0) { HF_LOAD_A(0, ap, 0) }                 // taps 1..8: read at the end of the tap before
                HF_LOAD_B(0, 0)
                HF_LOAD_B(1, 1)
                HF_MFMA(0)
                HF_DMA(par ^ 1, t1)                                  // the next tap's weights
                // the counted wait of the next tap is right only if the two DMAs are OLDER than the piece: pin the order (the resource
                // test in tests/test_conv_f16_cpu.py walks the compiled ISA for it)
                __builtin_amdgcn_sched_barrier(0);
                t1 = t1 + 1 == period ? 0 : t1 + 1;
                if (tap == 0) fetch_piece_f<DIL, X32, 0 * PIECE, 1 * PIECE>(nx, st, xpre);
                if (tap == 1) fetch_piece_f<DIL, X32, 1 * PIECE, 2 * PIECE>(nx, st, xpre);
                if (tap == 2) fetch_piece_f<DIL, X32, 2 * PIECE, 3 * PIECE>(nx, st, xpre);
                if (tap == 3) fetch_piece_f<DIL, X32, 3 * PIECE, 4 * PIECE>(nx, st, xpre);
                if (tap == 4) fetch_piece_f<DIL, X32, 4 * PIECE, 5 * PIECE>(nx, st, xpre);
                if (tap == 5) fetch_piece_f<DIL, X32, 5 * PIECE, 6 * PIECE>(nx, st, xpre);
                HF_LOAD_A(1, ap, 1)
                HF_LOAD_B(0, 2)
                HF_MFMA(1)
                HF_LOAD_B(1, 3)
                HF_MFMA(2)
                if (tap + 1 < 9) {
                    const int ky1 = (tap + 1) / 3, kx1 = tap + 1 - 3 * ky1;
                    HF_LOAD_A(0, a0 + (ky1 * DIL * HX + kx1 * DIL) * HF_PS, 0)
                }
                HF_MFMA(3)
                par ^= 1;
            }
#undef HF_LOAD_A
#undef HF_LOAD_B
#undef HF_MFMA
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // every wave is done with this chunk's input (raw barrier: the DMA of
            __builtin_amdgcn_s_barrier();                            // the next tap's weights stays in flight)
            asm volatile("" ::: "memory");
            if (last) {
                // accumulator (reg r, lane (i, kb)) of tile (mt, nt) = pixel (tile row mt of the wave, column 4 kb + r), channel 16 nt + i: into
                // the wave's staging rows (pixel order, H3_STR floats apart: the four lane groups of a write start 16 banks apart), + bias
                float* stage = reinterpret_cast<float*>(xin) + wv * (32 * H3_STR);
                float bs[4] = {0.f, 0.f, 0.f, 0.f};
                if (a.bias) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bs[nt] = a.bias[64 * cb + 16 * nt + i];
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            stage[(16 * mt + 4 * kb + r) * H3_STR + 16 * nt + i] = acc[mt][nt][r] + bs[nt];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // a wave's LDS instructions execute in order: compiler-only ordering
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                store_rows_f16(a, q, stage, wv, lane, cb);
                if (more) __syncthreads();                           // every wave is done with the staging area
            }
            if (more) put_input_f<DIL, X32>(xin, tid, xpre);         // published by the barrier of the next chunk's first tap
        };
        chunk(0, std::true_type{});
#pragma unroll 1
        for (int cc = 1; cc < NC; ++cc) chunk(cc, std::false_type{});
    }
    // the last tap requested one more block of weights: no wave ends with an LDS-DMA in flight (its LDS may belong to the next
    // workgroup by the time the data lands)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// torch.nn.Conv2d weight [C out][C in][3][3] -> halves (round to nearest even) in fragment order, blocks [cb][chunk cc][tap] of 8 KiB:
// half j of lane (n, kb) of fragment (K step s, N tile nt) is half(W[out = 64 cb + 16 nt + n][in = 64 cc + 32 s + 8 kb + j][tap]).
// Half as many bytes as the float32 weights.  Once per model.
__global__ __launch_bounds__(256) void k_conv_pack_w_f16(const float* w_oihw, _Float16* wfrag, int C) { conv_pack_w_body<false>(w_oihw, wfrag, C); }

// ------------------------------------------------------------------------------------------
// First layer of the stacks (CIN <= 8 -> 64 channels; FFDNet's pixel-unshuffle / noise-level stage folded in): the float32 direct
// arithmetic of kernels_conv.hip's k_conv3x3_head on the float32 network input -- the same body (conv_ends.h) -- storing halves.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_conv3x3_head_f16(HeadArgs a) { conv3x3_head_body<true>(a); }

// ------------------------------------------------------------------------------------------
// Last layer of the stacks (64 -> COUT <= 4 channels, half NHWC in, float32 NCHW out, + bias) as a 16-column matrix product of which
// COUT columns are used (kernels_conv_f16x3.hip: k_conv3x3_tail_h3, one product instead of three): 36 MFMAs per wave and tile, bound by
// reading its input.  Persistent, two workgroups per compute unit.  The weights are rounded to half here, once per workgroup.
// x2: a second half tensor added to x in float32 while it is staged, the sum rounded to half once (the U-Net's last skip sum).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CV_THREADS, 2) void k_conv3x3_tail_f16(TailMmaArgs t, int ntiles) {
    constexpr int HX = GeoF<1>::HX, XU = GeoF<1>::XU;
    __shared__ __attribute__((aligned(16))) char xin[GeoF<1>::XINB];
    __shared__ __attribute__((aligned(16))) _Float16 wl[TAIL_WL];                    // [tap][K step][kb][n < 4][8 halves]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kb = lane >> 4;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;                                   // (uniform)
    StagingF<1> st;
    staging_init_f<1>(t.W, tid, st, 128);
    XRegs<1, false> xpre, x2pre;                                  // x2 keeps registers of its own: adding at load time would wait for the loads on the spot
    auto fetch = [&](const TilePos& q) __attribute__((always_inline)) {
        const FetchF f = fetch_begin_f<1, false>(t.x, t.H, t.W, q, tid, 128, 0);
        fetch_piece_f<1, false, 0, XU>(f, st, xpre);
        if (t.x2) {                                               // uniform
            const FetchF f2 = fetch_begin_f<1, false>(t.x2, t.H, t.W, q, tid, 128, 0);
            fetch_piece_f<1, false, 0, XU>(f2, st, x2pre);
        }
    };
    auto add_x2 = [&]() __attribute__((always_inline)) {         // x + x2 in float32, rounded to half once: the operand
#pragma unroll
        for (int u = 0; u < XU; ++u) {
            const h8 p = __builtin_bit_cast(h8, xpre.v[u]), r = __builtin_bit_cast(h8, x2pre.v[u]);
            h8 s;
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] = (_Float16)((float)p[e] + (float)r[e]);
            xpre.v[u] = __builtin_bit_cast(u32x4v, s);
        }
    };
    fetch(tile_pos_f(t.tiles_x, t.tiles_y, tile));
    for (int e = tid; e < TAIL_WL; e += CV_THREADS) wl[e] = (_Float16)tail_mma_weight(t, e);
    const char* const a0 = xin + (2 * wv * HX + i) * HF_PS + 16 * kb;
    const char* const b0 = reinterpret_cast<const char*>(wl) + kb * 64 + (i & 3) * 16;
    const bool col = i < t.cout;
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const float b = (col && t.bias) ? t.bias[i] : 0.f;
#pragma unroll 1
    for (; tile < ntiles; tile += gridDim.x) {
        const TilePos q = tile_pos_f(t.tiles_x, t.tiles_y, tile);
        if (t.x2) add_x2();
        put_input_f<1, false>(xin, tid, xpre);
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) fetch(tile_pos_f(t.tiles_x, t.tiles_y, tile + gridDim.x));       // in flight behind this tile's matrix products
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const char* ap = a0 + (ky * HX + kx) * HF_PS;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                h8 bw = *reinterpret_cast<const h8*>(b0 + (tap * 2 + s2) * 256);
                bw = col ? bw : zero;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(ap + mt * (HX * HF_PS) + 64 * s2), bw, acc[mt], 0, 0, 0);
            }
        }
        // accumulator (reg r, lane (i, kb)) of M tile mt = pixel (tile row 2 w + mt, column 4 kb + r), output channel i
        __syncthreads();                                          // every wave is past its taps: the tile may be reused (below, or by the next tile)
        tail_mma_store(t, q, reinterpret_cast<float*>(xin), tid, wv, i, 4 * kb, col, b, acc);
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
template <int DIL>
static hipError_t launch_f16_dil(hipStream_t s, const ConvF16Args& a, long long items, int cus) {
    // persistent workgroups, GeoFK<DIL>::WPS per compute unit, a multiple of NC = C / 64 of them (a workgroup keeps its block of output channels:
    // cp_grid); every workgroup's loop ends: item < nitems
    const dim3 grid((unsigned)cp_grid(items, GeoFK<DIL>::WPS, cus, a.C / CP_CSTEP));
    if (a.fmt & HF_FMT_X32) hipLaunchKernelGGL((k_conv3x3_f16<DIL, true>), grid, dim3(CV_THREADS), 0, s, a, (int)items);
    else hipLaunchKernelGGL((k_conv3x3_f16<DIL, false>), grid, dim3(CV_THREADS), 0, s, a, (int)items);
    return hipGetLastError();
}

hipError_t launch_conv3x3_f16(hipStream_t s, const void* x, const void* w, const float* bias, const void* skip, void* y,
                              int n, int C, int H, int W, int relu, int dilation, int fmt) {
    if (cp_check_body(n, C, H, W, dilation, fmt)) return hipErrorInvalidValue;
    const ConvTiling t = cp_tiling(n, H, W, CP_NARROW, C / CP_CSTEP);
    ConvF16Args a;
    a.x = x; a.w = w; a.bias = bias; a.skip = skip; a.y = y; a.n = n; a.H = H; a.W = W; a.relu = relu; a.C = C; a.fmt = fmt;
    a.tiles_x = t.tiles_x; a.tiles_y = t.tiles_y;
    const int cus = conv_compute_units();
    if (cus <= 0) return hipGetLastError();
    switch (dilation) {
        case 1: return launch_f16_dil<1>(s, a, t.items, cus);
        case 2: return launch_f16_dil<2>(s, a, t.items, cus);
        case 3: return launch_f16_dil<3>(s, a, t.items, cus);
        default: return launch_f16_dil<4>(s, a, t.items, cus);
    }
}

hipError_t launch_conv_pack_w_f16(hipStream_t s, const float* w_oihw, void* wfrag, int C) {
    if (cp_check_pack3(C)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_conv_pack_w_f16, dim3((unsigned)(9LL * C * C / 256)), dim3(256), 0, s, w_oihw, reinterpret_cast<_Float16*>(wfrag), C);
    return hipGetLastError();
}

hipError_t launch_conv3x3_head_f16(hipStream_t s, const float* x, const float* sigma, int sigma_per_image, const float* w_oihw, const float* bias,
                                   void* y_nhwc, int n, int cin, int H, int W, int relu, int ffdnet) {
    // ffdnet: x is the full-resolution image [n][1][H][W], the layer runs at ceil(H / 2) x ceil(W / 2) with cin = 5
    if (ffdnet ? cp_check_ffdnet(n, H, W) : cp_check_head(n, cin, H, W)) return hipErrorInvalidValue;
    HeadArgs a;
    a.x = x; a.w = w_oihw; a.bias = bias; a.y = y_nhwc; a.n = n; a.relu = relu;
    a.ffdnet = ffdnet ? 1 : 0; a.src_h = ffdnet ? H : 0; a.src_w = ffdnet ? W : 0; a.sigma = sigma; a.sigma_stride = sigma_per_image ? 1 : 0;
    a.cin = ffdnet ? 5 : cin; a.H = ffdnet ? cp_ffdnet_dim(H) : H; a.W = ffdnet ? cp_ffdnet_dim(W) : W;
    const ConvTiling t = cp_tiling(n, a.H, a.W, CP_NARROW);
    a.tiles_x = t.tiles_x; a.tiles_y = t.tiles_y;
    hipLaunchKernelGGL(k_conv3x3_head_f16, dim3((unsigned)t.items), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_conv3x3_tail_f16(hipStream_t s, const void* x_nhwc, const void* x2_nhwc, const float* w_oihw, const float* bias, float* y,
                                   int n, int cout, int H, int W, int shuffle_h, int shuffle_w) {
    return launch_tail_mma(s, k_conv3x3_tail_f16, x_nhwc, x2_nhwc, w_oihw, bias, y, n, cout, H, W, shuffle_h, shuffle_w);
}

}  // namespace pnp
