// Any-size c2c kernels of libpnpmri.so for gfx950: H, W in [128, 1024], float and double.
//
// The row / column roles of c2c_roles.h (RowIn / RowEpi / ColMid element forms and legal triples, shared with kernels_generic.hip)
// for every slice shape outside {256, 512}^2: the generic loop body of api.hip drives them unchanged.  Plan,
// tables and butterflies: anysize_plan.h (7-smooth lengths: mixed-radix Stockham; others: Bluestein over a power of two).
//
//   rows   : G rows per 256-thread workgroup, each row a line of LDS (pitch m + 1), both ping-pong buffers in LDS
//   columns: a tile of G columns x H rows, transposed into LDS on load (pitch m + 1, odd: the transposing writes of
//            consecutive columns fall in distinct banks); global accesses are G-element row segments
// G is chosen per axis on the host so that a workgroup holds about 40 KiB of LDS (16 lines at most, 1 at least: a
// Bluestein line of m = 2048 in double takes 64 KiB).  Every stage is one pass of all 256 threads over the G lines'
// butterflies and ends in a workgroup barrier.  Twiddles, chirp and the Bluestein kernel spectrum are device tables owned by
// the context (fp64-generated, rounded once to float for a float context), read through the caches.
//
// Not a fast path: the iteration runs the three launches of the generic loop (rows, columns, rows) at any size.
#include "internal.h"
#include "anysize_plan.h"
#include "coil_plan.h"
#include <string.h>
#include <atomic>
#include <vector>

namespace pnp {

using anysize::Plan;

// one axis of a context, as the kernels see it
template <typename R> struct AxisT {
    using C = typename CxOf<R>::type;
    Plan plan;
    const C* tw;        // [m]  W_m^i
    const C* chirp;     // [n]  w_j (Bluestein only)
    const C* kern;      // [m]  FFT_m(conj chirp) / m (Bluestein only)
    int lines;          // G: lines per workgroup
    int pitch;          // LDS complex elements per line (m + 1)
};

struct AnySize {
    bool f64 = false;
    Plan plan[2];               // [0] rows (length W), [1] columns (length H)
    void* table[2] = {};        // per axis: tw [m], chirp [n], kern [m] in the context's precision
    int lines[2] = {};
};

constexpr int ANY_THREADS = 256;
constexpr size_t ANY_LDS_TARGET = 40 * 1024;        // per workgroup: four workgroups per compute unit for the float lines
constexpr size_t ANY_LDS_MAX = 96 * 1024;           // bounds what any configuration needs (the most: one double Bluestein line, 64 KiB + 32 B)

template <typename R> static size_t any_lds(const AxisT<R>& t) { return 2 * sizeof(typename CxOf<R>::type) * (size_t)t.lines * t.pitch; }

// ---- the line transform: G lines of LDS, unnormalised, forward or inverse ----

template <bool INV, typename C>
__device__ __forceinline__ C* stockham_lines(C* a, C* b, int G, int pitch, const Plan& pl, const C* tw) {
    const int L = pl.m;
    int Ns = 1;
    for (int s = 0; s < pl.nstages; ++s) {
        const int r = pl.radix[s], nb = L / r, total = G * nb;
        for (int i = threadIdx.x; i < total; i += ANY_THREADS) {
            const int g = i / nb, j = i - g * nb;
            anysize::stockham_bfly_r<INV>(r, a + g * pitch, b + g * pitch, tw, L, Ns, j);
        }
        __syncthreads();
        C* t = a; a = b; b = t;
        Ns *= r;
    }
    return a;
}

// a: G lines holding n values each; b: scratch.  Returns the buffer holding the n results of every line.
// Bluestein: chirp, forward m-point transform, times the kernel spectrum, inverse m-point transform, chirp.  The inverse
// transform is conj(forward(conj(x))): the conjugations ride on the two chirp passes.
template <bool INV, typename R>
__device__ __forceinline__ typename CxOf<R>::type* line_fft(typename CxOf<R>::type* a, typename CxOf<R>::type* b, const AxisT<R>& t) {
    using C = typename CxOf<R>::type;
    const int G = t.lines, pitch = t.pitch, n = t.plan.n, m = t.plan.m;
    if (!t.plan.bluestein) return stockham_lines<INV>(a, b, G, pitch, t.plan, t.tw);
    for (int i = threadIdx.x; i < G * m; i += ANY_THREADS) {
        const int g = i / m, j = i - g * m;
        C v = mkc<C>(R(0), R(0));
        if (j < n) {
            v = a[g * pitch + j];
            if (INV) v = cconj(v);
            v = cmul(v, t.chirp[j]);
        }
        a[g * pitch + j] = v;
    }
    __syncthreads();
    C* r = stockham_lines<false>(a, b, G, pitch, t.plan, t.tw);
    C* o = (r == a) ? b : a;
    for (int i = threadIdx.x; i < G * m; i += ANY_THREADS) {
        const int g = i / m, j = i - g * m;
        r[g * pitch + j] = cmul(r[g * pitch + j], t.kern[j]);
    }
    __syncthreads();
    r = stockham_lines<true>(r, o, G, pitch, t.plan, t.tw);
    for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
        const int g = i / n, j = i - g * n;
        C v = cmul(r[g * pitch + j], t.chirp[j]);
        if (INV) v = cconj(v);
        r[g * pitch + j] = v;
    }
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------------
// rows: row_load / row_store of c2c_roles.h around the line transform
// ------------------------------------------------------------------------------------------
template <int IN, bool INV, int EPI, typename R>
__global__ __launch_bounds__(ANY_THREADS) void k_any_rows(RowArgsT<R> p, AxisT<R> t) {
    using C = typename CxOf<R>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char any_smem[];
    C* sA = reinterpret_cast<C*>(any_smem);
    C* sB = sA + t.lines * t.pitch;
    const int G = t.lines, n = t.plan.n, pitch = t.pitch;
    const int row0 = blockIdx.x * G;
    for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
        const int g = i / n, k = i - g * n, row = row0 + g;
        C v = mkc<C>(R(0), R(0));
        if (row < p.nrows) v = row_load<IN>(p, (size_t)row * n + k);
        sA[g * pitch + k] = v;
    }
    __syncthreads();
    const C* r = line_fft<INV, R>(sA, sB, t);
    for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
        const int g = i / n, k = i - g * n, row = row0 + g;
        if (row < p.nrows) row_store<EPI>(p, (size_t)row * n + k, r[g * pitch + k]);
    }
}

// The LDS opt-in (internal.h) of the any-size kernels: only a double Bluestein line needs it (64 KiB + 32 B); ANY_LDS_MAX bounds every
// configuration.
template <int IN, bool INV, int EPI, typename R>
static hipError_t any_rows_t(hipStream_t s, const AxisT<R>& t, const RowArgsT<R>& a) {
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_any_rows<IN, INV, EPI, R>, done, any_lds(t), ANY_LDS_MAX)) return e;
    const unsigned grid = (unsigned)((a.nrows + t.lines - 1) / t.lines);
    hipLaunchKernelGGL((k_any_rows<IN, INV, EPI, R>), dim3(grid), dim3(ANY_THREADS), any_lds(t), s, a, t);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// rows with coils (coil_plan.h): the two row roles of the multi-coil data consistency.  A workgroup owns G rows as k_any_rows does and
// walks the C coils of each; beside the two ping-pong buffers it holds G * n values: the image rows (expanding) resp. the sums over
// the coils (combining).  Every thread touches the same (line, k) elements in every pass, so that third array needs no barrier.
// ------------------------------------------------------------------------------------------
template <typename R> static size_t coil_lds(const AxisT<R>& t) { return any_lds(t) + sizeof(typename CxOf<R>::type) * (size_t)t.lines * t.plan.n; }
// lines per workgroup of the coil rows: the third array counts against the same ANY_LDS_TARGET, so that as many workgroups share a compute
// unit as with the plain rows (at n = 256 in float: 6 lines of 6160 B instead of 9 of 4112 B + 2048 B)
template <typename R> static AxisT<R> coil_axis(AxisT<R> t) {
    using C = typename CxOf<R>::type;
    const size_t per_line = sizeof(C) * (2 * (size_t)t.pitch + (size_t)t.plan.n);
    int g = (int)(ANY_LDS_TARGET / per_line);
    if (g > t.lines) g = t.lines;
    t.lines = g < 1 ? 1 : g;
    return t;
}

// expanding rows, forward: work[b][c][h][:] = F_W(S_c[h][:] * image[b][h][:]), c = 0 .. C - 1 -- the image row is read once
template <bool REAL, typename R>
__global__ __launch_bounds__(ANY_THREADS) void k_any_rows_coil_in(CoilRowArgsT<R> p, AxisT<R> t) {
    using C = typename CxOf<R>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char any_smem[];
    C* sA = reinterpret_cast<C*>(any_smem);
    C* sB = sA + t.lines * t.pitch;
    C* sP = sB + t.lines * t.pitch;
    const int G = t.lines, n = t.plan.n, pitch = t.pitch, H = p.H;
    const int row0 = blockIdx.x * G;
    for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
        const int g = i / n, row = row0 + g;
        C v = mkc<C>(R(0), R(0));
        if (row < p.nrows) {
            const size_t e = (size_t)row * n + (i - g * n);
            if (REAL) v = mkc<C>(p.rin[e], R(0)); else v = p.cin[e];
        }
        sP[i] = v;
    }
    for (int c = 0; c < p.ncoils; ++c) {
        for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
            const int g = i / n, k = i - g * n, row = row0 + g;
            C v = mkc<C>(R(0), R(0));
            if (row < p.nrows) {
                const int b = coil_row_slice(row, H), h = coil_row_line(row, H);
                v = cmul(sP[i], p.maps[coil_map_index(coil_set_of(p.coil_id, b), c, p.ncoils, h, k, H, n)]);
            }
            sA[g * pitch + k] = v;
        }
        __syncthreads();
        const C* r = line_fft<false, R>(sA, sB, t);
        for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
            const int g = i / n, k = i - g * n, row = row0 + g;
            if (row >= p.nrows) continue;
            p.work[coil_work_index(coil_row_slice(row, H), c, p.ncoils, coil_row_line(row, H), k, H, n)] = r[g * pitch + k];
        }
        __syncthreads();
    }
}

// combining rows, inverse: out[b][h][:] = sum_c conj(S_c[h][:]) * scale * F_W^-1(work[b][c][h][:]) [+ la2 * p[b][h][:]], coils in order;
// with p the row's Re<p, out> goes to partial[row], summed in double by one wave (coil_plan.h, cg_wave_sum)
template <typename R>
__global__ __launch_bounds__(ANY_THREADS) void k_any_rows_coil_epi(CoilRowArgsT<R> p, AxisT<R> t) {
    using C = typename CxOf<R>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char any_smem[];
    C* sA = reinterpret_cast<C*>(any_smem);
    C* sB = sA + t.lines * t.pitch;
    C* sAcc = sB + t.lines * t.pitch;
    const int G = t.lines, n = t.plan.n, pitch = t.pitch, H = p.H;
    const int row0 = blockIdx.x * G;
    for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) sAcc[i] = mkc<C>(R(0), R(0));
    for (int c = 0; c < p.ncoils; ++c) {
        for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
            const int g = i / n, k = i - g * n, row = row0 + g;
            C v = mkc<C>(R(0), R(0));
            if (row < p.nrows) v = p.work[coil_work_index(coil_row_slice(row, H), c, p.ncoils, coil_row_line(row, H), k, H, n)];
            sA[g * pitch + k] = v;
        }
        __syncthreads();
        const C* r = line_fft<true, R>(sA, sB, t);
        for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
            const int g = i / n, k = i - g * n, row = row0 + g;
            if (row >= p.nrows) continue;
            const int b = coil_row_slice(row, H), h = coil_row_line(row, H);
            const C v = r[g * pitch + k];
            const C sv = mkc<C>(v.x * p.scale, v.y * p.scale);
            sAcc[i] = cadd(sAcc[i], cmulc(sv, p.maps[coil_map_index(coil_set_of(p.coil_id, b), c, p.ncoils, h, k, H, n)]));
        }
        __syncthreads();
    }
    double* prod = reinterpret_cast<double*>(any_smem);          // [G][n] doubles over sA (G * pitch complex: room enough); sA is idle now
    for (int i = threadIdx.x; i < G * n; i += ANY_THREADS) {
        const int g = i / n, row = row0 + g;
        double d = 0.0;
        if (row < p.nrows) {
            const size_t e = (size_t)row * n + (i - g * n);
            C o = sAcc[i];
            if (p.p) {
                const C pv = p.p[e];
                o = mkc<C>(fma_r(p.la2, pv.x, o.x), fma_r(p.la2, pv.y, o.y));
                d = (double)pv.x * (double)o.x + (double)pv.y * (double)o.y;
            }
            p.cout[e] = o;
        }
        prod[i] = d;
    }
    if (!p.p) return;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int g = wave; g < G; g += ANY_THREADS / 64) {
        const int row = row0 + g;
        double s = 0.0;
        for (int k = lane; k < n; k += 64) s += prod[g * n + k];
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0 && row < p.nrows) p.partial[row] = s;
    }
}

template <typename R> static AxisT<R> axis(const AnySize* A, int i);          // below, with the host side

template <typename R>
hipError_t anysize_coil_rows_in(const AnySize* A, hipStream_t s, const CoilRowArgsT<R>& a) {
    if (!A || A->f64 != std::is_same<R, double>::value || a.ncoils < 1 || a.ncoils > COIL_MAX_C || a.H != A->plan[1].n) return hipErrorInvalidValue;
    const AxisT<R> t = coil_axis(axis<R>(A, 0));
    static std::atomic<bool> done[2][64] = {};
    const void* fn = a.cin ? (const void*)k_any_rows_coil_in<false, R> : (const void*)k_any_rows_coil_in<true, R>;
    if (hipError_t e = lds_opt_in(fn, done[a.cin ? 0 : 1], coil_lds(t), ANY_LDS_MAX)) return e;
    const unsigned grid = (unsigned)((a.nrows + t.lines - 1) / t.lines);
    if (a.cin) hipLaunchKernelGGL((k_any_rows_coil_in<false, R>), dim3(grid), dim3(ANY_THREADS), coil_lds(t), s, a, t);
    else       hipLaunchKernelGGL((k_any_rows_coil_in<true, R>), dim3(grid), dim3(ANY_THREADS), coil_lds(t), s, a, t);
    return hipGetLastError();
}
template hipError_t anysize_coil_rows_in<float>(const AnySize*, hipStream_t, const CoilRowArgsT<float>&);
template hipError_t anysize_coil_rows_in<double>(const AnySize*, hipStream_t, const CoilRowArgsT<double>&);

template <typename R>
hipError_t anysize_coil_rows_epi(const AnySize* A, hipStream_t s, const CoilRowArgsT<R>& a) {
    if (!A || A->f64 != std::is_same<R, double>::value || a.ncoils < 1 || a.ncoils > COIL_MAX_C || a.H != A->plan[1].n) return hipErrorInvalidValue;
    const AxisT<R> t = coil_axis(axis<R>(A, 0));
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_any_rows_coil_epi<R>, done, coil_lds(t), ANY_LDS_MAX)) return e;
    const unsigned grid = (unsigned)((a.nrows + t.lines - 1) / t.lines);
    hipLaunchKernelGGL((k_any_rows_coil_epi<R>), dim3(grid), dim3(ANY_THREADS), coil_lds(t), s, a, t);
    return hipGetLastError();
}
template hipError_t anysize_coil_rows_epi<float>(const AnySize*, hipStream_t, const CoilRowArgsT<float>&);
template hipError_t anysize_coil_rows_epi<double>(const AnySize*, hipStream_t, const CoilRowArgsT<double>&);

// ------------------------------------------------------------------------------------------
// columns: [optional forward] -> col_mid of c2c_roles.h -> [optional inverse]
// ------------------------------------------------------------------------------------------
template <bool PRE, int MID, bool POST, typename R>
__global__ __launch_bounds__(ANY_THREADS) void k_any_cols(ColArgsT<R> p, AxisT<R> t, int W) {
    using C = typename CxOf<R>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char any_smem[];
    C* sA = reinterpret_cast<C*>(any_smem);
    C* sB = sA + t.lines * t.pitch;
    const int G = t.lines, H = t.plan.n, pitch = t.pitch;
    const int tiles = (W + G - 1) / G;
    const int b = blockIdx.x / tiles;
    const int k0 = (blockIdx.x % tiles) * G;
    const int gc = min(G, W - k0);                     // columns of this tile inside the slice
    const size_t sbase = (size_t)b * H * W;
    for (int idx = threadIdx.x; idx < H * G; idx += ANY_THREADS) {
        const int r = idx / G, c = idx - r * G;
        sA[c * pitch + r] = c < gc ? p.in[sbase + (size_t)r * W + k0 + c] : mkc<C>(R(0), R(0));
    }
    __syncthreads();
    C* cur = sA;
    C* oth = sB;
    if (PRE) {
        C* r = line_fft<false, R>(sA, sB, t);
        if (r != sA) { cur = sB; oth = sA; }
    }
    if (MID != MID_NONE) {
        const int mid = p.mask_id ? p.mask_id[b] : 0;
        const uint8_t* mask = p.mask_bank + (size_t)mid * H * W;
        const C* yb = p.y + ((MID == MID_MASK_ADD && !p.y_per_slice) ? 0 : sbase);
        for (int idx = threadIdx.x; idx < H * G; idx += ANY_THREADS) {
            const int r = idx / G, c = idx - r * G;
            if (c >= gc) continue;
            const size_t g = (size_t)r * W + k0 + c;
            cur[c * pitch + r] = col_mid<MID>(cur[c * pitch + r], mask[g] != 0, &yb[g], p.c);
        }
        __syncthreads();
    }
    if (POST) {
        C* r = line_fft<true, R>(cur, oth, t);
        if (r != cur) { oth = cur; cur = r; }
    }
    for (int idx = threadIdx.x; idx < H * G; idx += ANY_THREADS) {
        const int r = idx / G, c = idx - r * G;
        if (c < gc) p.out[sbase + (size_t)r * W + k0 + c] = cur[c * pitch + r];
    }
}

template <bool PRE, int MID, bool POST, typename R>
static hipError_t any_cols_t(hipStream_t s, const AxisT<R>& t, int W, const ColArgsT<R>& a) {
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_any_cols<PRE, MID, POST, R>, done, any_lds(t), ANY_LDS_MAX)) return e;
    const unsigned grid = (unsigned)a.B * (unsigned)((W + t.lines - 1) / t.lines);
    hipLaunchKernelGGL((k_any_cols<PRE, MID, POST, R>), dim3(grid), dim3(ANY_THREADS), any_lds(t), s, a, t, W);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// host: plan and tables per context
// ------------------------------------------------------------------------------------------
template <typename R> static AxisT<R> axis(const AnySize* A, int i) {
    using C = typename CxOf<R>::type;
    AxisT<R> t;
    t.plan = A->plan[i];
    t.tw = reinterpret_cast<const C*>(A->table[i]);
    t.chirp = t.tw + t.plan.m;
    t.kern = t.chirp + t.plan.n;
    t.lines = A->lines[i];
    t.pitch = t.plan.m + 1;
    return t;
}

// lines per workgroup: about ANY_LDS_TARGET of LDS, 1..16, and no more than the lines there are across the axis
static int lines_per_wg(const Plan& p, size_t cbytes, int across) {
    const size_t per_line = 2 * cbytes * (size_t)(p.m + 1);
    int g = (int)(ANY_LDS_TARGET / per_line);
    if (g > 16) g = 16;
    if (g > across) g = across;
    return g < 1 ? 1 : g;
}

template <typename C>
static hipError_t upload_axis(const Plan& p, void** out) {
    std::vector<double> tre, tim, cre, cim;
    anysize::twiddles(p.m, tre, tim);
    std::vector<C> h((size_t)2 * p.m + p.n, mkc<C>(0.0, 0.0));
    for (int i = 0; i < p.m; ++i) h[i] = mkc<C>(tre[i], tim[i]);
    if (p.bluestein) {
        anysize::chirp(p.n, cre, cim);
        std::vector<double2> kd;
        anysize::bluestein_kernel<double2>(p, cre, cim, kd);
        for (int j = 0; j < p.n; ++j) h[p.m + j] = mkc<C>(cre[j], cim[j]);
        for (int i = 0; i < p.m; ++i) h[p.m + p.n + i] = mkc<C>(kd[i].x, kd[i].y);
    }
    hipError_t e = hipMalloc(out, h.size() * sizeof(C));
    if (e == hipSuccess) e = hipMemcpy(*out, h.data(), h.size() * sizeof(C), hipMemcpyHostToDevice);
    return e;
}

bool anysize_supported(int n) { return n >= anysize::MIN_N && n <= anysize::MAX_N; }

AnySize* anysize_create(int H, int W, bool f64, hipError_t* err) {
    *err = hipSuccess;
    if (!anysize_supported(H) || !anysize_supported(W)) { *err = hipErrorInvalidValue; return nullptr; }
    AnySize* A = new (std::nothrow) AnySize();
    if (!A) { *err = hipErrorOutOfMemory; return nullptr; }
    A->f64 = f64;
    const int len[2] = {W, H}, across[2] = {1 << 30, W};
    const size_t cb = f64 ? sizeof(double2) : sizeof(float2);
    for (int i = 0; i < 2 && *err == hipSuccess; ++i) {
        A->plan[i] = anysize::make_plan(len[i]);
        if (A->plan[i].nstages < 1 || A->plan[i].m > anysize::MAX_M) { *err = hipErrorInvalidValue; break; }
        A->lines[i] = lines_per_wg(A->plan[i], cb, across[i]);
        *err = f64 ? upload_axis<double2>(A->plan[i], &A->table[i]) : upload_axis<float2>(A->plan[i], &A->table[i]);
    }
    if (*err != hipSuccess) { anysize_destroy(A); return nullptr; }
    return A;
}

void anysize_destroy(AnySize* A) {
    if (!A) return;
    for (void* p : A->table) if (p) (void)hipFree(p);
    delete A;
}

int anysize_describe(const AnySize* A, int i, char* buf, int len) {
    if (!A || i < 0 || i > 1 || !buf || len < 1) return -1;
    const Plan& p = A->plan[i];
    int o = p.bluestein ? snprintf(buf, (size_t)len, "bluestein %d -> %d =", p.n, p.m) : snprintf(buf, (size_t)len, "stockham %d =", p.n);
    for (int s = 0; s < p.nstages && o >= 0 && o < len; ++s) o += snprintf(buf + o, (size_t)(len - o), s ? "*%d" : " %d", p.radix[s]);
    return 0;
}

template <typename R>
hipError_t anysize_rows(const AnySize* A, hipStream_t s, RowIn in, bool inv, RowEpi epi, const RowArgsT<R>& a) {
    if (!A || A->f64 != std::is_same<R, double>::value) return hipErrorInvalidValue;
    const AxisT<R> t = axis<R>(A, 0);
    return row_roles(in, inv, epi, hipErrorInvalidValue,
                     [&](auto IN, auto INV, auto EPI) { return any_rows_t<IN(), INV(), EPI()>(s, t, a); });
}
template hipError_t anysize_rows<float>(const AnySize*, hipStream_t, RowIn, bool, RowEpi, const RowArgsT<float>&);
template hipError_t anysize_rows<double>(const AnySize*, hipStream_t, RowIn, bool, RowEpi, const RowArgsT<double>&);

template <typename R>
hipError_t anysize_cols(const AnySize* A, hipStream_t s, bool pre, ColMid mid, bool post, const ColArgsT<R>& a) {
    if (!A || A->f64 != std::is_same<R, double>::value) return hipErrorInvalidValue;
    const AxisT<R> t = axis<R>(A, 1);
    const int W = A->plan[0].n;
    return col_roles(pre, mid, post, hipErrorInvalidValue,
                     [&](auto PRE, auto MID, auto POST) { return any_cols_t<PRE(), MID(), POST()>(s, t, W, a); });
}
template hipError_t anysize_cols<float>(const AnySize*, hipStream_t, bool, ColMid, bool, const ColArgsT<float>&);
template hipError_t anysize_cols<double>(const AnySize*, hipStream_t, bool, ColMid, bool, const ColArgsT<double>&);

}  // namespace pnp
