// g++ host emulation of k_slice<2> (kernels_slice256.hip) with its transient LDS halved: the exchange of a 16-lane transform group in
// two planes (real parts, then imaginary parts through the same words: slice_layout.h sl_xw), the transpositions' four passes in eight
// halves (sl_row8; passes and slots sl_pass4 / sl_slot4) and the resident units of w (sl_units_lds / sl_units_reg / w_home) -- lane by
// lane, on ONE array of LDS words laid out by the map SL2_* of slice_layout.h, with the cores of csrc/fft16.h.  A launch of `iters`
// iterations: prologue (rows, resident units go home) -> iters x (T1 -> columns -> T2 -> rows) -> flush; the last iteration stores x in
// natural order through the exchange regions, one image row of a pair after the other.
// Every transient word carries the lane that wrote it in the current PHASE (one plane of one wave's exchanges, one half of a pass, ...);
// a phase starts with its words poisoned.  Exits non-zero when
//   40  two LDS areas overlap, an area leaves the compute unit's 163 840 bytes, or a user of the exchange regions does not fit its region
//   41  a transient word is read in a phase in which no lane wrote it          42  a transient word is written twice in one phase
//   43  a transient access leaves the area of its phase                        44  a pass half moves the wrong number of values
//   21 / 23  a resident float has two owners / none       31  a lane reads resident w another lane wrote       28 / 29  a w element with two homes / units miscounted
//   25 / 32  the flush leaves the state incomplete / the HBM copy of a resident element was written meanwhile
// Input file as fused_emulation.cpp (slice 0 of it is used); argv[3] = iterations; output x, z, w (double).  -DSLICE_UNITS_LDS1= /
// -DSLICE_UNITS_REG= select another table than the kernel's (the test runs both).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../pnp_admm_cnc_mri_amd/csrc/fused_layout.h"
#include "../../pnp_admm_cnc_mri_amd/csrc/slice_layout.h"
using namespace pnp;
typedef float R;
typedef cxT<R> C;

static C TW[256];
static C F[8][64][4][16];         // the register file: [wave][lane][set][j]
static C G[8][64][4][16];
static float REGS[8][64][SL_NREG > 0 ? SL_NREG : 1][4];      // register units of w
static const int WORDS = SL_LDS_CU / 4;
static float LDSW[WORDS];         // the compute unit's LDS
static int WRITER[WORDS];         // transient words: thread (64 wave + lane) that wrote it in this phase, -1 = poisoned; resident words: the owner
static int PH_LO, PH_HI;          // words of the current phase

static void fail(int code) { exit(code); }
static void phase(int lo_byte, int bytes) {
    PH_LO = lo_byte / 4; PH_HI = (lo_byte + bytes) / 4;
    for (int i = PH_LO; i < PH_HI; ++i) { WRITER[i] = -1; LDSW[i] = NAN; }
}
static void t_write(int word, int thread, float v) {
    if (word < PH_LO || word >= PH_HI) fail(43);
    if (WRITER[word] != -1) fail(42);
    WRITER[word] = thread; LDSW[word] = v;
}
static float t_read(int word) {
    if (word < PH_LO || word >= PH_HI) fail(43);
    if (WRITER[word] == -1) fail(41);
    return LDSW[word];
}
static void t_write_c(int cword, int thread, C v, bool swapped) { t_write(2 * cword, thread, swapped ? v.y : v.x); t_write(2 * cword + 1, thread, swapped ? v.x : v.y); }
static C t_read_c(int cword) { const float a = t_read(2 * cword), b = t_read(2 * cword + 1); return mk<R>(a, b); }

static int wave_words(int wv) { return SL2_XB / 4 + wv * SL_XWAVE; }          // first word of a wave's exchange regions
static void wave_phase(int wv) { phase(SL2_XB + 4 * wv * SL_XWAVE, 4 * SL_XWAVE); }

// home of the k-th float of access q of register set `set` of thread (wv, lane): an LDS word, a register, or HBM
static float* w_at_home(int set, int wv, int lane, int q, int k, int* word = nullptr) {
    const int t = lane & 15, rr = 4 * wv + (lane >> 4);
    if (word) *word = -1;
    switch (w_home(set, q)) {
    case W_LDS: {
        const int at = set == 0 ? SL2_RES0 / 4 + sl_res_index(rr, t, q) + k
                                : SL2_RES1 / 4 + sl_res1_index(popc8(sl_units_lds(set) & ((1u << q) - 1)), rr, t) + k;
        if (at < SL2_RES0 / 4 || at >= SL2_END / 4) fail(20);
        if (word) *word = at;
        return LDSW + at;
    }
    case W_REG: return &REGS[wv][lane][sl_reg_slot(set, q)][k];
    default: return nullptr;
    }
}

// 16-lane transform of the group (wave wv, lanes 16 g ..), register set `set` of F: the exchange crosses the group's region in two planes
static void group_fft(int wv, int g, int set, bool inv) {
    const int base = wave_words(wv) + g * SL_XREGION;
    C a[16][16];
    for (int t = 0; t < 16; ++t) {
        C tw[16];
        for (int j = 0; j < 16; ++j) { a[t][j] = F[wv][16 * g + t][set][j]; tw[j] = TW[t * j]; }
        if (inv) fft256_head<true>(a[t], tw); else fft256_head<false>(a[t], tw);
    }
    for (int h = 0; h < 2; ++h) {
        phase(4 * base, 4 * SL_XREGION);
        for (int t = 0; t < 16; ++t) for (int k = 0; k < 16; ++k) t_write(base + sl_xw(k, t), 64 * wv + 16 * g + t, h ? a[t][k].y : a[t][k].x);
        for (int t = 0; t < 16; ++t) for (int k = 0; k < 16; ++k) { const float v = t_read(base + sl_xw(t, k)); if (h) a[t][k].y = v; else a[t][k].x = v; }
    }
    for (int t = 0; t < 16; ++t) {
        if (inv) fft256_tail<true>(a[t]); else fft256_tail<false>(a[t]);
        for (int j = 0; j < 16; ++j) F[wv][16 * g + t][set][j] = a[t][j];
    }
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int iters = atoi(argv[3]);
    if (iters < 1) return 2;
    for (int m = 0; m < 256; ++m) { const double a = -2.0 * M_PI * m / 256.0; TW[m] = mk<R>((R)cos(a), (R)sin(a)); }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int mode, cnc; float cdc; ProxCoef pc;
    if (fread(&mode, 4, 1, f) != 1 || fread(&cnc, 4, 1, f) != 1 || fread(&cdc, 4, 1, f) != 1 || fread(&pc, sizeof(pc), 1, f) != 1) return 4;
    const int N = 65536;
    std::vector<float> z(2 * N), w(2 * N), x(N, NAN);
    std::vector<c32> y(2 * N);
    std::vector<uint8_t> mask(2 * N);
    if (fread(z.data(), 4, 2 * N, f) != 2u * N || fread(w.data(), 4, 2 * N, f) != 2u * N ||
        fread(y.data(), 8, 2 * N, f) != 2u * N || fread(mask.data(), 1, 2 * N, f) != 2u * N) return 5;
    fclose(f);
    // ---- the LDS map: areas in the compute unit, pairwise apart; what lives in the exchange regions fits there -----------------
    {
        const int area[5][2] = {{SL2_XB, SL2_XB_BYTES}, {SL2_TW, SL2_TW_BYTES}, {SL2_YS, SL2_YS_BYTES}, {SL2_RES0, SL2_RES0_BYTES}, {SL2_RES1, SL2_RES1_BYTES}};
        long total = 0;
        for (int i = 0; i < 5; ++i) {
            if (area[i][0] < 0 || area[i][1] <= 0 || area[i][0] + area[i][1] > SL_LDS_CU || area[i][0] % 16) fail(40);
            for (int k = 0; k < i; ++k) if (area[i][0] < area[k][0] + area[k][1] && area[k][0] < area[i][0] + area[i][1]) fail(40);
            total += area[i][1];
        }
        if (total > SL_LDS_CU || SL2_END > SL_LDS_CU) fail(40);
        if (SL_WAVES * SL_XWAVE * 4 > SL2_XB_BYTES || SL_BUF8 * 8 > SL2_XB_BYTES) fail(40);                   // regions and buffer inside their area
        if (sl_xw(15, 15) >= SL_XREGION || 256 > SL_XREGION || 272 * 2 > SL_XWAVE || (SL_XREGION * 4) % 16) fail(40);   // exchange, a plane of x, the packed column
        if (SL_NLDS1 > SL_RES1 || (SLICE_RESIDENT && sl_units_lds(0) != 0xFFu)) fail(30);
        for (int set = 0; set < SL_SETS; ++set) if ((sl_units_lds(set) & sl_units_reg(set)) || (set >= 2 && sl_units_lds(set))) fail(30);
    }
    for (int i = 0; i < WORDS; ++i) { LDSW[i] = NAN; WRITER[i] = -1; }
    // ---- tables of slice 0 in column-form thread order -----------------------------------------
    std::vector<C> Yh(YH3_SLICE), Ys(256);
    std::vector<uint32_t> Mh(MH3_SLICE, 0), Ms(16, 0);
    for (int set = 0; set < SL_SETS; ++set) for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) {
        const int c = sl_unit(set, wv, lane), t = lane & 15;
        for (int j = 0; j < 16; ++j) {
            int code; C yh;
            hermitian_entry_t<R>(y.data(), mask.data(), t + 16 * j, c, yh, code);
            Yh[yh3_index(0, set, j, wv, lane)] = yh;
            Mh[mh3_index(0, set, wv, lane)] |= (uint32_t)code << (2 * j);
        }
    }
    for (int t = 0; t < 16; ++t) for (int j = 0; j < 16; ++j) {
        int code; C yh;
        hermitian_entry_t<R>(y.data(), mask.data(), t + 16 * j, 128, yh, code);
        Ys[t + 16 * j] = yh;
        Ms[t] |= (uint32_t)code << (2 * j);
    }
    // ---- state in slice order ---------------------------------------------------------------------
    std::vector<float> zs(N), ws(N);
    for (int row = 0; row < 256; ++row) for (int n = 0; n < 256; ++n) { zs[sl_state_index(row, n)] = z[row * 256 + n]; ws[sl_state_index(row, n)] = w[row * 256 + n]; }
    auto lane_access = [](int r, int t, int q, int k) { return (size_t)512 * r + 64 * q + 4 * t + k; };
    // ---- prologue: every resident access goes to its home; one owner per resident float, none left out, one home per w element
    std::vector<float> w_hbm = ws;
    {
        std::vector<char> covered(N, 0);
        int units = 0;
        for (int set = 0; set < SL_SETS; ++set) for (int q = 0; q < 8; ++q) units += w_home(set, q) != W_HBM;
        for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) {
            std::vector<char> slot_hit(4 * (SL_NREG > 0 ? SL_NREG : 1), 0);
            for (int set = 0; set < SL_SETS; ++set) for (int q = 0; q < 8; ++q) {
                const int home = w_home(set, q), r = sl_unit(set, wv, lane), t = lane & 15;
                if (home == W_HBM) continue;
                for (int k = 0; k < 4; ++k) {
                    int word;
                    float* at = w_at_home(set, wv, lane, q, k, &word);
                    if (home == W_LDS) { if (WRITER[word] != -1) fail(21); WRITER[word] = 64 * wv + lane; }
                    else { const int i = 4 * sl_reg_slot(set, q) + k; if (i < 0 || i >= 4 * SL_NREG || slot_hit[i]) fail(21); slot_hit[i] = 1; }
                    const size_t e = lane_access(r, t, q, k);
                    if (covered[e]) fail(28);
                    covered[e] = 1;
                    *at = w_hbm[e];
                    ws[e] = NAN;                                                      // the HBM copy is stale from here to the flush
                }
            }
            for (int i = 0; i < 4 * SL_NREG; ++i) if (!slot_hit[i]) fail(23);
        }
        for (int i = SL2_RES0 / 4; i < SL2_RES0 / 4 + (SLICE_RESIDENT ? SL_RES * 512 : 0); ++i) if (WRITER[i] == -1) fail(23);
        for (int i = SL2_RES1 / 4; i < SL2_RES1 / 4 + SL_NLDS1 * 2048; ++i) if (WRITER[i] == -1) fail(23);
        size_t n = 0;
        for (int i = 0; i < N; ++i) n += covered[i];
        if (n != (size_t)units * 2048) fail(29);
    }
    // ---- rows (first): v = z - w, forward transform ------------------------------------------------
    for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) for (int set = 0; set < SL_SETS; ++set) {
        const int r = sl_unit(set, wv, lane), t = lane & 15;
        for (int j = 0; j < 16; ++j) {
            const size_t ia = sl_state_index(2 * r, t + 16 * j), ib = sl_state_index(2 * r + 1, t + 16 * j);
            F[wv][lane][set][j] = mk<R>(zs[ia] - w_hbm[ia], zs[ib] - w_hbm[ib]);
        }
    }
    for (int wv = 0; wv < SL_WAVES; ++wv) for (int set = 0; set < SL_SETS; ++set) for (int g = 0; g < 4; ++g) group_fft(wv, g, set, false);

    const R ch = 0.5f * cdc, scale = 1.0f / 65536.0f, cs = cdc * scale, chs = ch * scale;
    const int buf = SL2_XB / 8;                                                      // the buffer in complex words
    for (int it = 0; it < iters; ++it) {
        const bool last = it + 1 == iters;
        // ---- T1: pass p in two halves; half h = row pairs 64 h .. 64 h + 63 = registers 8 h .. 8 h + 7 of the column ----------
        for (int p = 0; p < 4; ++p) for (int h = 0; h < 2; ++h) {
            phase(SL2_XB, SL_BUF8 * 8);
            int written = 0;
            for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) for (int s = 0; s < 2; ++s) {
                const int set = 2 * h + s, r = sl_unit(set, wv, lane), t = lane & 15;
                if ((r >> 6) != h) fail(44);
                for (int j = 0; j < 16; ++j) {
                    const int k = t + 16 * j;
                    if (sl_pass4(k) != p) continue;
                    if (sl_slot4(k) < 0 || sl_slot4(k) >= SL_P4) fail(43);
                    t_write_c(buf + sl_row8(r) * SL_P4 + sl_slot4(k), 64 * wv + lane, F[wv][lane][set][j], sl_slot4(k) >= SL_M4);
                    ++written;
                }
            }
            if (written != 64 * 64) fail(44);
            C own[8][64][8];
            for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) {
                const int cc = 4 * wv + (lane >> 4), t = lane & 15, odd = t & 1;
                for (int k = 0; k < 8; ++k) {
                    const int r = (t + 16 * (8 * h + k)) >> 1;                       // = (t >> 1) + 8 k + 64 h
                    if (sl_row8(r) != (t >> 1) + 8 * k || (r >> 6) != h) fail(44);
                    own[wv][lane][k] = t_read_c(buf + sl_row8(r) * SL_P4 + cc + (odd ? SL_M4 : 0));
                }
            }
            for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) for (int k = 0; k < 8; ++k) {
                const C o = own[wv][lane][k], other = own[wv][lane ^ 1][k];
                const int odd = lane & 1;
                C v = mk<R>(o.x + other.y, o.y - other.x);                             // twice the unpacked value
                if (sl_unit(p, wv, lane) == 0) v = odd ? mk<R>(other.y, o.x) : mk<R>(o.x, other.y);       // packed column: raw values
                G[wv][lane][p][8 * h + k] = v;
            }
        }
        memcpy(F, G, sizeof(F));
        // ---- columns -------------------------------------------------------------------------------
        for (int wv = 0; wv < SL_WAVES; ++wv) for (int set = 0; set < SL_SETS; ++set) {
            for (int g = 0; g < 4; ++g) group_fft(wv, g, set, false);
            for (int g = 0; g < 4; ++g) {
                if (sl_unit(set, wv, 16 * g) == 0) {
                    // the packed column borrows the wave's whole region: 256 values and a wrap-around copy of the first 16, as complex
                    if (wv != 0 || g != 0) fail(44);
                    wave_phase(wv);
                    const int cb = wave_words(wv) / 2;
                    for (int t = 0; t < 16; ++t) {
                        for (int j = 0; j < 16; ++j) t_write_c(cb + t + 16 * j, t, F[wv][t][set][j], false);
                        t_write_c(cb + 256 + t, t, F[wv][t][set][0], false);
                    }
                    C out[16][16];
                    for (int t = 0; t < 16; ++t) for (int j = 0; j < 16; ++j) {
                        const int k1 = t + 16 * j;
                        const C gk = F[wv][t][set][j], gm = t_read_c(cb + (16 - t) + 16 * (15 - j));
                        const C chk = F[wv][((256 - k1) & 255) & 15][set][((256 - k1) & 255) >> 4];
                        if (gm.x != chk.x || gm.y != chk.y) fail(45);                  // the mirror address delivers G[-k1]
                        const C A = blend_scaled(unpack_a(gk, gm), Yh[yh3_index(0, set, j, wv, t)], (int)((Mh[mh3_index(0, set, wv, t)] >> (2 * j)) & 3u), cs, chs, scale);
                        const C Bv = blend_scaled(unpack_b(gk, gm), Ys[k1], (int)((Ms[t] >> (2 * j)) & 3u), cs, chs, scale);
                        out[t][j] = repack_p(A, Bv);
                    }
                    for (int t = 0; t < 16; ++t) for (int j = 0; j < 16; ++j) F[wv][t][set][j] = out[t][j];
                } else {
                    for (int t = 0; t < 16; ++t) for (int j = 0; j < 16; ++j) {
                        const int lane = 16 * g + t;
                        F[wv][lane][set][j] = blend_scaled(F[wv][lane][set][j], Yh[yh3_index(0, set, j, wv, lane)],
                                                           (int)((Mh[mh3_index(0, set, wv, lane)] >> (2 * j)) & 3u), cs, (R)0.5 * chs, (R)0.5 * scale);
                    }
                }
            }
            for (int g = 0; g < 4; ++g) group_fft(wv, g, set, true);
        }
        // ---- T2: the way back, same halves -------------------------------------------------------------
        for (int p = 0; p < 4; ++p) for (int h = 0; h < 2; ++h) {
            phase(SL2_XB, SL_BUF8 * 8);
            for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) {
                const int cc = 4 * wv + (lane >> 4), t = lane & 15, odd = t & 1;
                for (int k = 0; k < 8; ++k) {
                    const int j = 8 * h + k, r = (t + 16 * j) >> 1;
                    const C own = F[wv][lane][p][j], other = F[wv][lane ^ 1][p][j];
                    C v = mk<R>(own.x - other.y, own.y + other.x);
                    if (sl_unit(p, wv, lane) == 0) v = odd ? mk<R>(own.y, other.y) : mk<R>(own.x, other.x);
                    t_write_c(buf + sl_row8(r) * SL_P4 + cc + (odd ? SL_M4 : 0), 64 * wv + lane, v, false);
                }
            }
            int got_n = 0;
            for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) for (int s = 0; s < 2; ++s) {
                const int set = 2 * h + s, r = sl_unit(set, wv, lane), t = lane & 15;
                for (int j = 0; j < 16; ++j) {
                    const int k = t + 16 * j;
                    if (sl_pass4(k) != p) continue;
                    const C got = t_read_c(buf + sl_row8(r) * SL_P4 + sl_slot4(k));
                    G[wv][lane][set][j] = sl_slot4(k) >= SL_M4 ? mk<R>(got.y, got.x) : got;
                    ++got_n;
                }
            }
            if (got_n != 64 * 64) fail(44);
        }
        memcpy(F, G, sizeof(F));
        // ---- rows: inverse transform, (last: x through the regions in two halves,) prox at the units' homes, v = z - w, forward transform
        for (int wv = 0; wv < SL_WAVES; ++wv) for (int set = 0; set < SL_SETS; ++set) {
            for (int g = 0; g < 4; ++g) group_fft(wv, g, set, true);
            if (last) for (int h = 0; h < 2; ++h) {
                wave_phase(wv);
                for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 16; ++j) {
                    const C o = F[wv][lane][set][j];
                    t_write(wave_words(wv) + (lane >> 4) * SL_XREGION + (lane & 15) + 16 * j, 64 * wv + lane, std::fabs(h ? o.y : o.x));
                }
                for (int lane = 0; lane < 64; ++lane) for (int i = 0; i < 4; ++i) for (int k = 0; k < 4; ++k) {
                    const int row = 2 * (32 * set + 4 * wv + i) + h, n = 4 * lane + k;
                    if (!std::isnan(x[row * 256 + n])) fail(46);                       // every pixel of x once
                    x[row * 256 + n] = t_read(wave_words(wv) + i * SL_XREGION + 4 * lane + k);
                }
            }
            for (int lane = 0; lane < 64; ++lane) {
                const int r = sl_unit(set, wv, lane), t = lane & 15;
                for (int j = 0; j < 16; ++j) {
                    const C o = F[wv][lane][set][j];
                    const size_t ia = sl_state_index(2 * r, t + 16 * j), ib = sl_state_index(2 * r + 1, t + 16 * j);
                    const R xa = std::fabs(o.x), xb = std::fabs(o.y);
                    int wa_word, wb_word;
                    float* ha = w_at_home(set, wv, lane, j >> 1, 2 * (j & 1), &wa_word);
                    float* hb = w_at_home(set, wv, lane, j >> 1, 2 * (j & 1) + 1, &wb_word);
                    if ((wa_word >= 0 && WRITER[wa_word] != 64 * wv + lane) || (wb_word >= 0 && WRITER[wb_word] != 64 * wv + lane)) fail(31);
                    float& wa = ha ? *ha : ws[ia];
                    float& wb = hb ? *hb : ws[ib];
                    if (cnc) { prox_cnc_pt(xa, zs[ia], wa, pc); prox_cnc_pt(xb, zs[ib], wb, pc); }
                    else     { prox_l1_pt(xa, zs[ia], wa, pc);  prox_l1_pt(xb, zs[ib], wb, pc); }
                    F[wv][lane][set][j] = mk<R>(zs[ia] - wa, zs[ib] - wb);
                }
            }
            for (int g = 0; g < 4; ++g) group_fft(wv, g, set, false);
        }
    }
    // ---- flush: the resident units return to HBM, every lane the accesses it owns ---------------------
    for (int wv = 0; wv < SL_WAVES; ++wv) for (int lane = 0; lane < 64; ++lane) for (int set = 0; set < SL_SETS; ++set)
        for (int q = 0; q < 8; ++q) for (int k = 0; k < 4; ++k) {
            int word;
            const float* at = w_at_home(set, wv, lane, q, k, &word);
            if (!at) continue;
            if (word >= 0 && WRITER[word] != 64 * wv + lane) fail(31);
            const size_t e = lane_access(sl_unit(set, wv, lane), lane & 15, q, k);
            if (!std::isnan(ws[e])) fail(32);
            ws[e] = *at;
        }
    for (int i = 0; i < N; ++i) if (std::isnan(ws[i]) || std::isnan(x[i])) fail(25);
    for (int row = 0; row < 256; ++row) for (int n = 0; n < 256; ++n) { z[row * 256 + n] = zs[sl_state_index(row, n)]; w[row * 256 + n] = ws[sl_state_index(row, n)]; }
    FILE* o = fopen(argv[2], "wb");
    std::vector<double> d(3 * N);
    for (int i = 0; i < N; ++i) { d[i] = x[i]; d[N + i] = z[i]; d[2 * N + i] = w[i]; }
    fwrite(d.data(), 8, d.size(), o);
    fclose(o);
    return 0;
}
