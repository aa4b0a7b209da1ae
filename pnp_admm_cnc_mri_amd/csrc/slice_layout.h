// Index maps of the slice-resident 256x256 kernel (kernels_slice256.hip), shared with the g++ host
// emulations (tests/host/slice_resident_emulation.cpp: two-pass form; slice_resident4_emulation.cpp: four-pass form + resident w;
// slice_resident_units_emulation.cpp: the resident units of w; slice_split_emulation.cpp: the plane-split exchange, the eighth passes and
// the LDS map of k_slice<2>).
//
// One 512-thread workgroup (8 waves, 2 per SIMD, 256 VGPRs each) keeps ONE real slice on a compute
// unit for a whole ADMM run: the 65536 values live in the register file (128 VGPRs per thread, four
// "register sets" of 16 complex values) as 128 complex rows or 128 complex columns of 256, and only
// z, w (and the Hermitian measurement table) travel to HBM.
//
//   row form   : row pair r = 0..127 carries c_r[n] = v[2r][n] + i v[2r+1][n]; its transform C_r[k]
//                is held by the 16 lanes of a group as C_r[t + 16 j] (lane t, register j).
//                thread (wave wv, lane l), register set s:  r = 32 s + 4 wv + (l >> 4),  t = l & 15
//   column form: column c = 0..127; c >= 1 is k-space column k2 = c of the real slice's row
//                transforms V_rho[k2] (rho = 0..255), c = 0 packs the two real columns k2 = 0 and
//                k2 = 128 as V_rho[0] + i V_rho[128].  Same thread shape:
//                c = 32 s + 4 wv + (l >> 4),  lane t holds rho (or k1) = t + 16 j
//
// Row form <-> column form goes through LDS in two passes (the buffer holds half the field; the ADMM_L1 instances) or in
// four (a quarter; ADMM_CNC, whose freed LDS keeps part of w on the compute unit -- a quarter as whole row pairs, SL_RES, and
// further (register set, access) units in LDS and in registers: SL_P4 ... the table sl_units_lds / sl_units_reg below; each of the
// four passes crosses in two halves, and the transforms exchange in two planes: "LDS OF k_slice<2>" below).  Two passes:
//   pass p moves the columns c = 64 p .. 64 p + 63 (register sets 2p and 2p + 1 of the column form).  A row pair needs, per column c, C_r[c] and its
//   mirror C_r[256 - c] (for c = 0: C_r[0] and C_r[128]) because
//     V_2r[k2] = (C_r[k2] + conj C_r[-k2]) / 2,   V_2r+1[k2] = (C_r[k2] - conj C_r[-k2]) / (2i)
//   buffer element (r, slot): slot = c - 64 p for the direct value, SL_M + c - 64 p for the mirror.
// The way back is the exact mirror: the thread pair (rho = 2r, 2r+1) of column c forms
//   D_r[c] = U_2r + i U_2r+1 (direct slot) and D_r[256 - c] = conj U_2r + i conj U_2r+1 (mirror slot).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fft16.h"

namespace pnp {

constexpr int SL_P = 132;     // pitch (complex) of a row pair in the transposition buffer; 132 % 32 == 4:
                              // 8 consecutive row pairs x 2 neighbouring columns hit 16 distinct 8-byte banks
constexpr int SL_M = 66;      // mirrored half starts here; 66 % 4 == 2 keeps direct / mirror stores of a lane pair apart
constexpr int SL_BUF = 128 * SL_P;                       // complex elements of the transposition buffer

// pass in which k-space column k (0..255) of a row pair crosses, and its slot
PNP_HD int sl_pass(int k) { return (k < 64 || k > 192 || k == 128) ? 0 : 1; }
PNP_HD int sl_slot(int k) {
    if (k < 64) return k;                      // pass 0, direct:  c = k
    if (k == 128) return SL_M;                 // pass 0, partner of the packed column c = 0
    if (k > 192) return SL_M + 256 - k;        // pass 0, mirror of c = 256 - k = 1..63
    if (k < 128) return k - 64;                // pass 1, direct:  c = k = 64..127
    return SL_M + 192 - k;                     // pass 1, mirror of c = 256 - k = 64..127  (k = 129..192)
}
// FOUR-pass form (ADMM_CNC, k_slice<2>): pass q moves the columns c = 32 q .. 32 q + 31 = register set q of the column form, so
// a pass moves a quarter of the field -- 128 row pairs x pitch 68 x 8 B = 69 632 bytes; the kernel crosses it in two halves of 64 row
// pairs (sl_row8 below) -- and LDS has room for SL_RES row pairs of w that stay on the compute unit for a whole launch (below).
//   slot of (r, c): c - 32 q direct, SL_M4 + c - 32 q mirror (k = 256 - c; for c = 0: k = 128).  Register j of lane t holds
//   k = t + 16 j, so pass q takes registers 2q, 2q + 1 (direct) and 15 - 2q, 14 - 2q (mirror) -- except in lane 0 of a group,
//   whose register 14 - 2q holds k = 224 - 32 q, the mirror of column 32 (q + 1): it crosses one pass later (k = 224, 192, 160),
//   and lane 0's k = 128 (register 8) partners the packed column c = 0 in pass 0.
constexpr int SL_P4 = 68;     // pitch; 68 % 32 == 4, the bank property of SL_P
constexpr int SL_M4 = 34;     // mirrored half; 34 % 4 == 2 as SL_M
constexpr int SL_BUF4 = 128 * SL_P4;
PNP_HD int sl_pass4(int k) { return k == 128 ? 0 : k < 128 ? (k >> 5) : ((256 - k) >> 5); }
PNP_HD int sl_slot4(int k) { return k == 128 ? SL_M4 : k < 128 ? (k & 31) : SL_M4 + ((256 - k) & 31); }
// thread shape shared by both forms
constexpr int SL_WAVES = 8, SL_SETS = 4;
// Resident w: the row pairs r = 0 .. SL_RES - 1 (register set 0 of the row form: 4 wave + group, the same share for every
// wave) keep w in LDS between the iterations of a launch, in the order of a row pair in HBM (sl_state_index): the lane's
// q-th 16-byte access of row pair r starts at float sl_res_index(r, t, q) of the region.  A lane reads back what it wrote.
constexpr int SL_RES = 32;
PNP_HD int sl_res_index(int r, int t, int q) { return 512 * r + 64 * q + 4 * t; }
// Residency is counted in UNITS: unit (s, q) = the q-th 16-byte access of register set s -- the same instruction slot in every
// lane of every wave, for the workgroup 8 KiB = the q-th eighth (256 bytes) of each of the set's 32 row pairs.  Whether a
// unit's w lives in HBM, in LDS or in registers is a compile-time property of that slot (the table sl_units_lds / sl_units_reg
// below): no wave-dependent choice.  The region above is the units (0, 0) .. (0, 7).  The units (1, q) that
// stay in LDS follow it in a second region of SL_RES1 units x 2048 floats, numbered u = 0 .. SL_RES1 - 1 by rising q: the
// access of row pair 32 + rr (rr = 4 wave + group = 0..31) and lane t starts at float sl_res1_index(u, rr, t) -- a wave's
// 64 lanes read 1 KiB contiguous.  A lane reads back what it wrote.
#ifndef SLICE_RES1_UNITS
#define SLICE_RES1_UNITS 7        // size of the second region: what the compute unit's LDS has room for (the arms of the A/B: 6, 2)
#endif
constexpr int SL_RES1 = SLICE_RES1_UNITS;
PNP_HD int sl_res1_index(int u, int rr, int t) { return 2048 * u + 64 * rr + 4 * t; }
// The table: which units are resident, and where (compile-time knobs of the kernel; the host emulation reads the same table).
#ifndef SLICE_RESIDENT
#define SLICE_RESIDENT 1    // k_slice<2>: part of w stays on the compute unit for a launch, by (register set, access) units -- set 0 in LDS and the units of the
#endif                      // two masks below (0: no residency at all, four-pass transpositions alone; 2: set 0 only, the kernel before the unit form: the arms of the A/B)
#ifndef SLICE_UNITS_LDS1
#define SLICE_UNITS_LDS1 0x7F       // bit q: unit (1, q) of w lives in the second LDS region (at most SL_RES1 units)
#endif
#ifndef SLICE_UNITS_REG
#define SLICE_UNITS_REG 0x03000000  // bit 8 s + q: unit (s, q) of w lives in four registers of every lane across the iteration loop (default: (3, 0), (3, 1))
#endif
constexpr int popc8(unsigned m) { int n = 0; for (int i = 0; i < 8; ++i) n += (m >> i) & 1; return n; }
constexpr unsigned sl_units_lds(int set) { return SLICE_RESIDENT == 0 ? 0u : set == 0 ? 0xFFu : (SLICE_RESIDENT == 1 && set == 1) ? (SLICE_UNITS_LDS1 & 0xFFu) : 0u; }
constexpr unsigned sl_units_reg(int set) { return SLICE_RESIDENT == 1 && set < SL_SETS ? ((unsigned)SLICE_UNITS_REG >> (8 * set)) & 0xFFu & ~sl_units_lds(set) : 0u; }
enum { W_HBM = 0, W_LDS = 1, W_REG = 2 };                  // where the w of a unit is between the iterations of a launch
constexpr int w_home(int set, int q) { return ((sl_units_lds(set) >> q) & 1) ? W_LDS : ((sl_units_reg(set) >> q) & 1) ? W_REG : W_HBM; }
// register unit (set, q): its place among the lane's resident registers
constexpr int sl_reg_slot(int set, int q) {
    int n = 0;
    for (int s = 0; s < set; ++s) n += popc8(sl_units_reg(s));
    return n + (set < SL_SETS ? popc8(sl_units_reg(set) & ((1u << q) - 1)) : 0);
}
constexpr int SL_NREG = sl_reg_slot(SL_SETS, 0);         // register units
constexpr int SL_NLDS1 = popc8(sl_units_lds(1));          // LDS units of set 1
static_assert(SL_NLDS1 <= SL_RES1, "the second resident region holds SL_RES1 units");

// LDS OF k_slice<2>, HALVED TRANSIENTS.  The room for SL_RES1 = 7 units comes from the two transient users of LDS:
//   exchange in two planes: a 16-lane transform group swaps its 16 x 16 complex values through a region of 16 rows of FLOATS, the real
//     parts first and then the imaginary parts through the same words.  Lane t writes its k-th value to float sl_xw(k, t) and reads its
//     row, the floats sl_xw(t, 0 .. 15), one dword per access, each straight into the half of the register pair it belongs to.  Pitch 17
//     and regions of 272 floats: the 32 lanes of a dword access (two groups; bank = word mod 32) hit 32 distinct banks both ways --
//     17 t mod 32 is the even banks 0 .. 14 and the odd ones 17 .. 31, the next group's region starts 16 banks further.
//   eighth passes: a transposition pass q (sl_pass4 / sl_slot4 above: same passes, same slots) crosses in two halves, row pairs
//     0 .. 63 (register sets 0, 1 of the row form = registers j < 8 of the column form) and 64 .. 127; the buffer holds 64 row pairs at
//     pitch SL_P4, row pair r in row sl_row8(r) of half r >> 6.  Every lane stores 8 values and reads 8 in each half.
constexpr int SL_XP = 17;
constexpr int SL_XREGION = 16 * SL_XP;                     // floats of one transform group's region (holds one plane of a row pair in natural order: 256)
constexpr int SL_XWAVE = 4 * SL_XREGION;                   // floats of a wave's private region (holds the packed column and its wrap-around copy: 2 x 272)
PNP_HD int sl_xw(int k, int t) { return SL_XP * k + t; }
constexpr int SL_BUF8 = 64 * SL_P4;                        // complex elements of the eighth-pass buffer
PNP_HD int sl_row8(int r) { return r & 63; }
// The map, in bytes, each area behind the one before it (no two can overlap) -- the host emulations check it again:
//   exchange regions of the 8 waves / the buffer that aliases them | W256 table (16 rows of 18 complex) | Ys (256 complex) + Ms (64 words) |
//   resident w: set 0 (SL_RES row pairs) | the LDS units of set 1 (SL_RES1 x 8 KiB)
constexpr int sl_max(int a, int b) { return a > b ? a : b; }
constexpr int SL2_XB = 0,             SL2_XB_BYTES = sl_max(SL_WAVES * SL_XWAVE * 4, SL_BUF8 * 8);
constexpr int SL2_TW = SL2_XB + SL2_XB_BYTES,     SL2_TW_BYTES = 16 * 18 * 8;
constexpr int SL2_YS = SL2_TW + SL2_TW_BYTES,     SL2_YS_BYTES = (256 + 32) * 8;
constexpr int SL2_RES0 = SL2_YS + SL2_YS_BYTES,   SL2_RES0_BYTES = SL_RES * 2048;
constexpr int SL2_RES1 = SL2_RES0 + SL2_RES0_BYTES, SL2_RES1_BYTES = SL_RES1 * 8192;
constexpr int SL2_END = SL2_RES1 + SL2_RES1_BYTES;
constexpr int SL_LDS_CU = 163840;                          // LDS of a compute unit
static_assert(SL2_END <= SL_LDS_CU && SL2_TW % 16 == 0 && SL2_RES0 % 16 == 0, "LDS map of k_slice<2>");
static_assert(2 * SL_XREGION >= 272 && SL_XREGION >= 256 && SL_XREGION % 4 == 0, "what else lives in the exchange regions");

PNP_HD int sl_unit(int set, int wv, int lane) { return 32 * set + 4 * wv + (lane >> 4); }     // r or c

// per-slice operand tables in column-form thread order
//   Yh3 : [slice][set 4][wave 8][j/2 8][lane 64][j%2] complex   Yh at (k1 = t + 16 j, k2 = c); for c = 0: k2 = 0.
//         A wave's operands of a set are ONE contiguous 8 KiB block read by eight 16-byte-per-lane accesses (two j each)
//   Mh3 : [slice][set 4][wave 8][lane 64] u32, 2 bits per j = 2 Mh
//   Ys3 : [slice][256] complex, Ms3 : [slice][16] u32 -- the same for k2 = 128 (second half of c = 0), lane t, bits j
constexpr size_t YH3_SLICE = 4 * 16 * 8 * 64;
constexpr size_t MH3_SLICE = 4 * 8 * 64;
PNP_HD size_t yh3_index(int slice, int set, int j, int wv, int lane) {
    return (size_t)slice * YH3_SLICE + ((((size_t)set * 8 + wv) * 8 + (j >> 1)) * 64 + lane) * 2 + (j & 1);
}
PNP_HD size_t mh3_index(int slice, int set, int wv, int lane) { return (size_t)slice * MH3_SLICE + (((size_t)set * 8 + wv) * 64 + lane); }

// State arrays (z, w) of a slice-resident run live in HBM in "slice order": rows stay where they are, but the 512 values
// of a ROW PAIR r (image rows 2r, 2r + 1 = re / im of the packed complex row) are stored in the thread order of the row
// transform, so that the z-/w-update works on the transform's own registers (no natural-order staging through LDS) and
// every access is still a full 16-byte lane access of a 256-byte contiguous run per 16-lane group:
//   pixel n = t + 16 j of row 2r + sel  ->  float index  512 r + 64 (j >> 1) + 4 t + 2 (j & 1) + sel
// i.e. lane t's q-th 16-byte access (q = 0..7) holds (row 2r, row 2r+1) x (j = 2q, 2q + 1) = its registers a[2q], a[2q + 1].
// pnp_get_state / pnp_set_state / the other kernel families see the natural [256][256] order: api.hip converts in place
// (k_state_order) when a run switches families.  x is always natural.
PNP_HD size_t sl_state_index(int row, int n) {                 // within the slice's 65536 floats
    return (size_t)(row >> 1) * 512 + 64 * (n >> 5) + 4 * (n & 15) + 2 * ((n >> 4) & 1) + (row & 1);
}
// (A variant that interleaves the four row pairs of a wave's register set so that every wave access is 1 KiB contiguous
// instead of 4 x 256 bytes measured the same, 10.3 k it/s: the kernel is at the memory system's limit for its bytes.)

// the packed column c = 0 after its transform: G[k1] = A[k1] + i B[k1] with A, B the transforms of the
// REAL columns k2 = 0 and k2 = 128:  A = unpack_a(G[k1], G[-k1]),  B = unpack_b(G[k1], G[-k1]),
// and back  G' = repack_p(A', B') = A' + i B'   (fft16.h).

}  // namespace pnp
