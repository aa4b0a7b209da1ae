// g++ emulation of the host-testable parts of the convergence trace (csrc/trace_plan.h, kernels_trace.hip):
//   trace_emulation plan ITERS EVERY     prints "checks C", then per check "leg PRE ITER" (trace_leg)
//   trace_emulation slice IN OUT         the slice-order flavour of the reduction (k_residuals_slice) walked workgroup by workgroup, thread
//                                        by thread: IN = int32 B, int32 pad (floats), then x, z, z_prev, w [B][65536] float32 in NATURAL
//                                        order and gt [B][65536] uint8; the program lays z, z_prev, w out as the slice-resident kernel does
//                                        (sl_state_index of the whole slice, stride 65536 + pad, the padding poisoned with NaN), then forms
//                                        the TRACE_Q sums exactly as the kernel addresses them -- tiles of four row pairs, x scattered into a
//                                        tile buffer by the tile-local index map, z read by 16-byte access -- accumulating in long double.
//                                        OUT = [TRACE_Q][B] float64.  Exit 2 when an address leaves its slice's 65536 floats or a tile-buffer
//                                        element is written twice or never.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "../../pnp_admm_cnc_mri_amd/csrc/slice_layout.h"
#include "../../pnp_admm_cnc_mri_amd/csrc/trace_plan.h"

using namespace pnp;

static int plan(int iters, int every) {
    const int checks = trace_checks(iters, every);
    printf("checks %d\n", checks);
    for (int c = 0; c < checks; ++c) {
        const TraceLeg leg = trace_leg(iters, every, c);
        if (leg.iter != trace_check_iter(iters, every, c)) return 2;
        printf("leg %d %d\n", leg.pre, leg.iter);
    }
    return 0;
}

static int slice(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 1;
    int32_t hdr[2];
    if (fread(hdr, sizeof(int32_t), 2, f) != 2) return 1;
    const int B = hdr[0];
    const size_t N = 65536, pad = (size_t)hdr[1], stride = N + pad;
    std::vector<float> nat[4];
    for (auto& a : nat) { a.resize((size_t)B * N); if (fread(a.data(), sizeof(float), a.size(), f) != a.size()) return 1; }
    std::vector<uint8_t> gt((size_t)B * N);
    if (fread(gt.data(), 1, gt.size(), f) != gt.size()) return 1;
    fclose(f);
    const std::vector<float>& x = nat[0];
    std::vector<float> st[3];                                              // z, z_prev, w in slice order, padded
    for (int a = 0; a < 3; ++a) {
        st[a].assign((size_t)B * stride, std::numeric_limits<float>::quiet_NaN());
        for (int b = 0; b < B; ++b)
            for (int row = 0; row < 256; ++row)
                for (int n = 0; n < 256; ++n) st[a][(size_t)b * stride + sl_state_index(row, n)] = nat[a + 1][(size_t)b * N + (size_t)row * 256 + n];
    }
    const int groups = trace_groups(B, N);
    const size_t span = trace_span(B, N);
    if (span % TRACE_TILE != 0 || (size_t)groups * span < N) return 2;
    std::vector<double> res((size_t)TRACE_Q * B);
    for (int b = 0; b < B; ++b) {
        long double s[TRACE_Q] = {};
        for (int g = 0; g < groups; ++g) {
            const size_t lo = (size_t)g * span, hi = lo + span < N ? lo + span : N;
            for (size_t base = lo; base < hi; base += TRACE_TILE) {
                float xt[TRACE_TILE];
                int written[TRACE_TILE] = {};
                for (int tid = 0; tid < TRACE_THREADS; ++tid)
                    for (int u = 0; u < 2; ++u) {
                        const int fa = tid + TRACE_THREADS * u, row = fa >> 6, n0 = 4 * (fa & 63);
                        for (int k = 0; k < 4; ++k) {
                            const size_t i = base + 4 * (size_t)fa + k;
                            if (i >= N) return 2;
                            const float xv = x[(size_t)b * N + i];
                            const size_t at = sl_state_index(row, n0 + k);
                            if (at >= (size_t)TRACE_TILE) return 2;
                            xt[at] = xv; ++written[at];
                            s[TR_X] += (long double)xv * xv;
                            const long double gv = gt[(size_t)b * N + i], d = (long double)((double)xv * 255.0) - gv;
                            s[TR_E] += d * d; s[TR_G] += gv * gv;
                        }
                    }
                for (int i = 0; i < TRACE_TILE; ++i) if (written[i] != 1) return 2;
                for (int tid = 0; tid < TRACE_THREADS; ++tid)
                    for (int u = 0; u < 2; ++u) {
                        const int fa = tid + TRACE_THREADS * u;
                        for (int k = 0; k < 4; ++k) {
                            const size_t i = base + 4 * (size_t)fa + k;
                            if (i >= N) return 2;                          // never into the padding
                            const long double xs = xt[4 * fa + k], z = st[0][(size_t)b * stride + i], zp = st[1][(size_t)b * stride + i],
                                              w = st[2][(size_t)b * stride + i];
                            s[TR_XZ] += (xs - z) * (xs - z); s[TR_ZZP] += (z - zp) * (z - zp); s[TR_Z] += z * z; s[TR_W] += w * w;
                        }
                    }
            }
        }
        for (int q = 0; q < TRACE_Q; ++q) res[(size_t)q * B + b] = (double)s[q];
    }
    FILE* o = fopen(out, "wb");
    if (!o) return 1;
    fwrite(res.data(), sizeof(double), res.size(), o);
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "plan")) return plan(atoi(argv[2]), atoi(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "slice")) return slice(argv[2], argv[3]);
    fprintf(stderr, "usage: trace_emulation plan ITERS EVERY | slice IN OUT\n");
    return 1;
}
