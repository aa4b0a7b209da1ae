// g++ emulation of the host-testable parts of the multi-coil data consistency (csrc/coil_plan.h):
//   coil_emulation walk H W C B Ks     forms every index the coil kernels form, the way they form it -- the expanding / combining rows of
//                                      kernels_anysize.hip (row -> slice and line, coil_id lookup, work and map offsets), the expanded mask
//                                      index of the column kernels' B * C pseudo-slices, the pointwise CG kernels' (workgroup, thread) ->
//                                      element map and their partial slots -- on arrays of EXACTLY the plan's sizes (the sanitizers see any
//                                      index outside).  Exit 2 when an element is visited twice or never, or a lookup disagrees.
//   coil_emulation sums                the two summation orders (cg_tree_sum, cg_wave_sum) on integer data (exact in any order) and on random
//                                      data against long double; cg_ratio's zero and non-finite cases; the launch counts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../pnp_admm_cnc_mri_amd/csrc/coil_plan.h"

using namespace pnp;

static int walk(int H, int W, int C, int B, int Ks) {
    if (coil_check(C, Ks, H, W) != COIL_OK) return 3;
    const size_t N = (size_t)H * W;
    std::vector<uint8_t> work(coil_work_elems(B, C, H, W), 0), maps(coil_map_elems(Ks, C, H, W), 0);
    std::vector<int32_t> coil_id((size_t)B), mask_id((size_t)B), mask_idx((size_t)B * C, -1);
    for (int b = 0; b < B; ++b) { coil_id[b] = (b * 5 + 1) % Ks; mask_id[b] = (b * 3 + 2) % 7; }
    // expanded mask index: one thread per pseudo-slice
    for (int s = 0; s < B * C; ++s) mask_idx[(size_t)s] = mask_id[(size_t)coil_pseudo_slice(s, C)];
    for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) if (mask_idx[(size_t)b * C + c] != mask_id[b]) return 2;
    // the rows, for several lines-per-workgroup G (the host picks 1 .. 16): row0 = block * G, rows past B * H are skipped
    for (int G : {1, 3, 16}) {
        std::fill(work.begin(), work.end(), 0);
        const int nrows = B * H, blocks = (nrows + G - 1) / G;
        for (int blk = 0; blk < blocks; ++blk)
            for (int c = 0; c < C; ++c)
                for (int i = 0; i < G * W; ++i) {
                    const int g = i / W, k = i - g * W, row = blk * G + g;
                    if (row >= nrows) continue;
                    const int b = coil_row_slice(row, H), h = coil_row_line(row, H);
                    if (b < 0 || b >= B || h < 0 || h >= H || b * H + h != row) return 2;
                    const int set = coil_set_of(coil_id.data(), b);
                    if (set != coil_id[b] || coil_set_of(nullptr, b) != 0) return 2;
                    const size_t wi = coil_work_index(b, c, C, h, k, H, W), mi = coil_map_index(set, c, C, h, k, H, W);
                    // the pseudo-slice view of the column kernels: slice s = b * C + c at stride N
                    if (wi != ((size_t)b * C + c) * N + (size_t)h * W + k) return 2;
                    ++work.at(wi);
                    maps.at(mi) = 1;
                }
        for (uint8_t v : work) if (v != 1) return 2;
    }
    // only the sets in use are touched, each of them completely
    for (int set = 0; set < Ks; ++set) {
        bool used = false;
        for (int b = 0; b < B; ++b) used = used || coil_id[b] == set;
        for (size_t i = 0; i < (size_t)C * N; ++i) if ((maps[(size_t)set * C * N + i] != 0) != used) return 2;
    }
    // pointwise CG kernels: grid (cg_blocks(N), B), thread t of block x takes lo + t, lo + t + 256, ... below lo + CG_SPAN and N
    const int nblk = cg_blocks(N);
    if ((size_t)nblk * CG_SPAN < N || (size_t)(nblk - 1) * CG_SPAN >= N) return 2;
    std::vector<uint8_t> img((size_t)B * N, 0);
    std::vector<uint8_t> part((size_t)B * nblk, 0), part_row((size_t)B * cg_row_partials(H), 0);
    for (int b = 0; b < B; ++b)
        for (int x = 0; x < nblk; ++x) {
            const size_t lo = (size_t)x * CG_SPAN;
            for (int t = 0; t < CG_THREADS; ++t)
                for (size_t i = lo + t; i < lo + CG_SPAN && i < N; i += CG_THREADS) ++img.at((size_t)b * N + i);
            ++part.at(cg_partial_index(b, x, nblk));
        }
    for (uint8_t v : img) if (v != 1) return 2;
    for (uint8_t v : part) if (v != 1) return 2;
    for (int row = 0; row < B * H; ++row) ++part_row.at((size_t)row);          // the combining rows: partial[row]
    for (int b = 0; b < B; ++b) for (int h = 0; h < H; ++h) if (part_row.at(cg_partial_index(b, h, cg_row_partials(H))) != 1) return 2;
    printf("ok %d %d %d blocks %d rows %d\n", H, W, C, nblk, cg_row_partials(H));
    return 0;
}

static int sums() {
    for (int n : {1, 16, 63, 64, 128, 131, 160, 255, 256, 257, 1024}) {
        std::vector<double> v((size_t)n);
        for (int i = 0; i < n; ++i) v[i] = (double)(i + 1);
        const double want = 0.5 * n * (n + 1.0);
        if (cg_tree_sum(v.data(), n) != want || cg_wave_sum(v.data(), n) != want) return 2;
        std::mt19937_64 rng(n);
        std::uniform_real_distribution<double> u(0.0, 1.0);
        long double ref = 0;
        for (int i = 0; i < n; ++i) { v[i] = u(rng); ref += v[i]; }
        if (std::fabs((double)(cg_tree_sum(v.data(), n) - ref)) > 1e-13 * (double)ref) return 2;
        if (std::fabs((double)(cg_wave_sum(v.data(), n) - ref)) > 1e-13 * (double)ref) return 2;
    }
    if (cg_ratio(0.0, 0.0) != 0.0 || cg_ratio(1.0, 0.0) != 0.0 || cg_ratio(6.0, 3.0) != 2.0) return 2;
    if (cg_ratio(1e300, 1e-300) != 0.0 || cg_ratio(NAN, 1.0) != 0.0) return 2;
    if (cg_launches(3) != 20 || cg_launches(1) != 10 || coil_iteration_launches(3, false) != 21 || coil_iteration_launches(3, true) != 22) return 2;
    if (coil_check(0, 1, 128, 128) != COIL_BAD_C || coil_check(33, 1, 128, 128) != COIL_BAD_C || coil_check(32, 0, 128, 128) != COIL_BAD_SETS ||
        coil_check(1, 1, 127, 128) != COIL_BAD_SHAPE || coil_check(32, 9, 1024, 128) != COIL_OK) return 2;
    printf("ok sums\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "walk")) return walk(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
    if (argc == 2 && !strcmp(argv[1], "sums")) return sums();
    fprintf(stderr, "usage: coil_emulation walk H W C B Ks | sums\n");
    return 1;
}
