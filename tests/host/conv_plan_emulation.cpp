// CPU driver of csrc/conv_plan.h (tests/test_conv_plan_host.py; g++ with the sanitizers): answers one request per line of stdin.
//   tiling KIND n C H W up wps cus mode dil   ->  tiles_x tiles_y items grid wide      KIND: narrow | wide | direct | pix2 | ffdnet
//   check KIND args..                         ->  the ConvWhy code                     KIND: body head tail ffdnet pix2 pack3 pack2 relayout
//   rows H W pix                              ->  one line per kernel geometry: name max_inside min_outside_u32 size lowest_row
// `rows` walks every tile of an H-row image and every row the geometry addresses (tile rows, halo rows on either side), at the first and the
// last image column and the first and last 16 bytes of a pixel of `pix` bytes, and forms the byte offset the way the kernels do: in 32 bits.
#include "../../pnp_admm_cnc_mri_amd/csrc/conv_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

using namespace pnp;

struct RowGeo { const char* name; ConvTile t; int halo; };

static void rows(int H, int W, int pix) {
    const RowGeo geos[] = {{"narrow_d1", CP_NARROW, 1}, {"narrow_d2", CP_NARROW, 2}, {"narrow_d3", CP_NARROW, 3}, {"narrow_d4", CP_NARROW, CP_MAX_DIL},
                           {"wide", CP_WIDE, 1}, {"pix2", CP_PIX2, 0}};
    const uint64_t size = (uint64_t)H * W * pix;
    for (const RowGeo& g : geos) {
        int64_t max_inside = -1;
        uint64_t min_outside = UINT64_MAX;
        int lowest = 0;
        for (int y0 = 0; y0 < H; y0 += g.t.ty)
            for (int r = -g.halo; r < g.t.ty + g.halo; ++r) {
                const int row = y0 + r;
                lowest = row > lowest ? row : lowest;
                for (int col : {0, W - 1})
                    for (int chunk : {0, pix - 16}) {
                        const int64_t off = ((int64_t)row * W + col) * pix + chunk;
                        const uint32_t off32 = (uint32_t)(uint64_t)off;              // what a 32-bit offset register holds
                        if (row >= 0 && row < H) {
                            if (off != (int64_t)off32) { std::printf("error: an inside offset left 32 bits\n"); return; }
                            max_inside = off > max_inside ? off : max_inside;
                        } else if (std::strcmp(g.name, "pix2") != 0) {               // the 2 x 2 kernels test their rows: none outside is formed
                            min_outside = off32 < min_outside ? off32 : min_outside;
                        }
                    }
            }
        if (lowest != cp_max_row(H, g.t, g.halo)) { std::printf("error: cp_max_row\n"); return; }
        std::printf("%s %lld %llu %llu %d\n", g.name, (long long)max_inside, (unsigned long long)min_outside, (unsigned long long)size, lowest);
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, kind;
        in >> cmd;
        if (cmd == "tiling") {
            int n, C, H, W, up, wps, cus, mode, dil;
            in >> kind >> n >> C >> H >> W >> up >> wps >> cus >> mode >> dil;
            ConvTiling t{};
            int nc = 1;
            if (kind == "narrow") { nc = C / CP_CSTEP; t = cp_tiling(n, H, W, CP_NARROW, nc); }
            else if (kind == "wide") { nc = C / CP_CSTEP; t = cp_tiling(n, H, W, CP_WIDE, nc); }
            else if (kind == "direct") t = cp_tiling(n, H, W, CP_NARROW);
            else if (kind == "ffdnet") t = cp_tiling(n, cp_ffdnet_dim(H), cp_ffdnet_dim(W), CP_NARROW);
            else if (kind == "pix2") { const Pix2Plan p = cp_pix2_plan(n, C, H, W, up != 0); nc = p.NB; t = p.t; }
            else return 2;
            std::printf("%d %d %lld %lld %d\n", t.tiles_x, t.tiles_y, t.items, cp_grid(t.items, wps, cus, nc), (int)cp_use_wide(mode, dil, n, C, H, W, cus));
        } else if (cmd == "check") {
            int a[6] = {0, 0, 0, 0, 0, 0};
            in >> kind;
            for (int& v : a) in >> v;
            int why = -1;
            if (kind == "body") why = cp_check_body(a[0], a[1], a[2], a[3], a[4], a[5]);
            else if (kind == "head") why = cp_check_head(a[0], a[1], a[2], a[3]);
            else if (kind == "tail") why = cp_check_tail(a[0], a[1], a[2], a[3], a[4], a[5]);
            else if (kind == "ffdnet") why = cp_check_ffdnet(a[0], a[1], a[2]);
            else if (kind == "pix2") why = cp_check_pix2(a[0], a[1], a[2], a[3], a[4] != 0);
            else if (kind == "pack3") why = cp_check_pack3(a[0]);
            else if (kind == "pack2") why = cp_check_pack2(a[0], a[1] != 0);
            else if (kind == "relayout") why = cp_check_relayout(a[0], a[1], a[2]);
            else return 2;
            std::printf("%d\n", why);
        } else if (cmd == "rows") {
            int H, W, pix;
            in >> H >> W >> pix;
            rows(H, W, pix);
        } else if (cmd == "constants") {
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", CP_NARROW.tx, CP_NARROW.ty, CP_WIDE.tx, CP_WIDE.ty, CP_PIX2.tx, CP_PIX2.ty, CP_CSTEP, CP_CMIN, CP_CMAX,
                        CP_MAX_CIN, CP_MAX_COUT, CP_SPARE_ROWS, CP_MAX_DIL);
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
