// The denoisers' conv layers (pnp_conv* / pnp_ffdnet* / pnp_relayout_c64; kernels_conv*.hip, kernels_pix2x2*.hip): what a caller may pass
// and how a launch is laid out -- tile sizes, the shape check of every layer kind, tiles / items, the persistent grid, the choice between
// the wide and the narrow f16x3 kernel.  Plain C++17 without HIP: api_conv.hip turns a failed check into the message, the launchers fill
// their *Args from here and launch nothing the check refuses, the kernels' headers take their tile constants from here, and
// tests/host/conv_plan_emulation.cpp runs all of it under g++ and the sanitizers.
//
// The three arithmetic families (float32, f16x3, f16) share the shapes: activations NHWC in blocks of 64 channels, an ITEM = one output
// tile x one block of 64 output channels (or matrix columns), persistent workgroups that stride through the items.
#pragma once

namespace pnp {

// ---- geometry ---------------------------------------------------------------------------------------------------------------------
struct ConvTile { int tx, ty; };                            // output pixels of a tile: columns, rows
constexpr ConvTile CP_NARROW = {16, 8};                     // k_conv3x3_c64, k_conv3x3_c64_h3, k_conv3x3_f16 and the first / last layer kernels
constexpr ConvTile CP_WIDE = {16, 16};                      // k_conv3x3_h3w (dilation 1 only)
constexpr ConvTile CP_PIX2 = {16, 8};                       // k_pix2x2_h3, k_pix2x2_f16: tiles of the coarser of the two pixel grids
constexpr int CP_CSTEP = 64;                                // channels of a block: C is a multiple of it (128 for the transposed 2 x 2 layer)
constexpr int CP_CMIN = 64, CP_CMAX = 1024;
constexpr int CP_MAX_CIN = 8, CP_MAX_COUT = 4;              // first layer: cin -> 64, last layer: 64 -> cout
constexpr int CP_MAX_DIL = 4;                               // dilation = width of the halo; above 1 at C = 64 only

// The size bound.  The kernels address a tensor through a buffer descriptor of H W pix bytes with ONE signed 32-bit byte offset and test
// columns only: a halo row above the image has a negative offset, a halo or overhang row below it an offset of at least H W pix -- both
// out of the descriptor's range, where loads return zeros and stores are dropped -- PROVIDED the offset of the lowest row a tile forms
// does not wrap around 2^32 back into range.  The lowest row (image height H, last tile at y0 <= H - 1):
//     narrow kernels, dilation d     staging y0 - d .. y0 + 7 + d  <= H + 6 + d <= H + 10;   epilogue <= y0 + 7 <= H + 6
//     wide kernel                    staging y0 - 1 .. y0 + 16     <= H + 15;                epilogue <= y0 + 15 <= H + 14
//     first / last layer kernels     staging y0 - 1 .. y0 + 8      <= H + 7;                 stores <= H + 6 (or tested against H)
//     2 x 2 kernels                  rows are tested against the grid: none beyond H - 1
// so with CP_SPARE_ROWS = 16 rows more than the image below 2^31 bytes every offset is below 2^31 or negative.  Taken on the float32
// size of the tensor (pix = 4 C) for all three families: a half tensor has the smaller offsets.
constexpr int CP_SPARE_ROWS = 16;
constexpr long long CP_MAX_BYTES = 0x7fffffffLL;
constexpr int cp_div_up(int a, int b) { return (a + b - 1) / b; }
// the lowest row a tile of an H-row image addresses (halo rows on either side)
constexpr int cp_max_row(int H, ConvTile t, int halo) { return (cp_div_up(H, t.ty) - 1) * t.ty + t.ty - 1 + halo; }
static_assert(cp_max_row(1, CP_WIDE, 1) < 1 + CP_SPARE_ROWS && cp_max_row(1, CP_NARROW, CP_MAX_DIL) < 1 + CP_SPARE_ROWS, "a tile's lowest row must lie within the spare rows");
// (H + CP_SPARE_ROWS) W C 4 <= CP_MAX_BYTES, without overflow for any int H, W >= 1 and C >= 1
constexpr bool cp_fits(int H, int W, int C) { return ((long long)H + CP_SPARE_ROWS) * W <= CP_MAX_BYTES / (4LL * C); }

// ---- tiles, items, grid -------------------------------------------------------------------------------------------------------------
struct ConvTiling {
    int tiles_x, tiles_y;
    long long items;                                        // n images x tiles x blocks
};
constexpr ConvTiling cp_tiling(int n, int H, int W, ConvTile t, int blocks = 1) {
    return {cp_div_up(W, t.tx), cp_div_up(H, t.ty), (long long)n * cp_div_up(W, t.tx) * cp_div_up(H, t.ty) * blocks};
}
constexpr bool cp_items_ok(long long items) { return items >= 1 && items <= 0x7fffffffLL; }     // the kernels count items in an int
// Persistent workgroups: `wps` per compute unit, rounded down to a multiple of the nc blocks (workgroup b strides by the grid and so keeps
// block b % nc: its weights stay in cache), at least nc, never more than the items (a multiple of nc themselves).  nc = 1: min(items, wps cus).
constexpr long long cp_grid(long long items, int wps, int cus, int nc = 1) {
    long long grid = (long long)wps * cus;
    grid -= grid % nc;
    if (grid < nc) grid = nc;
    return items < grid ? items : grid;
}

// ---- shape checks: CP_OK or which rule fails --------------------------------------------------------------------------------------
enum ConvWhy { CP_OK = 0, CP_DIMS, CP_CHANNELS, CP_CHANNELS_UP, CP_DILATION, CP_FMT, CP_CIN, CP_COUT, CP_ODD, CP_SIZE, CP_ITEMS, CP_SHUFFLE };

constexpr bool cp_channels_ok(int C, int step = CP_CSTEP) { return C >= CP_CMIN && C <= CP_CMAX && C % step == 0; }
// n images of H x W x C (C valid): at least one pixel, the size bound, the item bound for tile t
constexpr ConvWhy cp_check_image(int n, int C, int H, int W, ConvTile t = CP_NARROW) {
    if (n < 1 || H < 1 || W < 1) return CP_DIMS;
    if (!cp_fits(H, W, C)) return CP_SIZE;
    return cp_items_ok(cp_tiling(n, H, W, t, C / CP_CSTEP).items) ? CP_OK : CP_ITEMS;
}
// 3 x 3, C -> C, any family; fmt: the family's mask of three tensor-format bits
constexpr ConvWhy cp_check_body(int n, int C, int H, int W, int dilation, int fmt) {
    if (!cp_channels_ok(C)) return CP_CHANNELS;
    if (dilation < 1 || dilation > CP_MAX_DIL || (C != CP_CSTEP && dilation != 1)) return CP_DILATION;
    if (fmt & ~7) return CP_FMT;
    return cp_check_image(n, C, H, W);
}
// first layer (cin -> 64) and last layer (64 -> cout) at H x W
constexpr ConvWhy cp_check_head(int n, int cin, int H, int W) {
    if (cin < 1 || cin > CP_MAX_CIN) return CP_CIN;
    return cp_check_image(n, CP_CSTEP, H, W);
}
// shuffle_h, shuffle_w != 0: the four channels leave as ONE pixel-shuffled channel of that size, cropped (FFDNet)
constexpr ConvWhy cp_check_tail(int n, int cout, int H, int W, int shuffle_h = 0, int shuffle_w = 0) {
    if (cout < 1 || cout > CP_MAX_COUT) return CP_COUT;
    if ((shuffle_h || shuffle_w) && (cout != 4 || shuffle_h < 1 || shuffle_w < 1 || (shuffle_h + 1) / 2 != H || (shuffle_w + 1) / 2 != W)) return CP_SHUFFLE;
    return cp_check_image(n, CP_CSTEP, H, W);
}
// FFDNet's first and last layer on an h x w image: the layers run at ceil(h / 2) x ceil(w / 2)
constexpr int cp_ffdnet_dim(int full) { return full / 2 + (full & 1); }
constexpr ConvWhy cp_check_ffdnet(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1) return CP_DIMS;
    return cp_check_image(n, CP_CSTEP, cp_ffdnet_dim(h), cp_ffdnet_dim(w));
}

// 2 x 2 stride-2 convolution C -> 2 C (up = false: H, W even) and transposed convolution C -> C / 2 (up = true) of n images H x W x C
struct Pix2Plan {
    int Hout, Wout, Cout;
    int GH, GW;                                             // the tiled grid: the coarser side (down: the output, up: the input)
    int KC, NB;                                             // chunks of 64 along K (even), blocks of 64 matrix columns
    ConvTiling t;
};
constexpr Pix2Plan cp_pix2_plan(int n, int C, int H, int W, bool up) {
    const int GH = up ? H : H / 2, GW = up ? W : W / 2, NB = 2 * C / CP_CSTEP;
    return {up ? 2 * H : H / 2, up ? 2 * W : W / 2, up ? C / 2 : 2 * C, GH, GW, (up ? C : 4 * C) / CP_CSTEP, NB, cp_tiling(n, GH, GW, CP_PIX2, NB)};
}
constexpr ConvWhy cp_check_pix2(int n, int C, int H, int W, bool up) {
    if (n < 1 || H < 1 || W < 1) return CP_DIMS;
    if (!cp_channels_ok(C)) return up ? CP_CHANNELS_UP : CP_CHANNELS;
    if (!up && ((H | W) & 1)) return CP_ODD;
    if (!cp_fits(H, W, C)) return CP_SIZE;                                   // (first: it bounds H and W for what follows)
    if (up ? !cp_fits(2 * H, 2 * W, C / 2) : !cp_fits(H / 2, W / 2, 2 * C)) return CP_SIZE;
    if (up && !cp_channels_ok(C, 2 * CP_CSTEP)) return CP_CHANNELS_UP;       // (behind the sizes, which are defined for every multiple of 64)
    return cp_items_ok(cp_pix2_plan(n, C, H, W, up).t.items) ? CP_OK : CP_ITEMS;
}

// weight packs: 3 x 3 (C -> C) and 2 x 2 (down / up)
constexpr ConvWhy cp_check_pack3(int C) { return cp_channels_ok(C) ? CP_OK : CP_CHANNELS; }
constexpr ConvWhy cp_check_pack2(int C, bool up) { return cp_channels_ok(C, up ? 2 * CP_CSTEP : CP_CSTEP) ? CP_OK : up ? CP_CHANNELS_UP : CP_CHANNELS; }
// NCHW <-> NHWC of n images H x W x 64: the kernel takes the pixel count as an int and rounds it up to 64
constexpr ConvWhy cp_check_relayout(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1) return CP_DIMS;
    return (long long)H * W <= 0x7fffffffLL - 63 ? CP_OK : CP_ITEMS;
}

// ---- wide or narrow (f16x3, dilation 1) -------------------------------------------------------------------------------------------------
// mode 1: always wide, 0: never, -1: by size -- wide (ONE workgroup per compute unit) once every compute unit has a wide item of its own;
// below that the narrow tiles on two workgroups per unit spread a small layer better
constexpr bool cp_use_wide(int mode, int dilation, int n, int C, int H, int W, int cus) {
    if (dilation != 1 || mode == 0) return false;
    return mode > 0 || cp_tiling(n, H, W, CP_WIDE, C / CP_CSTEP).items >= cus;
}

}  // namespace pnp
