// C ABI of the denoisers' conv layers (include/pnp_mri.h: pnp_conv*, pnp_ffdnet*, pnp_relayout_c64): no context, caller-owned device
// tensors.  Every entry point is three steps: null / alias checks (NEED), the shape check of conv_plan.h turned into a message (PLAN), the
// launch (LAUNCH: PNP_OK, or PNP_E_HIP with the runtime's message).
// Host-side only; the kernels live in kernels_conv*.hip and kernels_pix2x2*.hip.
#include "../../include/pnp_mri.h"
#include "internal.h"
#include "conv_plan.h"

using namespace pnp;

// the plan's reason as the error of entry point `who`; a, b: dilation and fmt (body), cin (first layer), cout (last layer)
static int plan_error(const char* who, int why, int C, int H, int W, int a = 0, int b = 0) {
    switch (why) {
    case CP_DIMS:        return fail(PNP_E_ARG, "%s: n, H, W must be >= 1", who);
    case CP_CHANNELS:    return fail(PNP_E_ARG, "%s: C must be a multiple of 64 in 64..1024 (got %d)", who, C);
    case CP_CHANNELS_UP: return fail(PNP_E_ARG, "%s: C must be a multiple of 128 in 64..1024 (got %d)", who, C);
    case CP_DILATION:    return fail(PNP_E_ARG, "%s: dilation 1..4 at C = 64, 1 otherwise (got %d)", who, a);
    case CP_FMT:         return fail(PNP_E_ARG, "%s: fmt is a mask of the three tensor-format bits (got %d)", who, b);
    case CP_CIN:         return fail(PNP_E_ARG, "%s: 1 <= cin <= %d required (got %d)", who, CP_MAX_CIN, a);
    case CP_COUT:        return fail(PNP_E_ARG, "%s: 1 <= cout <= %d required (got %d)", who, CP_MAX_COUT, a);
    case CP_ODD:         return fail(PNP_E_ARG, "%s: H and W must be even (got %d x %d)", who, H, W);
    case CP_SIZE:        return fail(PNP_E_ARG, "%s: an image of %d x %d x %d values (or its result; + %d rows) exceeds the 2 GiB a float32 tensor of it may take",
                                     who, H, W, C, CP_SPARE_ROWS);
    case CP_ITEMS:       return fail(PNP_E_ARG, "%s: images of %d x %d x %d make more than 2^31 work items", who, H, W, C);
    default:             return fail(PNP_E_ARG, "%s: invalid shape", who);
    }
}
#define NEED(ok, what) do { if (!(ok)) return fail(PNP_E_ARG, "%s: " what, __func__); } while (0)
#define PLAN(check, ...) do { if (int why_ = (check)) return plan_error(__func__, why_, __VA_ARGS__); } while (0)
#define LAUNCH(call) do { HIPCHK(call); return PNP_OK; } while (0)
#define HALO_ALIAS "y must not alias x or skip (tiles read their neighbours' halo)"

extern "C" {

/* ---- float32 matrix cores (kernels_conv.hip) ---- */
int pnp_conv3x3_c64_nhwc(void* stream, const float* x, const float* w, const float* bias, const float* skip, float* y,
                         int n, int H, int W, int relu, int dilation) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && skip != y, HALO_ALIAS);
    PLAN(cp_check_body(n, 64, H, W, dilation, 0), 64, H, W, dilation);
    LAUNCH(launch_conv3x3_c64((hipStream_t)stream, x, w, bias, skip, y, n, H, W, relu, dilation));
}
int pnp_conv3x3_c64_pack(void* stream, const float* w_oihw, float* w_packed) {
    NEED(w_oihw && w_packed && w_oihw != w_packed, "null or aliased pointers");
    LAUNCH(launch_conv_pack_w((hipStream_t)stream, w_oihw, w_packed));
}
int pnp_conv3x3_head_nhwc(void* stream, const float* x, const float* w, const float* bias, float* y, int n, int cin, int H, int W, int relu) {
    NEED(x && w && y, "null pointer");
    PLAN(cp_check_head(n, cin, H, W), 64, H, W, cin);
    LAUNCH(launch_conv3x3_head((hipStream_t)stream, x, w, bias, y, n, cin, H, W, relu));
}
int pnp_conv3x3_tail_nchw(void* stream, const float* x, const float* w, const float* bias, float* y, int n, int cout, int H, int W) {
    NEED(x && w && y, "null pointer");
    PLAN(cp_check_tail(n, cout, H, W), 64, H, W, cout);
    LAUNCH(launch_conv3x3_tail((hipStream_t)stream, x, w, bias, y, n, cout, H, W));
}
int pnp_ffdnet_head_nhwc(void* stream, const float* x, const float* sigma, int sigma_per_image, const float* w, const float* bias, float* y,
                         int n, int h, int wd, int relu) {
    NEED(x && sigma && w && y, "null pointer");
    PLAN(cp_check_ffdnet(n, h, wd), 64, cp_ffdnet_dim(h), cp_ffdnet_dim(wd));
    LAUNCH(launch_ffdnet_head((hipStream_t)stream, x, sigma, sigma_per_image != 0, w, bias, y, n, h, wd, relu));
}
int pnp_relayout_c64(void* stream, const float* in, float* out, int n, int H, int W, int to_nhwc) {
    NEED(in && out && in != out, "null or aliased pointers");
    PLAN(cp_check_relayout(n, H, W), 64, H, W);
    LAUNCH(launch_relayout64((hipStream_t)stream, in, out, n, H * W, to_nhwc != 0));
}

/* ---- split-half arithmetic (kernels_conv_f16x3.hip, its _wide variant, kernels_pix2x2_f16x3.hip) ---- */
int pnp_conv3x3_nhwc_f16x3_fmt(void* stream, const float* x, const float* w, const float* bias, const float* skip, float* y,
                               int n, int C, int H, int W, int relu, int dilation, int fmt) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && skip != y, HALO_ALIAS);
    PLAN(cp_check_body(n, C, H, W, dilation, fmt), C, H, W, dilation, fmt);
    LAUNCH(launch_conv3x3_f16x3((hipStream_t)stream, x, w, bias, skip, y, n, C, H, W, relu, dilation, fmt));
}
int pnp_conv3x3_c64_nhwc_f16x3(void* stream, const float* x, const float* w, const float* bias, const float* skip, float* y,
                               int n, int H, int W, int relu, int dilation) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && skip != y, HALO_ALIAS);
    PLAN(cp_check_body(n, 64, H, W, dilation, 0), 64, H, W, dilation);
    LAUNCH(launch_conv3x3_f16x3((hipStream_t)stream, x, w, bias, skip, y, n, 64, H, W, relu, dilation));
}
int pnp_conv3x3_nhwc_f16x3(void* stream, const float* x, const float* w, const float* bias, const float* skip, float* y,
                           int n, int C, int H, int W, int relu) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && skip != y, HALO_ALIAS);
    PLAN(cp_check_body(n, C, H, W, 1, 0), C, H, W, 1);
    LAUNCH(launch_conv3x3_f16x3((hipStream_t)stream, x, w, bias, skip, y, n, C, H, W, relu, 1));
}
int pnp_conv3x3_f16x3_set_variant(int variant) { return conv_set_wide_mode(variant); }
int pnp_conv3x3_pack_f16x3(void* stream, const float* w_oihw, float* w_packed, int C) {
    NEED(w_oihw && w_packed && w_oihw != w_packed, "null or aliased pointers");
    PLAN(cp_check_pack3(C), C, 0, 0);
    LAUNCH(launch_conv_pack_w_f16x3((hipStream_t)stream, w_oihw, w_packed, C));
}
int pnp_conv3x3_c64_pack_f16x3(void* stream, const float* w_oihw, float* w_packed) {
    NEED(w_oihw && w_packed && w_oihw != w_packed, "null or aliased pointers");
    LAUNCH(launch_conv_pack_w_f16x3((hipStream_t)stream, w_oihw, w_packed, 64));
}
int pnp_conv3x3_tail_nchw_f16x3(void* stream, const float* x, const float* w, const float* bias, float* y, int n, int cout, int H, int W) {
    NEED(x && w && y, "null pointer");
    PLAN(cp_check_tail(n, cout, H, W), 64, H, W, cout);
    LAUNCH(launch_conv3x3_tail_f16x3((hipStream_t)stream, x, nullptr, w, bias, y, n, cout, H, W));
}
int pnp_conv3x3_tail_add_nchw_f16x3(void* stream, const float* x, const float* x2, const float* w, const float* bias, float* y, int n, int cout,
                                    int H, int W) {
    NEED(x && x2 && w && y, "null pointer");
    NEED(x != y && x2 != y, "y must not alias x or x2");
    PLAN(cp_check_tail(n, cout, H, W), 64, H, W, cout);
    LAUNCH(launch_conv3x3_tail_f16x3((hipStream_t)stream, x, x2, w, bias, y, n, cout, H, W));
}
int pnp_ffdnet_tail_f16x3(void* stream, const float* x, const float* w, const float* bias, float* y, int n, int h, int wd) {
    NEED(x && w && y, "null pointer");
    PLAN(cp_check_ffdnet(n, h, wd), 64, cp_ffdnet_dim(h), cp_ffdnet_dim(wd));
    LAUNCH(launch_conv3x3_tail_f16x3((hipStream_t)stream, x, nullptr, w, bias, y, n, 4, cp_ffdnet_dim(h), cp_ffdnet_dim(wd), h, wd));
}
#define PIX2_ALIAS "y must not alias x or x2 (tiles are re-read after their neighbours were written)"
int pnp_conv2x2s2_nhwc_f16x3(void* stream, const float* x, const float* x2, const float* w, float* y, int n, int C, int H, int W) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && x2 != y, PIX2_ALIAS);
    PLAN(cp_check_pix2(n, C, H, W, false), C, H, W);
    LAUNCH(launch_pix2x2_f16x3((hipStream_t)stream, x, x2, w, y, n, C, H, W, 0));
}
int pnp_convT2x2s2_nhwc_f16x3(void* stream, const float* x, const float* x2, const float* w, float* y, int n, int C, int H, int W) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && x2 != y, PIX2_ALIAS);
    PLAN(cp_check_pix2(n, C, H, W, true), C, H, W);
    LAUNCH(launch_pix2x2_f16x3((hipStream_t)stream, x, x2, w, y, n, C, H, W, 1));
}
int pnp_conv2x2_pack_f16x3(void* stream, const float* w, float* w_packed, int C, int transposed) {
    NEED(w && w_packed && w != w_packed, "null or aliased pointers");
    PLAN(cp_check_pack2(C, transposed != 0), C, 0, 0);
    LAUNCH(launch_pix2_pack_w_f16x3((hipStream_t)stream, w, w_packed, C, transposed != 0));
}

/* ---- the same layers in half precision (added after ABI 13, additive): kernels_conv_f16.hip, kernels_pix2x2_f16.hip ---- */
int pnp_conv3x3_nhwc_f16(void* stream, const void* x, const void* w, const float* bias, const void* skip, void* y,
                         int n, int C, int H, int W, int relu, int dilation, int fmt) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && skip != y, HALO_ALIAS);
    PLAN(cp_check_body(n, C, H, W, dilation, fmt), C, H, W, dilation, fmt);
    LAUNCH(launch_conv3x3_f16((hipStream_t)stream, x, w, bias, skip, y, n, C, H, W, relu, dilation, fmt));
}
int pnp_conv3x3_pack_f16(void* stream, const float* w_oihw, void* w_packed, int C) {
    NEED(w_oihw && w_packed && (const void*)w_oihw != w_packed, "null or aliased pointers");
    PLAN(cp_check_pack3(C), C, 0, 0);
    LAUNCH(launch_conv_pack_w_f16((hipStream_t)stream, w_oihw, w_packed, C));
}
int pnp_conv3x3_head_nhwc_f16(void* stream, const float* x, const float* w, const float* bias, void* y, int n, int cin, int H, int W, int relu) {
    NEED(x && w && y, "null pointer");
    PLAN(cp_check_head(n, cin, H, W), 64, H, W, cin);
    LAUNCH(launch_conv3x3_head_f16((hipStream_t)stream, x, nullptr, 0, w, bias, y, n, cin, H, W, relu, 0));
}
int pnp_ffdnet_head_nhwc_f16(void* stream, const float* x, const float* sigma, int sigma_per_image, const float* w, const float* bias, void* y,
                             int n, int h, int wd, int relu) {
    NEED(x && sigma && w && y, "null pointer");
    PLAN(cp_check_ffdnet(n, h, wd), 64, cp_ffdnet_dim(h), cp_ffdnet_dim(wd));
    LAUNCH(launch_conv3x3_head_f16((hipStream_t)stream, x, sigma, sigma_per_image != 0, w, bias, y, n, 5, h, wd, relu, 1));
}
int pnp_conv3x3_tail_nchw_f16(void* stream, const void* x, const void* x2, const float* w, const float* bias, float* y, int n, int cout, int H, int W) {
    NEED(x && w && y, "null pointer");
    NEED(x != (const void*)y && x2 != (const void*)y, "y must not alias x or x2");
    PLAN(cp_check_tail(n, cout, H, W), 64, H, W, cout);
    LAUNCH(launch_conv3x3_tail_f16((hipStream_t)stream, x, x2, w, bias, y, n, cout, H, W));
}
int pnp_ffdnet_tail_f16(void* stream, const void* x, const float* w, const float* bias, float* y, int n, int h, int wd) {
    NEED(x && w && y, "null pointer");
    PLAN(cp_check_ffdnet(n, h, wd), 64, cp_ffdnet_dim(h), cp_ffdnet_dim(wd));
    LAUNCH(launch_conv3x3_tail_f16((hipStream_t)stream, x, nullptr, w, bias, y, n, 4, cp_ffdnet_dim(h), cp_ffdnet_dim(wd), h, wd));
}
int pnp_conv2x2s2_nhwc_f16(void* stream, const void* x, const void* x2, const void* w, void* y, int n, int C, int H, int W, int y_f32) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && x2 != y, "y must not alias x or x2");
    PLAN(cp_check_pix2(n, C, H, W, false), C, H, W);
    LAUNCH(launch_pix2x2_f16((hipStream_t)stream, x, x2, w, y, n, C, H, W, 0, y_f32));
}
int pnp_convT2x2s2_nhwc_f16(void* stream, const void* x, const void* x2, const void* w, void* y, int n, int C, int H, int W, int y_f32) {
    NEED(x && w && y, "null pointer");
    NEED(x != y && x2 != y, "y must not alias x or x2");
    PLAN(cp_check_pix2(n, C, H, W, true), C, H, W);
    LAUNCH(launch_pix2x2_f16((hipStream_t)stream, x, x2, w, y, n, C, H, W, 1, y_f32));
}
int pnp_conv2x2_pack_f16(void* stream, const float* w, void* w_packed, int C, int transposed) {
    NEED(w && w_packed && (const void*)w != w_packed, "null or aliased pointers");
    PLAN(cp_check_pack2(C, transposed != 0), C, 0, 0);
    LAUNCH(launch_pix2_pack_w_f16((hipStream_t)stream, w, w_packed, C, transposed != 0));
}

}  // extern "C"
