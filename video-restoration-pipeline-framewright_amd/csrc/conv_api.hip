// The kernel-level C entries of the convolution kernels: the packers and one launch each, on the caller's buffers and stream,
// for tests, tools and the engines that sequence a network over the entries (restormer.hip, aesrgan.hip).  None takes an engine
// handle.  The kernels and their launchers: conv3x3_mfma.hip, conv3x3_pair*.hip, conv3x3_wino.hip, conv3x3_hr_last.hip,
// conv_up2x_phase.hip, frame_ops.hip.  No device code.
#include "fw_status.h"

using namespace fw;

namespace {

// a plane stride of 0 (or less) in the C-ABI: interleaved NHWC, a pixel's 32-channel chunks side by side
long plane_stride(long s) { return s > 0 ? s : 32; }

void fill_input(ConvParams& p, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int H, int W, const void* wpk, const float* bias) {
    p.in = x;
    p.in_cstride = in_cstride;
    p.in_pstride = plane_stride(in_plane_stride);
    p.cin_chunks = cin_chunks;
    p.H = H;
    p.W = W;
    p.wpk = wpk;
    p.bias = bias;
}

void fill_output(ConvParams& p, void* out, int out_cstride, long out_plane_stride, int out_coff) {
    p.out = out;
    p.out_cstride = out_cstride;
    p.out_pstride = plane_stride(out_plane_stride);
    p.out_coff = out_coff;
}

}  // namespace

extern "C" {

size_t fw_pack_conv3x3(int dtype, const float* weight, int cout, int cin, int cout_tiles, int cin_chunks,
                       uint16_t* dst) {
    if (cout < 1 || cin < 1 || cout_tiles < 1 || cin_chunks < 1 || cout > 32 * cout_tiles || cin > 32 * cin_chunks)
        return 0;
    if (dst && !weight) return 0;
    return pack_conv3x3_weights((DType)dtype, weight, cout, cin, cout_tiles, cin_chunks, dst);
}

int fw_conv3x3_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int H, int W,
                    const void* packed_weight, const float* bias, int cout_tiles, int act_lrelu, int upsample2x,
                    const float* res1, float s1, const float* res2, float s2, void* out, int out_cstride,
                    long out_plane_stride, int out_coff, float* out_f32, void* stream) {
    return fw_conv3x3_nhwc_ex(dtype, x, in_cstride, in_plane_stride, cin_chunks, H, W, packed_weight, bias, cout_tiles,
                              act_lrelu, upsample2x, res1, s1, res2, s2, nullptr, 0, 0, 0, out, out_cstride,
                              out_plane_stride, out_coff, out_f32, stream);
}

int fw_conv3x3_pair_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int in_chunks, int H, int W,
                         const void* packed_weight_a, const float* bias_a, const void* packed_weight_b, const float* bias_b,
                         void* out_a, void* out_b, int out_cstride, void* stream) {
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_conv3x3_pair_nhwc: bad dtype");
    return guarded([&] {
        ConvPairParams q{};
        q.in = x;
        q.in_cstride = in_cstride;
        q.in_pstride = plane_stride(in_plane_stride);
        q.na = in_chunks;
        q.H = H;
        q.W = W;
        q.wpk_a = packed_weight_a;
        q.bias_a = bias_a;
        q.wpk_b = packed_weight_b;
        q.bias_b = bias_b;
        q.out_a = out_a;
        q.out_b = out_b;
        q.out_cstride = out_cstride;
        // (a single pixel: the chunk-planar layout's plane stride H * W * 32 IS 32 and in_cstride addresses nothing, as in
        // launch_conv_up2x_phase)
        if (q.in_pstride == 32 && in_cstride < 32 * in_chunks && (long)H * W > 1)
            throw Error(FW_ERR_INVALID, "fw_conv3x3_pair_nhwc: input too narrow");
        launch_conv3x3_pair((DType)dtype, q, (hipStream_t)stream);
    });
}

int fw_conv3x3_nhwc_ex(int dtype, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int H, int W,
                       const void* packed_weight, const float* bias, int cout_tiles, int act_lrelu, int upsample2x,
                       const float* res1, float s1, const float* res2, float s2, const float* chan_scale, int post_act,
                       int f32_cstride, int f32_coff, void* out, int out_cstride, long out_plane_stride, int out_coff,
                       float* out_f32, void* stream) {
    if (!x || !packed_weight || !bias) return fail(FW_ERR_INVALID, "fw_conv3x3_nhwc: NULL argument");
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_conv3x3_nhwc: bad dtype");
    if (cout_tiles != 1 && cout_tiles != 2) return fail(FW_ERR_INVALID, "fw_conv3x3_nhwc: cout_tiles must be 1 or 2");
    if (res1 && cout_tiles != 2) return fail(FW_ERR_INVALID, "fw_conv3x3_nhwc: residual epilogue needs 64 channels");
    if (!res1 && res2) return fail(FW_ERR_INVALID, "fw_conv3x3_nhwc: res2 without res1");
    if (act_lrelu == 2 && (res1 || !chan_scale)) return fail(FW_ERR_INVALID, "fw_conv3x3_nhwc: PReLU needs slopes and no residual");
    return guarded([&] {
        ConvParams p{};
        fill_input(p, x, in_cstride, in_plane_stride, cin_chunks, H, W, packed_weight, bias);
        fill_output(p, out, out_cstride, out_plane_stride, out_coff);
        p.out_f32 = out_f32;
        p.res1 = res1;
        p.res2 = res2;
        p.s1 = s1;
        p.s2 = s2;
        p.act = act_lrelu;
        p.upsample2x = upsample2x;
        p.chan_scale = chan_scale;
        p.post_act = post_act;
        p.f32_cstride = f32_cstride;
        p.f32_coff = f32_coff;
        launch_conv3x3((DType)dtype, cout_tiles, res1 ? EPI_RESIDUAL : EPI_STORE, p, (hipStream_t)stream);
    });
}

size_t fw_pack_conv3x3_wino(int dtype, const float* weight, int cout, int cin, int cin_chunks, uint16_t* dst) {
    if (dtype != FW_DTYPE_F16) return 0;   // the Winograd kernel is f16 only
    if (cout < 1 || cin < 1 || cin_chunks < 1 || cout > 64 || cin > 32 * cin_chunks) return 0;
    if (dst && !weight) return 0;
    return pack_conv3x3_wino_weights(DT_F16, weight, cout, cin, cin_chunks, dst);
}

int fw_conv3x3_split_nhwc(int dtype, int winograd, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int H, int W,
                          const void* packed_weight, const float* bias, float s1, float in_id_scale, int n_id, const long* chunk_off,
                          const float* id_scale, int post_act, void* out, void* out_lo, int out_cstride, long out_plane_stride,
                          int out_coff, void* stream) {
    if (!x || !packed_weight || !bias || !out) return fail(FW_ERR_INVALID, "fw_conv3x3_split_nhwc: NULL argument");
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_conv3x3_split_nhwc: bad dtype");
    if (winograd != 0 && winograd != 1) return fail(FW_ERR_INVALID, "fw_conv3x3_split_nhwc: winograd must be 0 or 1");
    if (winograd && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_conv3x3_split_nhwc: the Winograd form is f16 only");
    if (n_id < 0 || n_id > 6) return fail(FW_ERR_INVALID, "fw_conv3x3_split_nhwc: n_id must be in [0, 6]");
    if (n_id > 0 && (!chunk_off || !id_scale)) return fail(FW_ERR_INVALID, "fw_conv3x3_split_nhwc: residual planes need chunk_off and id_scale");
    return guarded([&] {
        ConvParams p{};
        fill_input(p, x, in_cstride, in_plane_stride, cin_chunks, H, W, packed_weight, bias);
        p.s1 = s1;
        p.s2 = 1.f;
        p.in_id_scale = in_id_scale;
        p.n_id = n_id;
        for (int i = 0; i < n_id; ++i) {
            p.chunk_off[i] = chunk_off[i];
            p.id_scale[i] = id_scale[i];
        }
        p.post_act = post_act;
        fill_output(p, out, out_cstride, out_plane_stride, out_coff);
        p.out_lo = out_lo;
        if (winograd)
            launch_conv3x3_wino_split(p, (hipStream_t)stream);
        else
            launch_conv3x3((DType)dtype, 2, EPI_RESIDUAL_SPLIT, p, (hipStream_t)stream);
    });
}

size_t fw_pack_conv_last_pointwise(int dtype, const float* weight, uint16_t* dst) {
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return 0;
    if (dst && !weight) return 0;
    return pack_conv_last_pointwise((DType)dtype, weight, dst);
}

int fw_conv3x3_hr_last_nhwc(int dtype, int fused, const void* x, int in_cstride, long in_plane_stride, int H, int W,
                            const void* packed_w_hr, const float* bias_hr, const void* packed_w_last, const void* packed_w_last_pw,
                            const float* bias_last, void* scratch_u3, int img_H, int img_W, uint8_t* out_u8, uint16_t* out_u16,
                            float* out_rgb_f32, void* stream) {
    if (!x || !packed_w_hr || !bias_hr || !bias_last) return fail(FW_ERR_INVALID, "fw_conv3x3_hr_last_nhwc: NULL argument");
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_conv3x3_hr_last_nhwc: bad dtype");
    if (fused != 0 && fused != 1) return fail(FW_ERR_INVALID, "fw_conv3x3_hr_last_nhwc: fused must be 0 or 1");
    if (fused ? !packed_w_last_pw : (!packed_w_last || !scratch_u3))
        return fail(FW_ERR_INVALID, "fw_conv3x3_hr_last_nhwc: missing conv_last weights or scratch for this form");
    if (H < 1 || W < 1 || img_H < 1 || img_W < 1 || img_H > H || img_W > W) return fail(FW_ERR_INVALID, "fw_conv3x3_hr_last_nhwc: bad size");
    if (!out_u8 && !out_u16 && !out_rgb_f32) return fail(FW_ERR_INVALID, "fw_conv3x3_hr_last_nhwc: no output");
    return guarded([&] {
        ConvParams hr{};
        fill_input(hr, x, in_cstride, in_plane_stride, 2, H, W, packed_w_hr, bias_hr);
        hr.s1 = hr.s2 = 1.f;
        ConvParams img{};
        img.s1 = img.s2 = 1.f;
        img.out_u8 = out_u8;
        img.out_u16 = out_u16;
        img.out_rgb = out_rgb_f32;
        img.img_H = img_H;
        img.img_W = img_W;
        if (fused) {
            hr.out_u8 = out_u8;
            hr.out_u16 = out_u16;
            hr.out_rgb = out_rgb_f32;
            hr.img_H = img_H;
            hr.img_W = img_W;
            launch_conv3x3_hr_last((DType)dtype, hr, packed_w_last_pw, bias_last, (hipStream_t)stream);
            return;
        }
        const long plane = (long)H * W * 32;   // scratch_u3: two 32-channel planes [H][W][32]
        fill_output(hr, scratch_u3, 32, plane, 0);
        hr.act = 1;
        launch_conv3x3((DType)dtype, 2, EPI_STORE, hr, (hipStream_t)stream);
        fill_input(img, scratch_u3, 32, plane, 2, H, W, packed_w_last, bias_last);
        launch_conv3x3((DType)dtype, 1, EPI_IMAGE, img, (hipStream_t)stream);
    });
}

int fw_conv3x3_wino_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int H, int W,
                         const void* packed_weight, const float* bias, int act_lrelu, void* out, int out_cstride, long out_plane_stride,
                         int out_coff, void* stream) {
    if (!x || !packed_weight || !bias || !out) return fail(FW_ERR_INVALID, "fw_conv3x3_wino_nhwc: NULL argument");
    if (dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_conv3x3_wino_nhwc: the Winograd form is f16 only");
    if (act_lrelu != 0 && act_lrelu != 1) return fail(FW_ERR_INVALID, "fw_conv3x3_wino_nhwc: act_lrelu must be 0 or 1");
    return guarded([&] {
        ConvParams p{};
        fill_input(p, x, in_cstride, in_plane_stride, cin_chunks, H, W, packed_weight, bias);
        p.act = act_lrelu;
        fill_output(p, out, out_cstride, out_plane_stride, out_coff);
        launch_conv3x3_wino_store(p, (hipStream_t)stream);
    });
}

int fw_conv3x3_wino_check_fields(int* codes, int n) {
    // one valid problem per form, then one field at a time set to what the Winograd kernels do not implement (no launch, no device call)
    static const float one = 1.f;
    static char dummy[16];
    ConvParams ok{};
    ok.H = ok.W = 16;
    ok.cin_chunks = 2;
    ok.in_cstride = 32;
    ok.in_pstride = 16 * 16 * 32;
    ok.out = dummy;
    ok.out_cstride = 32;
    ok.out_pstride = 16 * 16 * 32;
    ok.s1 = 0.2f;
    ok.in_id_scale = 5.f;
    ok.n_id = 2;
    ok.id_scale[0] = ok.id_scale[1] = 5.f;
    ok.f32_native = 1;   // set for every conv of the engine; meaningless without fp32 side buffers, accepted
    struct Case { bool split; void (*set)(ConvParams&); };
    static const Case cases[] = {
        {true, [](ConvParams& p) { p.post_act = 1; }},
        {true, [](ConvParams& p) { p.chan_scale = &one; }},
        {true, [](ConvParams& p) { p.res1 = &one; }},
        {true, [](ConvParams& p) { p.res2 = &one; }},
        {true, [](ConvParams& p) { p.out_f32 = const_cast<float*>(&one); }},
        {true, [](ConvParams& p) { p.n_groups = 2; }},
        {true, [](ConvParams& p) { p.act = 1; }},
        {true, [](ConvParams& p) { p.in_id_scale = 0.1f; }},
        {true, [](ConvParams& p) { p.id_scale[1] = 0.1f; }},
        {false, [](ConvParams& p) { p.out_f32 = const_cast<float*>(&one); }},
        {false, [](ConvParams& p) { p.n_groups = 2; }},
        {false, [](ConvParams& p) { p.chan_scale = &one; }},
        {false, [](ConvParams& p) { p.post_act = 1; }},
        {false, [](ConvParams& p) { p.res1 = &one; }},
        {false, [](ConvParams& p) { p.act = 2; }},
        {false, [](ConvParams& p) { p.out_lo = dummy; }},
    };
    const int nc = (int)(sizeof(cases) / sizeof(cases[0]));
    ConvParams st = ok;
    st.n_id = 0;
    st.in_id_scale = 0.f;
    st.act = 1;
    try {   // the unmodified problems pass
        check_conv3x3_wino(ok, true);
        check_conv3x3_wino(st, false);
    } catch (const fw::Error& e) {
        fail(FW_ERR_INTERNAL, std::string("fw_conv3x3_wino_check_fields: a valid problem was rejected: ") + e.what());
        return -1;
    }
    for (int i = 0; i < nc && i < n; ++i) {
        ConvParams p = cases[i].split ? ok : st;
        cases[i].set(p);
        codes[i] = guarded([&] { check_conv3x3_wino(p, cases[i].split); });
    }
    return nc;
}

size_t fw_pack_conv_up2x_phase(int dtype, const float* weight, uint16_t* dst) {
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return 0;
    if (dst && !weight) return 0;
    return pack_conv_up2x_phase_weights((DType)dtype, weight, dst);
}

int fw_conv_up2x_phase_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int H, int W, const void* packed_weight,
                            const float* bias, int act_lrelu, void* out, int out_cstride, long out_plane_stride, void* stream) {
    if (!x || !packed_weight || !bias || !out) return fail(FW_ERR_INVALID, "fw_conv_up2x_phase_nhwc: NULL argument");
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_conv_up2x_phase_nhwc: bad dtype");
    if (H < 1 || W < 1) return fail(FW_ERR_INVALID, "fw_conv_up2x_phase_nhwc: bad size");
    return guarded([&] {
        ConvUpParams u{};
        u.in = x;
        u.in_cstride = in_cstride;
        u.in_pstride = plane_stride(in_plane_stride);
        u.H = H;
        u.W = W;
        u.wpk = packed_weight;
        u.bias = bias;
        u.act = act_lrelu;
        u.out = out;
        u.out_cstride = out_cstride;
        u.out_pstride = plane_stride(out_plane_stride);
        launch_conv_up2x_phase((DType)dtype, u, (hipStream_t)stream);
    });
}

int fw_u8_to_nhwc(int dtype, const uint8_t* in_bgr, int H, int W, void* out, int out_cstride, void* stream) {
    if (!in_bgr || !out || H < 1 || W < 1) return fail(FW_ERR_INVALID, "fw_u8_to_nhwc: bad argument");
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_u8_to_nhwc: bad dtype");
    return guarded([&] { launch_u8_to_nhwc((DType)dtype, in_bgr, H, W, out, out_cstride, 1, (hipStream_t)stream); });
}

int fw_pixel_shuffle_add_u8(const float* conv, int conv_cstride, const uint8_t* in_bgr, int H, int W, int scale,
                            uint8_t* out_bgr, float* out_rgb_f32, void* stream) {
    if (!conv || !in_bgr || (!out_bgr && !out_rgb_f32) || H < 1 || W < 1)
        return fail(FW_ERR_INVALID, "fw_pixel_shuffle_add_u8: bad argument");
    return guarded([&] {
        launch_pixel_shuffle_add(conv, conv_cstride, in_bgr, H, W, scale, out_bgr, out_rgb_f32, (hipStream_t)stream);
    });
}

}  // extern "C"
