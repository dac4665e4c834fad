// Compression-artifact removal, the classical path (kernel set K21 of DESIGN.md): the reference's processors/qp_artifact_removal.py
// with backend 'opencv' - `_remove_blocking_opencv`, `_remove_ringing_opencv`, `_remove_banding_opencv` in `_process_frame`'s order - on
// uint8 BGR frames that are already on the device.  tests/qp_artifact_ref.py states every step in numpy and is the contract, byte
// for byte; this file follows its float32 summation orders and its float32 / float64 promotions literally.
//
// Every a * b + c here must round twice, as numpy's does: the file is compiled with -ffp-contract=off (build.py PER_FILE_FLAGS).
// The Canny edge map is frame_ops.hip's (launch_canny_edge_map), unchanged; its hysteresis reads round flags on the host, so a call
// with the ringing step synchronises its stream.
#include <hip/hip_runtime.h>

#include "stage_common.h"

namespace fw {
namespace {

constexpr int QA_NT = 256;
constexpr int QA_TW = 32, QA_TH = 16;          // the bilateral's output tile: 256 lanes, two pixels a lane (rows ly and ly + 8)
constexpr int QA_MAX_R = 7;                    // d = int(5 + 10 strength) <= 15
constexpr int QA_BLOCKING = 1, QA_RINGING = 2, QA_BANDING = 4;

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// ---- cv2.bilateralFilter --------------------------------------------------------------------------------------------------------------
// One workgroup per 32 x 16 tile.  The tile and its R-pixel halo (REFLECT_101, reflected as often as it takes) are staged once in LDS
// as packed pixels b | g << 8 | r << 16, next to the 768-entry colour table and the (2R + 1)^2 space table.  A wave reads one tap of
// two tile rows at a time: 32 consecutive words a row, no bank conflict; the colour-table read is a gather and takes what conflicts
// the picture gives it.  A lane keeps the eight float32 chains of its two pixels going side by side.
// Order of the sums (tests/qp_artifact_ref.py): per window row a partial sum from 0, taps left to right; the row sums top to bottom.
__device__ __forceinline__ void bilateral_tap(uint32_t p, uint32_t c, float sw, const float* __restrict__ s_col, float* row) {
    const float w = sw * s_col[__builtin_amdgcn_sad_u8(p, c, 0u)];      // |db| + |dg| + |dr|: the fourth byte of both is 0
    row[0] += (float)(p & 255u) * w;
    row[1] += (float)((p >> 8) & 255u) * w;
    row[2] += (float)(p >> 16) * w;
    row[3] += w;
}

template <int R>
__global__ __launch_bounds__(QA_NT) void bilateral_u8c3_kernel(const uint8_t* __restrict__ src, int H, int W, const float* __restrict__ color_g,
                                                               const float* __restrict__ space_g, uint8_t* __restrict__ dst) {
    constexpr int LW = QA_TW + 2 * R, LH = QA_TH + 2 * R, D = 2 * R + 1;
    __shared__ uint32_t s_px[LH * LW];
    __shared__ float s_col[768];
    __shared__ float s_sp[D * D];
    const int tid = threadIdx.x, x0 = blockIdx.x * QA_TW, y0 = blockIdx.y * QA_TH;
    for (int k = tid; k < 768; k += QA_NT) s_col[k] = color_g[k];
    for (int k = tid; k < D * D; k += QA_NT) s_sp[k] = space_g[k];
    for (int k = tid; k < LH * LW; k += QA_NT) {
        const int yy = k / LW, xx = k - yy * LW;
        const uint8_t* p = src + ((size_t)reflect101(y0 + yy - R, H) * W + reflect101(x0 + xx - R, W)) * 3;
        s_px[k] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
    __syncthreads();
    const int lx = tid & 31, ly = tid >> 5;
    const uint32_t* centre = s_px + (ly + R) * LW + lx + R;
    const uint32_t c0 = centre[0], c1 = centre[8 * LW];
    float acc0[4] = {0.f, 0.f, 0.f, 0.f}, acc1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1   // unrolled over the rows, the small radii take hundreds of registers and one wave a SIMD
    for (int dy = -R; dy <= R; ++dy) {
        int hw = 0;                                                        // the circular support's half width on this row
        while ((hw + 1) * (hw + 1) + dy * dy <= R * R) ++hw;
        const uint32_t* r0 = centre + dy * LW;
        const float* sp = s_sp + (dy + R) * D + R;
        float row0[4] = {0.f, 0.f, 0.f, 0.f}, row1[4] = {0.f, 0.f, 0.f, 0.f};
        for (int dx = -hw; dx <= hw; ++dx) {
            const float sw = sp[dx];
            bilateral_tap(r0[dx], c0, sw, s_col, row0);
            bilateral_tap(r0[dx + 8 * LW], c1, sw, s_col, row1);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc0[i] += row0[i], acc1[i] += row1[i];
    }
    const int x = x0 + lx;
    if (x >= W) return;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int y = y0 + ly + 8 * q;
        if (y >= H) continue;
        const float* a = q ? acc1 : acc0;
        uint8_t* o = dst + ((size_t)y * W + x) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = (uint8_t)rintf(a[i] / a[3]);      // half to even; 0 .. 255: a weighted mean of bytes
    }
}

// ---- cv2.GaussianBlur(uint8, (5, 5), 0): ([1 4 6 4 1] x [1 4 6 4 1] + 128) >> 8 ---------------------------------------------------
struct Taps5 {
    int y[5], x[5];
};

__device__ __forceinline__ Taps5 taps5(int y, int x, int H, int W) {
    Taps5 t;
#pragma unroll
    for (int k = 0; k < 5; ++k) t.y[k] = reflect101(y + k - 2, H), t.x[k] = reflect101(x + k - 2, W);
    return t;
}

__device__ __forceinline__ void gauss5_px(const uint8_t* __restrict__ src, int W, const Taps5& t, int* out) {
    constexpr int K[5] = {1, 4, 6, 4, 1};
    int s[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        int r[3] = {0, 0, 0};
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const uint8_t* p = src + ((size_t)t.y[a] * W + t.x[b]) * 3;
            r[0] += K[b] * p[0], r[1] += K[b] * p[1], r[2] += K[b] * p[2];
        }
        s[0] += K[a] * r[0], s[1] += K[a] * r[1], s[2] += K[a] * r[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (s[c] + 128) >> 8;
}

#define QA_FOR_EACH_PIXEL(i, y, x)                                                                                          \
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x, n_ = (long)H * W; i < n_; i += (long)gridDim.x * blockDim.x) \
        if (const int y = (int)(i / W), x = (int)(i - (long)y * W); true)

__global__ __launch_bounds__(QA_NT) void gaussian5_u8_kernel(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        int g[3];
        gauss5_px(src, W, taps5(y, x, H, W), g);
        dst[i * 3] = (uint8_t)g[0], dst[i * 3 + 1] = (uint8_t)g[1], dst[i * 3 + 2] = (uint8_t)g[2];
    }
}

// ---- the block-boundary blend of `_remove_blocking_opencv` -----------------------------------------------------------------------
// mask = 1 on the rows y - 1 .. y + 1 around every multiple y of the block size below H (clipped to the frame), the same for columns
__device__ __forceinline__ bool on_boundary(int p, int len, int block) {
    const int r = p & (block - 1);                                         // the block size is a power of two
    return r <= 1 || (r == block - 1 && p + 1 < len);
}

// result * (1 - mask * strength * 0.5) + smooth * mask * strength * 0.5 in float64, truncated; mask is float32 0 or 1
__global__ __launch_bounds__(QA_NT) void boundary_blend_kernel(const uint8_t* __restrict__ filtered, const uint8_t* __restrict__ frame, int H,
                                                               int W, int block, double strength, uint8_t* __restrict__ dst) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        if (!on_boundary(y, H, block) && !on_boundary(x, W, block)) {      // mask 0: result * 1.0 + 0.0
            dst[i * 3] = filtered[i * 3], dst[i * 3 + 1] = filtered[i * 3 + 1], dst[i * 3 + 2] = filtered[i * 3 + 2];
            continue;
        }
        int g[3];
        gauss5_px(frame, W, taps5(y, x, H, W), g);
        const double keep = 1.0 - (double)1.0f * strength * 0.5;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = (double)filtered[i * 3 + c] * keep + (double)((float)g[c] * 1.0f) * strength * 0.5;
            dst[i * 3 + c] = (uint8_t)v;
        }
    }
}

// ---- `_remove_ringing_opencv` ------------------------------------------------------------------------------------------------------
// ring = dilate(edges, 3 x 3, twice) - edges: a pixel that is no edge and has an edge in its 5 x 5 neighbourhood inside the frame
__global__ __launch_bounds__(QA_NT) void ring_plane_kernel(const uint8_t* __restrict__ map, int H, int W, uint8_t* __restrict__ ring) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        bool near = false;
        for (int a = max(y - 2, 0); a <= min(y + 2, H - 1); ++a)
            for (int b = max(x - 2, 0); b <= min(x + 2, W - 1); ++b) near |= map[(size_t)a * W + b] == 2;
        ring[i] = (uint8_t)(near && map[i] != 2);
    }
}

// the float32 5-tap Gaussian of oracle/temporal_ref.py (gaussian5_f32): c * k2 + (l1 + r1) * k1, plus (l2 + r2) * k0
__device__ __forceinline__ float gauss5_f32(float l2, float l1, float c, float r1, float r2) {
    return (c * 0.375f + (l1 + r1) * 0.25f) + ((l2 + r2) * 0.0625f);
}

__global__ __launch_bounds__(QA_NT) void ring_rows_kernel(const uint8_t* __restrict__ ring, int H, int W, float* __restrict__ rows) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        const uint8_t* r = ring + (size_t)y * W;
        rows[i] = gauss5_f32((float)r[reflect101(x - 2, W)], (float)r[reflect101(x - 1, W)], (float)r[x], (float)r[reflect101(x + 1, W)],
                             (float)r[reflect101(x + 2, W)]);
    }
}

// frame * (1 - mask * strength) + smoothed * mask * strength: the mask float32, the rest float64, truncated
__global__ __launch_bounds__(QA_NT) void ring_blend_kernel(const uint8_t* __restrict__ frame, const float* __restrict__ rows, int H, int W,
                                                           double strength, uint8_t* __restrict__ dst) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        auto R = [&](int yy) { return rows[(size_t)reflect101(yy, H) * W + x]; };
        const float mask = gauss5_f32(R(y - 2), R(y - 1), R(y), R(y + 1), R(y + 2));
        if (mask == 0.0f) {                                                 // frame * 1.0 + smoothed * 0.0
            dst[i * 3] = frame[i * 3], dst[i * 3 + 1] = frame[i * 3 + 1], dst[i * 3 + 2] = frame[i * 3 + 2];
            continue;
        }
        int g[3];
        gauss5_px(frame, W, taps5(y, x, H, W), g);
        const double rm = (double)mask * strength, keep = 1.0 - rm;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = (double)frame[i * 3 + c] * keep + (double)g[c] * rm;
            dst[i * 3 + c] = (uint8_t)v;
        }
    }
}

// ---- `_remove_banding_opencv` ------------------------------------------------------------------------------------------------------
// 1 - clip(|Laplacian(gray)| / 30, 0, 1) in float32; the Laplacian is [0 1 0; 1 -4 1; 0 1 0] with REFLECT_101, exact on integers
__global__ __launch_bounds__(QA_NT) void band_flat_kernel(const uint8_t* __restrict__ frame, int H, int W, float* __restrict__ flat) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        auto G = [&](int yy, int xx) { return gray_bgr<3>(frame + ((size_t)reflect101(yy, H) * W + reflect101(xx, W)) * 3); };
        const int lap = G(y - 1, x) + G(y + 1, x) + G(y, x - 1) + G(y, x + 1) - 4 * G(y, x);
        const float v = fabsf((float)lap) / 30.0f;
        flat[i] = 1.0f - fminf(fmaxf(v, 0.0f), 1.0f);
    }
}

struct Gauss15 {
    float c[15];
};

// acc = 0; acc += p[k] * c[k], k = 0 .. 14
__global__ __launch_bounds__(QA_NT) void band_rows_kernel(const float* __restrict__ flat, int H, int W, Gauss15 g, float* __restrict__ rows) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        const float* r = flat + (size_t)y * W;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 15; ++k) acc += r[reflect101(x + k - 7, W)] * g.c[k];
        rows[i] = acc;
    }
}

// the column pass, then trunc(clip(float32(frame) + (noise * mask) * strength, 0, 255)): the product float32, the rest float64
__global__ __launch_bounds__(QA_NT) void band_dither_kernel(const uint8_t* __restrict__ frame, const float* __restrict__ rows, int H, int W,
                                                            Gauss15 g, double strength, const float* __restrict__ noise,
                                                            const float* __restrict__ noise_table, uint64_t key, uint8_t* __restrict__ dst) {
    QA_FOR_EACH_PIXEL(i, y, x) {
        float mask = 0.0f;
#pragma unroll
        for (int k = 0; k < 15; ++k) mask += rows[(size_t)reflect101(y + k - 7, H) * W + x] * g.c[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint64_t e = (uint64_t)i * 3 + c;
            const float nz = noise ? noise[e] : noise_table[mix64(key + e) >> 48];
            const float t = nz * mask;
            const double v = (double)(float)frame[e] + (double)t * strength;
            dst[e] = (uint8_t)fmin(fmax(v, 0.0), 255.0);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
int pixel_blocks(size_t n) { return (int)std::min<size_t>((n + QA_NT - 1) / QA_NT, 8192); }

int check_frame(const char* fn, const void* frame, const void* out, int H, int W, int C) {
    if (!frame || !out) return invalid(fn, "null pointer");
    if (const int st = check_side_and_channels(fn, H, W, C)) return st;
    if (C != 3) return invalid(fn, "3 (BGR) channels expected");
    FrameMarks marks = {{(uintptr_t)out, 0}, {(uintptr_t)frame, 1}};
    if (frames_overlap(marks, (size_t)H * W * 3)) return invalid(fn, "out overlaps frame");
    return FW_OK;
}

int check_bilateral(const char* fn, int d, const float* color, const float* space) {
    if (d < 2 || d > 2 * QA_MAX_R + 1) return invalid(fn, "d 2 .. 15 expected");
    if (!color || !space) return invalid(fn, "null pointer");
    return FW_OK;
}

void launch_bilateral(const uint8_t* src, int H, int W, int d, const float* color, const float* space, uint8_t* dst, hipStream_t st) {
    const dim3 grid((unsigned)((W + QA_TW - 1) / QA_TW), (unsigned)((H + QA_TH - 1) / QA_TH));
#define FW_QA_BILATERAL(R) \
    case R: hipLaunchKernelGGL((bilateral_u8c3_kernel<R>), grid, dim3(QA_NT), 0, st, src, H, W, color, space, dst); break
    switch (std::max(d / 2, 1)) {
        FW_QA_BILATERAL(1);
        FW_QA_BILATERAL(2);
        FW_QA_BILATERAL(3);
        FW_QA_BILATERAL(4);
        FW_QA_BILATERAL(5);
        FW_QA_BILATERAL(6);
        FW_QA_BILATERAL(7);
    }
#undef FW_QA_BILATERAL
    FW_HIP_CHECK(hipGetLastError());
}

// scratch: the Canny planes, three frames (the bilateral's result and two to alternate between the steps), two float32 planes, the ring
struct Scratch {
    void* canny;
    uint8_t* frames[3];
    float* planes[2];
    uint8_t* ring;
    static size_t bytes(int H, int W) {
        const size_t n = (size_t)H * W;
        return align256(preserve_edges_scratch_bytes(H, W)) + 3 * align256(3 * n) + 2 * align256(4 * n) + align256(n);
    }
    Scratch(void* base, int H, int W) {
        const size_t n = (size_t)H * W;
        char* s = static_cast<char*>(base);
        canny = s, s += align256(preserve_edges_scratch_bytes(H, W));
        for (auto& f : frames) f = reinterpret_cast<uint8_t*>(s), s += align256(3 * n);
        for (auto& p : planes) p = reinterpret_cast<float*>(s), s += align256(4 * n);
        ring = reinterpret_cast<uint8_t*>(s);
    }
};

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

size_t fw_qp_artifacts_scratch_bytes(int height, int width) {
    if (height < 1 || height > MAX_FRAME_SIDE || width < 1 || width > MAX_FRAME_SIDE) return 0;
    return Scratch::bytes(height, width);
}

int fw_bilateral_u8c3(const uint8_t* frame, uint8_t* out, int height, int width, int channels, int d, const float* color, const float* space,
                      void* stream) {
    const char* fn = "fw_bilateral_u8c3";
    if (const int st = check_frame(fn, frame, out, height, width, channels)) return st;
    if (const int st = check_bilateral(fn, d, color, space)) return st;
    return guarded([&] { launch_bilateral(frame, height, width, d, color, space, out, (hipStream_t)stream); });
}

int fw_gaussian5_u8(const uint8_t* frame, uint8_t* out, int height, int width, int channels, void* stream) {
    const char* fn = "fw_gaussian5_u8";
    if (const int st = check_frame(fn, frame, out, height, width, channels)) return st;
    hipLaunchKernelGGL(gaussian5_u8_kernel, dim3(pixel_blocks((size_t)height * width)), dim3(QA_NT), 0, (hipStream_t)stream, frame, height, width,
                       out);
    return hip_status(fn, hipGetLastError());
}

int fw_qp_artifacts_u8(const uint8_t* frame, uint8_t* out, int height, int width, int channels, int d, const float* color, const float* space,
                       const float* gauss15, double strength, int block_size, int type_mask, const float* noise, const float* noise_table,
                       uint64_t noise_key, void* scratch, void* stream) {
    const char* fn = "fw_qp_artifacts_u8";
    const int H = height, W = width;
    if (const int st = check_frame(fn, frame, out, H, W, channels)) return st;
    if (type_mask < 0 || type_mask > 7) return invalid(fn, "a type mask 0 .. 7 expected (1 blocking, 2 ringing, 4 banding)");
    if (!(strength > 0.0 && strength <= 1.0)) return invalid(fn, "a strength in (0, 1] expected");
    if (type_mask & QA_BLOCKING) {
        if (const int st = check_bilateral(fn, d, color, space)) return st;
        if (block_size != 4 && block_size != 8 && block_size != 16 && block_size != 32) return invalid(fn, "block size 4, 8, 16 or 32 expected");
    }
    if ((type_mask & QA_BANDING) && (!gauss15 || (!noise && !noise_table))) return invalid(fn, "null pointer");
    if (type_mask && (!scratch || ((uintptr_t)scratch & 255)))
        return invalid(fn, "a 256-byte aligned scratch of fw_qp_artifacts_scratch_bytes(height, width) expected");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const size_t n = (size_t)H * W;
        const int blocks = pixel_blocks(n);
        if (!type_mask) {
            FW_HIP_CHECK(hipMemcpyAsync(out, frame, n * 3, hipMemcpyDeviceToDevice, st));
            return;
        }
        const Scratch s(scratch, H, W);
        const uint8_t* cur = frame;
        int turn = 0;
        // the destination of the step `bit`: `out` for the last step of the mask, else the alternate of the two frames
        auto dest = [&](int bit) { return (type_mask >> 1) < bit ? out : s.frames[1 + (turn++ & 1)]; };
        if (type_mask & QA_BLOCKING) {
            uint8_t* dst = dest(QA_BLOCKING);
            launch_bilateral(cur, H, W, d, color, space, s.frames[0], st);
            hipLaunchKernelGGL(boundary_blend_kernel, dim3(blocks), dim3(QA_NT), 0, st, (const uint8_t*)s.frames[0], cur, H, W, block_size, strength,
                               dst);
            cur = dst;
        }
        if (type_mask & QA_RINGING) {
            uint8_t* dst = dest(QA_RINGING);
            const uint8_t* map = launch_canny_edge_map(cur, H, W, 50, 150, s.canny, st);
            hipLaunchKernelGGL(ring_plane_kernel, dim3(blocks), dim3(QA_NT), 0, st, map, H, W, s.ring);
            hipLaunchKernelGGL(ring_rows_kernel, dim3(blocks), dim3(QA_NT), 0, st, (const uint8_t*)s.ring, H, W, s.planes[0]);
            hipLaunchKernelGGL(ring_blend_kernel, dim3(blocks), dim3(QA_NT), 0, st, cur, (const float*)s.planes[0], H, W, strength, dst);
            cur = dst;
        }
        if (type_mask & QA_BANDING) {
            uint8_t* dst = dest(QA_BANDING);
            Gauss15 g;
            std::copy(gauss15, gauss15 + 15, g.c);
            hipLaunchKernelGGL(band_flat_kernel, dim3(blocks), dim3(QA_NT), 0, st, cur, H, W, s.planes[0]);
            hipLaunchKernelGGL(band_rows_kernel, dim3(blocks), dim3(QA_NT), 0, st, (const float*)s.planes[0], H, W, g, s.planes[1]);
            hipLaunchKernelGGL(band_dither_kernel, dim3(blocks), dim3(QA_NT), 0, st, cur, (const float*)s.planes[1], H, W, g, strength, noise,
                               noise_table, (uint64_t)noise_key, dst);
        }
        FW_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
