// Missing-frame generation (kernel set K22 of DESIGN.md): the frame methods of the reference's processors/frame_generation.py -
// `_generate_optical_flow` behind its two Farneback flows, `_match_film_grain`, `_blend_edges`, `_extrapolate_frames` - on uint8 BGR
// frames that are already on the device.  tests/frame_generation_ref.py states every step in numpy and is the contract, byte for
// byte; the one float64 reduction (the grain deviation) may differ from numpy's order within the bound DESIGN.md K22 derives.
//
// Every a * b + c here must round twice, as numpy's does: the file is compiled with -ffp-contract=off (build.py PER_FILE_FLAGS).
// Nothing here allocates or waits: the two deviations the grain decision needs are read from device memory by the kernel that
// uses them.
#include <hip/hip_runtime.h>
#include <math.h>

#include "stage_common.h"
#include "add_weighted.h"
#include "remap_linear.h"

namespace fw {
namespace {

constexpr int FG_NT = 256;
constexpr int FG_TW = 64, FG_TH = 16, FG_R = 8;            // the blur's output tile and the 17-tap kernel's radius
constexpr int FG_LW = FG_TW + 2 * FG_R, FG_LH = FG_TH + 2 * FG_R;
constexpr int FG_MIN_SIDE = 16;

#define FG_FOR_EACH(i, n)                                                                                    \
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x, n_ = (long)(n); i < n_; i += (long)gridDim.x * blockDim.x)

// ---- `_generate_optical_flow`, one generated frame ----------------------------------------------------------------------------------
// map = grid + flow * t in float32 (the product rounded, then the sum), both frames sampled with BORDER_REFLECT, the two samples
// blended as cv2.addWeighted(warped_before, 1 - t, warped_after, t).  One lane a pixel, consecutive lanes along a row: a flow that
// varies slowly sends a wave's 64 x 4 neighbours per frame to a few cache lines of two rows.  The kernel issues 24 byte loads a
// pixel and is bound by that address rate, not by the bytes.
__global__ __launch_bounds__(FG_NT) void warp_blend_kernel(const uint8_t* __restrict__ before, const uint8_t* __restrict__ after,
                                                           const float* __restrict__ fwd_x, const float* __restrict__ fwd_y,
                                                           const float* __restrict__ bwd_x, const float* __restrict__ bwd_y, int H, int W,
                                                           float t, float one_minus_t, uint8_t* __restrict__ out) {
    FG_FOR_EACH(i, (long)H * W) {
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        int a[3], b[3];
        remap_linear_u8c3(before, H, W, (float)x + fwd_x[i] * t, (float)y + fwd_y[i] * t, BorderReflect(), a);
        remap_linear_u8c3(after, H, W, (float)x + bwd_x[i] * one_minus_t, (float)y + bwd_y[i] * one_minus_t, BorderReflect(), b);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[i * 3 + c] = (uint8_t)aw_byte((uint32_t)a[c], one_minus_t, (uint32_t)b[c], t);
    }
}

// ---- the statistic of `_match_film_grain` -------------------------------------------------------------------------------------------
// gray = cv2's 8-bit gray as float32; blur = the 17-tap separable Gaussian (REFLECT_101), rows then columns, each acc = 0;
// acc += p[k] * c[k] for k = 0 .. 16; grain = gray - blur.  One workgroup a 64 x 16 tile: the gray tile with its 8-pixel halo and the
// row pass of its 32 rows live in LDS.  A lane adds the grain and its square of its four pixels in float64, top to bottom; the
// wave's butterfly, then the four waves in order, give the workgroup's partial pair.
struct Gauss17 {
    float c[17];
};

__global__ __launch_bounds__(FG_NT) void grain_partials_kernel(const uint8_t* __restrict__ frame, int H, int W, Gauss17 g,
                                                               double* __restrict__ partials) {
    __shared__ float s_g[FG_LH][FG_LW];
    __shared__ float s_r[FG_LH][FG_TW];
    __shared__ double s_p[FG_NT / 64][2];
    const int tid = threadIdx.x, x0 = blockIdx.x * FG_TW, y0 = blockIdx.y * FG_TH;
    for (int k = tid; k < FG_LH * FG_LW; k += FG_NT) {
        const int yy = k / FG_LW, xx = k - yy * FG_LW;
        s_g[yy][xx] = (float)gray_bgr<3>(frame + ((size_t)reflect101(y0 + yy - FG_R, H) * W + reflect101(x0 + xx - FG_R, W)) * 3);
    }
    __syncthreads();
    for (int k = tid; k < FG_LH * FG_TW; k += FG_NT) {
        const int yy = k / FG_TW, xx = k - yy * FG_TW;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 17; ++j) acc += s_g[yy][xx + j] * g.c[j];
        s_r[yy][xx] = acc;
    }
    __syncthreads();
    const int lx = tid & 63, ly = tid >> 6;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int q = 0; q < FG_TH / 4; ++q) {
        const int row = ly * (FG_TH / 4) + q;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 17; ++j) acc += s_r[row + j][lx] * g.c[j];
        if (x0 + lx < W && y0 + row < H) {
            const double grain = (double)(s_g[row + FG_R][lx + FG_R] - acc);
            s1 += grain;
            s2 += grain * grain;
        }
    }
    s1 = wave_sum(s1), s2 = wave_sum(s2);
    if ((tid & 63) == 0) s_p[tid >> 6][0] = s1, s_p[tid >> 6][1] = s2;
    __syncthreads();
    if (tid == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < FG_NT / 64; ++w) t1 += s_p[w][0], t2 += s_p[w][1];
        const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[2 * b] = t1, partials[2 * b + 1] = t2;
    }
}

// One workgroup: lane t adds the partial pairs t, t + 256, ... in that order, then the butterfly and the four waves in order.
// std = sqrt(S2 / N - (S1 / N)^2) in float64, rounded once to float32.
__global__ __launch_bounds__(FG_NT) void grain_std_kernel(const double* __restrict__ partials, int count, double n, float* __restrict__ out) {
    __shared__ double s_p[FG_NT / 64][2];
    const int tid = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int b = tid; b < count; b += FG_NT) s1 += partials[2 * b], s2 += partials[2 * b + 1];
    s1 = wave_sum(s1), s2 = wave_sum(s2);
    if ((tid & 63) == 0) s_p[tid >> 6][0] = s1, s_p[tid >> 6][1] = s2;
    __syncthreads();
    if (tid == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < FG_NT / 64; ++w) t1 += s_p[w][0], t2 += s_p[w][1];
        const double mean = t1 / n;
        const double var = t2 / n - mean * mean;
        out[0] = (float)sqrt(fmax(var, 0.0));
    }
}

// ---- the rest of a generated frame: grain, then the edge blends ---------------------------------------------------------------------
// grain: where cur > 0 and ref > cur, trunc(clip(float32(v) + z * float64(ref - cur), 0, 255)) in float64, z one standard-normal
// value a pixel for its three channels: `draws[pixel]`, else quantiles[mix64(key + pixel) >> 48].  Then addWeighted against `before`
// (keep = float32(1 - alpha), formed in float64 on the host) and against `after`, each where its frame is given.
__global__ __launch_bounds__(FG_NT) void finish_kernel(const uint8_t* gen /* may be `out` */, int H, int W, const float* __restrict__ ref_std,
                                                       const float* __restrict__ cur_std, const double* __restrict__ draws,
                                                       const double* __restrict__ quantiles, uint64_t key,
                                                       const uint8_t* __restrict__ before, float keep_before, float alpha_before,
                                                       const uint8_t* __restrict__ after, float keep_after, float alpha_after, uint8_t* out) {
    bool add = false;
    double scale = 0.0;
    if (ref_std) {
        const float ref = ref_std[0], cur = cur_std[0];
        add = cur > 0.0f && ref > cur;
        scale = (double)(ref - cur);
    }
    FG_FOR_EACH(i, (long)H * W) {
        uint32_t v[3] = {gen[i * 3], gen[i * 3 + 1], gen[i * 3 + 2]};
        if (add) {
            const double grain = 0.0 + scale * (draws ? draws[i] : quantiles[mix64(key + (uint64_t)i) >> 48]);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (uint32_t)fmin(fmax((double)(float)v[c] + grain, 0.0), 255.0);
        }
        if (before) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = aw_byte(before[i * 3 + c], keep_before, v[c], alpha_before);
        }
        if (after) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = aw_byte(after[i * 3 + c], keep_after, v[c], alpha_after);
        }
        out[i * 3] = (uint8_t)v[0], out[i * 3 + 1] = (uint8_t)v[1], out[i * 3 + 2] = (uint8_t)v[2];
    }
}

// ---- `_extrapolate_frames`, one frame: trunc(clip(float32(reference) + noise, 0, 255)) in float32 ------------------------------------
__global__ __launch_bounds__(FG_NT) void extrapolate_kernel(const uint8_t* __restrict__ reference, long n, const float* __restrict__ noise,
                                                            const float* __restrict__ table, uint64_t key, uint8_t* __restrict__ out) {
    FG_FOR_EACH(e, n) {
        const float nz = noise ? noise[e] : table[mix64(key + (uint64_t)e) >> 48];
        out[e] = (uint8_t)fminf(fmaxf((float)reference[e] + nz, 0.0f), 255.0f);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
int blocks_for(size_t n) { return (int)std::min<size_t>((n + FG_NT - 1) / FG_NT, 8192); }

int check_sides(const char* fn, int H, int W, int min_side) {
    if (H < min_side || H > MAX_FRAME_SIDE || W < min_side || W > MAX_FRAME_SIDE)
        return invalid(fn, std::to_string(min_side) + " .. 16384 pixels a side expected");
    return FW_OK;
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

dim3 tile_grid(int H, int W) { return dim3((unsigned)((W + FG_TW - 1) / FG_TW), (unsigned)((H + FG_TH - 1) / FG_TH)); }

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_framegen_warp_blend_u8(const uint8_t* before, const uint8_t* after, const float* fwd_x, const float* fwd_y, const float* bwd_x,
                              const float* bwd_y, int height, int width, double t, uint8_t* out, void* stream) {
    const char* fn = "fw_framegen_warp_blend_u8";
    if (!before || !after || !fwd_x || !fwd_y || !bwd_x || !bwd_y || !out) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, 1)) return st;
    if (!(t > 0.0 && t < 1.0)) return invalid(fn, "t in (0, 1) expected");
    if (misaligned(fwd_x, 4) || misaligned(fwd_y, 4) || misaligned(bwd_x, 4) || misaligned(bwd_y, 4)) return invalid(fn, "4-byte aligned flow planes expected");
    FrameMarks marks = {{(uintptr_t)out, 0}, {(uintptr_t)before, 1}, {(uintptr_t)after, 1}};
    if (frames_overlap(marks, (size_t)height * width * 3)) return invalid(fn, "out overlaps a frame");
    hipLaunchKernelGGL(warp_blend_kernel, dim3(blocks_for((size_t)height * width)), dim3(FG_NT), 0, (hipStream_t)stream, before, after, fwd_x, fwd_y,
                       bwd_x, bwd_y, height, width, (float)t, (float)(1.0 - t), out);
    return hip_status(fn, hipGetLastError());
}

size_t fw_framegen_grain_scratch_bytes(int height, int width) {
    if (height < FG_MIN_SIDE || height > MAX_FRAME_SIDE || width < FG_MIN_SIDE || width > MAX_FRAME_SIDE) return 0;
    const dim3 grid = tile_grid(height, width);
    return (size_t)grid.x * grid.y * 2 * sizeof(double);
}

int fw_framegen_grain_std_u8(const uint8_t* frame, int height, int width, const float* gauss17, void* scratch, float* std_out, void* stream) {
    const char* fn = "fw_framegen_grain_std_u8";
    if (!frame || !gauss17 || !scratch || !std_out) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, FG_MIN_SIDE)) return st;
    if (misaligned(scratch, 8) || misaligned(std_out, 4))
        return invalid(fn, "an 8-byte aligned scratch of fw_framegen_grain_scratch_bytes(height, width) and a 4-byte aligned result expected");
    Gauss17 g;
    std::copy(gauss17, gauss17 + 17, g.c);
    const dim3 grid = tile_grid(height, width);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grain_partials_kernel, grid, dim3(FG_NT), 0, st, frame, height, width, g, (double*)scratch);
    hipLaunchKernelGGL(grain_std_kernel, dim3(1), dim3(FG_NT), 0, st, (const double*)scratch, (int)(grid.x * grid.y), (double)height * (double)width,
                       std_out);
    return hip_status(fn, hipGetLastError());
}

int fw_framegen_finish_u8(const uint8_t* generated, uint8_t* out, int height, int width, const float* ref_std, const float* cur_std,
                          const double* draws, const double* quantiles, uint64_t noise_key, const uint8_t* before, double alpha_before,
                          const uint8_t* after, double alpha_after, void* stream) {
    const char* fn = "fw_framegen_finish_u8";
    if (!generated || !out) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, 1)) return st;
    if ((ref_std == nullptr) != (cur_std == nullptr)) return invalid(fn, "both deviations or neither expected");
    if (ref_std && !draws && !quantiles) return invalid(fn, "null pointer");
    if (misaligned(ref_std, 4) || misaligned(cur_std, 4) || misaligned(draws, 8) || misaligned(quantiles, 8))
        return invalid(fn, "4-byte aligned deviations and 8-byte aligned draws expected");
    if ((before && !std::isfinite(alpha_before)) || (after && !std::isfinite(alpha_after))) return invalid(fn, "a finite alpha expected");
    FrameMarks marks = {{(uintptr_t)out, 0}};
    if (out != generated) marks.push_back({(uintptr_t)generated, 1});      // in place is fine: a pixel is read before it is written
    if (before) marks.push_back({(uintptr_t)before, 1});
    if (after) marks.push_back({(uintptr_t)after, 1});
    if (frames_overlap(marks, (size_t)height * width * 3)) return invalid(fn, "out overlaps a frame");
    hipLaunchKernelGGL(finish_kernel, dim3(blocks_for((size_t)height * width)), dim3(FG_NT), 0, (hipStream_t)stream, generated, height, width, ref_std,
                       cur_std, draws, quantiles, (uint64_t)noise_key, before, (float)(1.0 - alpha_before), (float)alpha_before, after,
                       (float)(1.0 - alpha_after), (float)alpha_after, out);
    return hip_status(fn, hipGetLastError());
}

int fw_framegen_extrapolate_u8(const uint8_t* reference, uint8_t* out, int height, int width, const float* noise, const float* noise_table,
                               uint64_t noise_key, void* stream) {
    const char* fn = "fw_framegen_extrapolate_u8";
    if (!reference || !out || (!noise && !noise_table)) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, 1)) return st;
    if (misaligned(noise, 4) || misaligned(noise_table, 4)) return invalid(fn, "4-byte aligned noise expected");
    FrameMarks marks = {{(uintptr_t)out, 0}, {(uintptr_t)reference, 1}};
    if (frames_overlap(marks, (size_t)height * width * 3)) return invalid(fn, "out overlaps reference");
    const size_t n = (size_t)height * width * 3;
    hipLaunchKernelGGL(extrapolate_kernel, dim3(blocks_for(n)), dim3(FG_NT), 0, (hipStream_t)stream, reference, (long)n, noise, noise_table,
                       (uint64_t)noise_key, out);
    return hip_status(fn, hipGetLastError());
}

}  // extern "C"
