// The three kernels that close the classical temporal denoise of the reference (src/framewright/processors/temporal_denoise.py)
// on the device, around the flow (optical_flow.hip), the accumulate (frame_ops.hip) and the non-local means (nlmeans.hip):
//
//   fw_frame_stats_u8            what `TemporalDenoiser.analyze` (:1110-1300) and `_estimate_noise_reduction` (:1734-1788) read
//                                from a frame: the 256-bin histogram of gray = cv2.cvtColor(BGR2GRAY) (scene cuts :1180-1207,
//                                brightness :563-564) and the exact integer sums of cv2.Laplacian(gray, CV_64F) and of its square
//                                (ksize 1: taps [[0,1,0],[1,-4,1],[0,1,0]], BORDER_REFLECT_101; the variance of :1236-1237).
//   fw_flow_accumulate_affine_u8 the per-neighbour step of `TemporalConsistencyFilter._apply_flow_guided_filter` (:975-1005):
//                                weight = a + b * confidence in float64, remap and accumulate of flow_accumulate.h.
//   fw_add_weighted_u8           cv2.addWeighted(a, alpha, b, beta, 0) on uint8 (:1016-1020, :1055-1059).
//
// cv2 is absent where this is built, so tests/temporal_chain_ref.py is the contract and parity with cv2 is unpinned.  For
// addWeighted that concerns exact .5 ties only: the restatement is t = fl32(fl32(a * alpha) + fl32(b * beta)) with alpha and beta
// rounded once to float32, rounded half to even and saturated; an OpenCV build that fuses the multiply-add can differ there.
// Compiled with -ffp-contract=off (build.py): the products above round before they are added.
//
// fw_frame_stats_u8 is bound by its one read of the frames.  A workgroup owns a 256 x 16 tile of one frame of the batch (frame =
// grid.z): gray goes once into LDS with a one-pixel reflected halo (18 rows re-read per 16: the halo rows come from L2), every
// pixel bumps its wave's private LDS histogram, the two sums are reduced across the wave by shuffles, and a workgroup ends with at
// most 256 32-bit and 8 64-bit vector atomics.  Integer atomics commute: the result does not depend on scheduling.
#include <math.h>

#include "stage_common.h"
#include "add_weighted.h"
#include "flow_accumulate.h"

namespace fw {
namespace {

constexpr int ST_TW = 256, ST_TH = 16, ST_NT = 256, ST_WAVES = ST_NT / 64;
constexpr int ST_LW = ST_TW + 2;

__global__ __launch_bounds__(ST_NT) void frame_stats_kernel(const uint8_t* __restrict__ frames, int H, int W, uint32_t* hist,
                                                            unsigned long long* lap_sums) {
    __shared__ uint8_t s_g[(ST_TH + 2) * ST_LW];
    __shared__ uint32_t s_hist[ST_WAVES][256];
    const int tid = threadIdx.x, x0 = blockIdx.x * ST_TW, y0 = blockIdx.y * ST_TH, f = blockIdx.z;
    const uint8_t* frame = frames + (size_t)f * H * W * 3;
    for (int i = tid; i < ST_WAVES * 256; i += ST_NT) (&s_hist[0][0])[i] = 0;
    for (int i = tid; i < (ST_TH + 2) * ST_LW; i += ST_NT) {
        const int ly = i / ST_LW, lx = i - ly * ST_LW;
        const int ry = y0 - 1 + ly, rx = x0 - 1 + lx;         // -1 .. : one past the frame is the last halo anybody reads
        uint8_t g = 0;
        if (ry <= H && rx <= W) {
            const uint8_t* p = frame + ((size_t)reflect101(ry, H) * W + reflect101(rx, W)) * 3;
            g = (uint8_t)gray_bgr<3>(p);
        }
        s_g[i] = g;
    }
    __syncthreads();
    const int x = x0 + tid;
    int s1 = 0, s2 = 0;                                        // 16 pixels: |s1| <= 16320, s2 <= 16.7e6
    if (x < W) {
        uint32_t* my_hist = s_hist[tid >> 6];
        for (int r = 0; r < ST_TH && y0 + r < H; ++r) {
            const uint8_t* c = &s_g[(r + 1) * ST_LW + tid + 1];
            const int g = c[0];
            const int lap = c[-ST_LW] + c[ST_LW] + c[-1] + c[1] - 4 * g;
            s1 += lap;
            s2 += lap * lap;
            atomicAdd(&my_hist[g], 1u);
        }
    }
    const long long t1 = wave_sum((long long)s1), t2 = wave_sum((long long)s2);
    if ((tid & 63) == 0 && (t1 != 0 || t2 != 0)) {
        atomicAdd(&lap_sums[(size_t)f * 2], (unsigned long long)t1);       // two's complement: the signed sum
        atomicAdd(&lap_sums[(size_t)f * 2 + 1], (unsigned long long)t2);
    }
    __syncthreads();
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < ST_WAVES; ++w) v += s_hist[w][tid];
    if (v) atomicAdd(&hist[(size_t)f * 256 + tid], v);
}

__global__ __launch_bounds__(256) void flow_accumulate_affine_kernel(const uint8_t* __restrict__ frame, const float* __restrict__ fx,
                                                                     const float* __restrict__ fy, const float* __restrict__ conf,
                                                                     double w_const, double w_conf, int inverse, int H, int W,
                                                                     double* acc, double* wsum) {
    flow_accumulate_pixels(frame, fx, fy, inverse, H, W, acc, wsum,
                           [=](long i) { return conf ? w_const + w_conf * (double)conf[i] : w_const; });
}

// words: how many leading 4-byte groups go through 32-bit loads and stores (0 unless all three pointers are 4-byte aligned)
__global__ __launch_bounds__(256) void add_weighted_kernel(const uint8_t* a, float alpha, const uint8_t* b, float beta, size_t n,
                                                           size_t words, uint8_t* out) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = t0; i < words; i += step) {
        const uint32_t va = reinterpret_cast<const uint32_t*>(a)[i], vb = reinterpret_cast<const uint32_t*>(b)[i];
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) o |= aw_byte((va >> (8 * k)) & 255u, alpha, (vb >> (8 * k)) & 255u, beta) << (8 * k);
        reinterpret_cast<uint32_t*>(out)[i] = o;
    }
    for (size_t i = words * 4 + t0; i < n; i += step) out[i] = (uint8_t)aw_byte(a[i], alpha, b[i], beta);
}

int tc_blocks(size_t n) {
    const size_t b = (n + 255) / 256;
    return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_frame_stats_u8(const uint8_t* frames_bgr, int count, int height, int width, uint32_t* hist, int64_t* lap_sums, void* stream) {
    if (!frames_bgr || !hist || !lap_sums) return fail(FW_ERR_INVALID, "fw_frame_stats_u8: null pointer");
    if (count < 1 || count > 65535) return fail(FW_ERR_INVALID, "fw_frame_stats_u8: 1 .. 65535 frames per call expected");
    if (height < 1 || width < 1 || (long)height * width > (1L << 30) || (height + ST_TH - 1) / ST_TH > 65535)
        return fail(FW_ERR_INVALID, "fw_frame_stats_u8: bad frame size");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        FW_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)count * 256 * sizeof(uint32_t), st));
        FW_HIP_CHECK(hipMemsetAsync(lap_sums, 0, (size_t)count * 2 * sizeof(int64_t), st));
        const dim3 grid((width + ST_TW - 1) / ST_TW, (height + ST_TH - 1) / ST_TH, count);
        hipLaunchKernelGGL(frame_stats_kernel, grid, dim3(ST_NT), 0, st, frames_bgr, height, width, hist, (unsigned long long*)lap_sums);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_flow_accumulate_affine_u8(const uint8_t* frame_bgr, const float* flow_x, const float* flow_y, const float* confidence,
                                 double w_const, double w_conf, int inverse, int height, int width, double* accumulated,
                                 double* weight_sum, void* stream) {
    if (!frame_bgr || !accumulated || !weight_sum || height < 1 || width < 1 || (flow_x == nullptr) != (flow_y == nullptr) ||
        (long)height * width > (1L << 30))
        return fail(FW_ERR_INVALID, "fw_flow_accumulate_affine_u8: bad argument");
    return guarded([&] {
        hipLaunchKernelGGL(flow_accumulate_affine_kernel, dim3(tc_blocks((size_t)height * width)), dim3(256), 0, (hipStream_t)stream,
                           frame_bgr, flow_x, flow_y, confidence, w_const, w_conf, inverse, height, width, accumulated, weight_sum);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_add_weighted_u8(const uint8_t* a, double alpha, const uint8_t* b, double beta, size_t nbytes, uint8_t* out, void* stream) {
    if (!a || !b || !out || !std::isfinite(alpha) || !std::isfinite(beta)) return fail(FW_ERR_INVALID, "fw_add_weighted_u8: bad argument");
    if (nbytes == 0) return FW_OK;
    return guarded([&] {
        const bool aligned = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) == 0;
        const size_t words = aligned ? nbytes / 4 : 0;
        hipLaunchKernelGGL(add_weighted_kernel, dim3(tc_blocks(aligned ? (nbytes + 3) / 4 : nbytes)), dim3(256), 0, (hipStream_t)stream, a,
                           (float)alpha, b, (float)beta, nbytes, words, out);
        FW_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
