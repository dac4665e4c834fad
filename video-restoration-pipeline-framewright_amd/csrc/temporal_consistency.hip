// Cross-frame temporal consistency (kernel set K23): the classical path of the reference's `CrossAttentionTemporalProcessor`
// (src/framewright/processors/cross_attention_temporal.py:347-429) on uint8 BGR H x W x 3 frames that are already on the device,
// behind the interpolation and in front of the colour grade (step 7b).  tests/temporal_consistency_ref.py is the contract, byte for
// byte.
//
//   fw_tcons_gray_hist_u8   the 256 counts of cv2.calcHist on cvtColor(BGR2GRAY) of one frame (`_detect_scene_change`; the
//                           normalisation and cv2.compareHist(HISTCMP_CORREL) are 256-element host arithmetic in the driver)
//   fw_tcons_apply_u8       `_detect_flicker` and the blend of `_apply_optical_flow_consistency` in one launch per output frame
//
// apply.  A workgroup of 256 threads owns a 64 x 32 tile of the output.
//   1. The 36 rows under the tile and its 2-pixel halo - the rows outside the frame are their BORDER_REFLECT_101 images, y -> -y and
//      y -> 2 H - 2 - y - are read once per frame as the aligned 32-bit words that cover the columns max(0, x0 - 2) .. min(W, x0 + 66)
//      (a frame of a contiguous clip may start at any byte) into LDS: 3 x 36 x 53 words.  The reflected COLUMNS are inside that span
//      (W >= 3), so they are an index into it and no second read.
//   2. The binary mask of the 36 x 68 pixels: per frame pair the 14-bit gray of the three absolute differences, g / 255 (a float32
//      division, made once per gray value into a 256-entry LDS table), min(dp, dn) * (1 - nb) - one subtraction, one product, each
//      rounded once - and the compare with the threshold.
//   3. Rows, then columns, taps 1 4 6 4 1 on the 0 / 1 bytes as integers: k = 256 x the blurred mask, exactly (every product and sum
//      of the reference's float32 blur of a 0 / 1 plane under the dyadic table is exact, so its order does not matter).
//   4. A thread blends eight pixels of its column: mask = k / 256, m3 = mask * strength, 1 - m3, cur * (1 - m3), ((prev + next) / 2) * m3,
//      their sum, truncated - eight float32 operations in the reference's order, none contracted (build.py: -ffp-contract=off).  The
//      bytes come from the LDS image of step 1.  The result stays inside [0, 255], so the conversion never wraps.
// The mask plane (float32 k / 256) and the area numerator (the sum of k over the frame, an integer: one 64-bit atomic add per
// workgroup, order-free) leave through nullable pointers.  Nothing is allocated and the host never waits.
//
// hist.  A workgroup takes 8192 pixels, each wave bumps a private 256-bin LDS table, and the workgroup ends with at most 256 32-bit
// integer vector atomics: integer adds commute, the counts are the same bits on every run.
#include "stage_common.h"

#include <cmath>

namespace fw {
namespace {

constexpr int TC_TW = 64, TC_TH = 32, TC_NT = 256, TC_WAVES = TC_NT / 64, TC_ROWS = TC_TH / TC_WAVES;   // 8 output rows per thread
constexpr int TC_MW = TC_TW + 4, TC_MH = TC_TH + 4;                   // 68 x 36 mask pixels under a tile
constexpr int TC_RAW_WORDS = (3 + TC_MW * 3 + 3) / 4;                 // 52: a row's 204 bytes from any alignment, in aligned words
constexpr int TC_RAW_LD = TC_RAW_WORDS + 1;                           // words per staged row
constexpr int TC_MLD = 72;                                            // bytes per mask row
constexpr int TH_NT = 256, TH_WAVES = TH_NT / 64, TH_PIX = 8192;      // pixels of one workgroup of the histogram kernel

// BORDER_REFLECT_101 one reflection deep (len >= 3, p in -2 .. len + 1); further out - positions whose results are not stored - it
// is some row or column of the frame
__device__ __forceinline__ int reflect_near(int p, int len) {
    p = p < 0 ? -p : p;
    p = p >= len ? 2 * len - 2 - p : p;
    return min(max(p, 0), len - 1);
}

__device__ __forceinline__ int absdiff_gray(const uint8_t* a, const uint8_t* b) {
    const int d0 = abs((int)a[0] - (int)b[0]), d1 = abs((int)a[1] - (int)b[1]), d2 = abs((int)a[2] - (int)b[2]);
    return (d0 * 1868 + d1 * 9617 + d2 * 4899 + (1 << 13)) >> 14;
}

__global__ __launch_bounds__(TC_NT) void tcons_apply_kernel(const uint8_t* __restrict__ prev, const uint8_t* __restrict__ cur,
                                                            const uint8_t* __restrict__ next, int H, int W, float threshold, float strength,
                                                            uint8_t* __restrict__ out, float* __restrict__ mask_out,
                                                            unsigned long long* __restrict__ area) {
    __shared__ uint32_t s_raw[3 * TC_MH * TC_RAW_LD];
    __shared__ uint8_t s_m[TC_MH * TC_MLD];
    __shared__ uint8_t s_h[TC_MH * TC_TW];
    __shared__ unsigned s_part[TC_WAVES];
    __shared__ float s_div[256];                                                  // g / 255, the float32 division, once per gray value
    const int tid = threadIdx.x, x0 = blockIdx.x * TC_TW, y0 = blockIdx.y * TC_TH;
    const size_t frame_bytes = (size_t)H * W * 3;
    const int xs = max(0, x0 - 2), cols = min(W, x0 + TC_TW + 2) - xs;            // the columns of the frame that are staged: 1 .. 68
    const uint8_t* const frames[3] = {prev, cur, next};

    static_assert(TC_NT == 256, "one thread per gray value");
    s_div[tid] = __fdiv_rn((float)tid, 255.0f);
    // 1. the rows' bytes, as the aligned words that cover them
    for (int i = tid; i < 3 * TC_MH * TC_RAW_WORDS; i += TC_NT) {
        const int fr = i / TC_RAW_WORDS, k = i - fr * TC_RAW_WORDS;               // fr = frame * TC_MH + row
        const int f = fr / TC_MH, r = fr - f * TC_MH;
        const uint8_t* frame = f == 0 ? prev : f == 1 ? cur : next;
        const uint8_t* row = frame + ((size_t)reflect_near(y0 - 2 + r, H) * W + xs) * 3;
        const int off = (int)((uintptr_t)row & 3);
        if (4 * k >= off + cols * 3) continue;
        s_raw[fr * TC_RAW_LD + k] = load_word_inside(row - off + 4 * k, frame, frame + frame_bytes);
    }
    __syncthreads();
    // 2. the binary mask of the tile and its halo
    for (int i = tid; i < TC_MH * TC_MW; i += TC_NT) {
        const int r = i / TC_MW, c = i - r * TC_MW;
        const size_t at = ((size_t)reflect_near(y0 - 2 + r, H) * W + xs) * 3;
        const int idx = min(max(reflect_near(x0 - 2 + c, W) - xs, 0), cols - 1) * 3;
        const uint8_t* p[3];
#pragma unroll
        for (int f = 0; f < 3; ++f)
            p[f] = reinterpret_cast<const uint8_t*>(&s_raw[(f * TC_MH + r) * TC_RAW_LD]) + ((uintptr_t)(frames[f] + at) & 3) + idx;
        const float dp = s_div[absdiff_gray(p[1], p[0])], dn = s_div[absdiff_gray(p[1], p[2])], nb = s_div[absdiff_gray(p[0], p[2])];
        const float score = fminf(dp, dn) * (1.0f - nb);
        s_m[r * TC_MLD + c] = score > threshold ? 1 : 0;
    }
    __syncthreads();
    // 3. rows: 0 .. 16
    for (int i = tid; i < TC_MH * TC_TW; i += TC_NT) {
        const uint8_t* m = &s_m[(i / TC_TW) * TC_MLD + (i % TC_TW)];
        s_h[i] = (uint8_t)(m[0] + 4 * m[1] + 6 * m[2] + 4 * m[3] + m[4]);
    }
    __syncthreads();
    // 4. columns: k = 0 .. 256, and the blend of eight pixels down one column
    const int tx = tid & 63, wv = tid >> 6, x = x0 + tx;
    unsigned sum_k = 0;
    if (x < W) {
#pragma unroll
        for (int j = 0; j < TC_ROWS; ++j) {
            const int ty = wv * TC_ROWS + j, y = y0 + ty;
            if (y >= H) break;
            const uint8_t* h = &s_h[ty * TC_TW + tx];
            const int k = h[0] + 4 * h[TC_TW] + 6 * h[2 * TC_TW] + 4 * h[3 * TC_TW] + h[4 * TC_TW];
            sum_k += (unsigned)k;
            const float mask = (float)k * (1.0f / 256.0f);                        // exact
            const size_t pix = (size_t)y * W + x;
            if (mask_out) mask_out[pix] = mask;
            if (out) {
                const float m3 = mask * strength, keep = 1.0f - m3;
                const size_t at = ((size_t)y * W + xs) * 3;
                const uint8_t* p[3];
#pragma unroll
                for (int f = 0; f < 3; ++f)
                    p[f] = reinterpret_cast<const uint8_t*>(&s_raw[(f * TC_MH + ty + 2) * TC_RAW_LD]) + ((uintptr_t)(frames[f] + at) & 3) + (x - xs) * 3;
                uint8_t* o = out + pix * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float blend = ((float)p[0][ch] + (float)p[2][ch]) * 0.5f;   // / 2: exact either way
                    const float a = (float)p[1][ch] * keep, b = blend * m3;
                    o[ch] = (uint8_t)(a + b);
                }
            }
        }
    }
    if (area) {                                                                   // kernel-uniform
        sum_k = wave_sum(sum_k);
        if (tx == 0) s_part[wv] = sum_k;
        __syncthreads();
        if (tid == 0) {
            unsigned long long t = 0;
#pragma unroll
            for (int w = 0; w < TC_WAVES; ++w) t += s_part[w];
            if (t) atomicAdd(area, t);
        }
    }
}

__global__ __launch_bounds__(TH_NT) void tcons_gray_hist_kernel(const uint8_t* __restrict__ frame, long n_pix, uint32_t* hist) {
    __shared__ uint32_t s_hist[TH_WAVES][256];
    const int tid = threadIdx.x;
    for (int i = tid; i < TH_WAVES * 256; i += TH_NT) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    uint32_t* my = s_hist[tid >> 6];
    const long p0 = (long)blockIdx.x * TH_PIX, p1 = min(p0 + TH_PIX, n_pix);
    if (((uintptr_t)frame & 3) == 0) {                                // block-uniform: four pixels = three aligned words per lane
        for (long p = p0 + 4 * tid; p < p1; p += 4 * TH_NT) {
            if (p + 4 <= p1) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(frame + p * 3);
                const uint32_t w[3] = {q[0], q[1], q[2]};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint8_t px[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[c] = (uint8_t)(w[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3)));
                    atomicAdd(&my[gray_bgr<3>(px)], 1u);
                }
            } else {
                for (long i = p; i < p1; ++i) atomicAdd(&my[gray_bgr<3>(frame + i * 3)], 1u);
            }
        }
    } else {
        for (long p = p0 + tid; p < p1; p += TH_NT) atomicAdd(&my[gray_bgr<3>(frame + p * 3)], 1u);
    }
    __syncthreads();
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < TH_WAVES; ++w) v += s_hist[w][tid];
    if (v) atomicAdd(&hist[tid], v);
}

int check_sides(const char* fn, int H, int W) {
    if (H < 3 || H > MAX_FRAME_SIDE || W < 3 || W > MAX_FRAME_SIDE)
        return invalid(fn, "3 .. 16384 pixels a side expected (the 5 x 5 blur reflects two pixels)");
    return FW_OK;
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_tcons_gray_hist_u8(const uint8_t* frame, int height, int width, uint32_t* hist, void* stream) {
    const char* fn = "fw_tcons_gray_hist_u8";
    if (!frame || !hist) return invalid(fn, "null pointer");
    if (const int st = check_side_and_channels(fn, height, width, 3)) return st;
    if ((uintptr_t)hist & 3) return invalid(fn, "a 4-byte aligned histogram expected");
    const long n_pix = (long)height * width;
    hipStream_t st = (hipStream_t)stream;
    if (const int e = hip_status(fn, hipMemsetAsync(hist, 0, 256 * sizeof(uint32_t), st))) return e;
    hipLaunchKernelGGL(tcons_gray_hist_kernel, dim3((unsigned)((n_pix + TH_PIX - 1) / TH_PIX)), dim3(TH_NT), 0, st, frame, n_pix, hist);
    return hip_status(fn, hipGetLastError());
}

int fw_tcons_apply_u8(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, int height, int width, float flicker_threshold,
                      float blend_strength, uint8_t* out, float* mask_out, uint64_t* area_out, void* stream) {
    const char* fn = "fw_tcons_apply_u8";
    if (!prev || !cur || !next) return invalid(fn, "null pointer");
    if (!out && !mask_out && !area_out) return invalid(fn, "nothing to write: out, mask_out and area_out are all null");
    if (const int st = check_sides(fn, height, width)) return st;
    if (!std::isfinite(flicker_threshold)) return invalid(fn, "a finite flicker threshold expected");
    if (!(blend_strength >= 0.0f && blend_strength <= 1.0f)) return invalid(fn, "a blend strength in [0, 1] expected");
    if (((uintptr_t)mask_out & 3) || ((uintptr_t)area_out & 7)) return invalid(fn, "a 4-byte aligned mask plane and an 8-byte aligned area cell expected");
    if (out) {
        FrameMarks marks = {{(uintptr_t)out, 0}, {(uintptr_t)prev, 1}, {(uintptr_t)cur, 1}, {(uintptr_t)next, 1}};
        if (frames_overlap(marks, (size_t)height * width * 3)) return invalid(fn, "out overlaps a source frame");
    }
    hipStream_t st = (hipStream_t)stream;
    if (area_out)
        if (const int e = hip_status(fn, hipMemsetAsync(area_out, 0, sizeof(uint64_t), st))) return e;
    const dim3 grid((unsigned)((width + TC_TW - 1) / TC_TW), (unsigned)((height + TC_TH - 1) / TC_TH));
    hipLaunchKernelGGL(tcons_apply_kernel, grid, dim3(TC_NT), 0, st, prev, cur, next, height, width, flicker_threshold, blend_strength, out,
                       mask_out, (unsigned long long*)area_out);
    return hip_status(fn, hipGetLastError());
}

}  // extern "C"
