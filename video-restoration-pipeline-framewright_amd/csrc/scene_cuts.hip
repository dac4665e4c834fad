// The two scene-cut tests of the reference's `FrameInterpolator` (src/framewright/processors/interpolation.py:267-366) on the
// device, on the uint8 frames the interpolator has already uploaded:
//
//   fw_scene_ssim_u8   skimage's structural_similarity (defaults, data_range 255) of the mean-gray images of `pairs` frame pairs
//   fw_hist64x3_u8     the 3 x 64-bin histograms of the fallback test (np.histogram(bins=64, range=(0, 256)) per channel)
//
// tests/scene_cut_ref.py is the contract; skimage parity is unpinned (it is absent where this is built).
//
// SSIM.  skimage crops 3 pixels from the map before the mean, so every 7 x 7 window that counts lies inside the image: no border
// rule, N = (H - 6)(W - 6) values.  On uint8 the window sums Sx, Sy, Sxx, Syy, Sxy are integers below 2^22, and the central moments
// mxx = 49 Sxx - Sx^2, myy, mxy = 49 Sxy - Sx Sy (signed) are exact integers below 2^28: everything up to there is int32.  With
// numerator and denominator multiplied by 49^2 * (49 * 48),
//     S = ((2 Sx Sy + K1) (2 mxy + K2)) / ((Sx^2 + Sy^2 + K1) (mxx + myy + K2)),   K1 = 2401 C1, K2 = 2352 C2,
// and float64 enters with the four additions of K1 / K2 to exact integers: four additions, two products, one division, each
// correctly rounded (-ffp-contract=off in build.py: no product is fused into anything), the contract's order.
//
// A workgroup of 256 threads owns a 64 x 32 tile of the map of one pair (pair = grid.z).  The 70 x 38 pixels under it are read once
// per frame as aligned 32-bit words into LDS (a frame of a contiguous clip may start at any byte: H W 3 can be odd), turned into two
// gray byte planes there, and each wave then walks 8 map rows down its 64 columns: the seven-pixel row sums of the five products
// come from LDS, the vertical direction is a running sum over a seven-row ring held in registers.
//
// Determinism.  A lane adds its 8 values in row order, a wave reduces by shuffles in a fixed tree, the four waves are added in
// order, and the workgroup stores that one float64 into the workspace slot it owns.  A second kernel, one wave per pair, adds the
// pair's slots - lane l takes l, l + 64, ... in order, then the same shuffle tree - and divides by N.  No floating-point atomics:
// the value of a pair depends on H, W and its bytes alone, not on the run, the batch it is in or where its frames lie.
//
// Histograms.  A workgroup takes 8192 pixels of one frame (frame = grid.y), each wave bumps a private 3 x 64 LDS table, and the
// workgroup ends with at most 192 32-bit integer vector atomics.  Integer atomics commute: the counts are exact.
#include "stage_common.h"

namespace fw {
namespace {

constexpr int SC_TW = 64, SC_TH = 32, SC_NT = 256, SC_WAVES = SC_NT / 64, SC_ROWS = SC_TH / SC_WAVES;   // 8 map rows per wave
constexpr int SC_IW = SC_TW + 6, SC_IH = SC_TH + 6;                   // 70 x 38 pixels under a tile
constexpr int SC_RAW_WORDS = (3 + SC_IW * 3 + 3) / 4;                 // 54: a row's 210 bytes from any alignment, in aligned words
constexpr int SC_RAW_LD = SC_RAW_WORDS + 1;                           // words per staged row
constexpr int SC_GLD = 72;                                            // bytes per gray row
constexpr int HS_NT = 256, HS_WAVES = HS_NT / 64, HS_PIX = 8192;      // pixels of one workgroup of the histogram kernel

constexpr double SC_C1 = (0.01 * 255.0) * (0.01 * 255.0), SC_C2 = (0.03 * 255.0) * (0.03 * 255.0);
constexpr double SC_K1 = SC_C1 * 2401.0, SC_K2 = SC_C2 * 2352.0;

__global__ __launch_bounds__(SC_NT) void scene_ssim_tile_kernel(const uint8_t* __restrict__ frames_a, const uint8_t* __restrict__ frames_b,
                                                                long stride, int H, int W, double* __restrict__ partial) {
    __shared__ uint32_t s_raw[2 * SC_IH * SC_RAW_LD];
    __shared__ uint8_t s_g[2 * SC_IH * SC_GLD];
    __shared__ double s_part[SC_WAVES];
    const int tid = threadIdx.x, x0 = blockIdx.x * SC_TW, y0 = blockIdx.y * SC_TH;
    const size_t frame_bytes = (size_t)H * W * 3;
    const uint8_t* fr_a = frames_a + (size_t)blockIdx.z * stride;
    const uint8_t* fr_b = frames_b + (size_t)blockIdx.z * stride;
    const int cols = min(SC_IW, W - x0), rows = min(SC_IH, H - y0);   // pixels of the frame under this tile (both >= 7)

    // 1. the rows' bytes, as the aligned words that cover them
    for (int i = tid; i < 2 * SC_IH * SC_RAW_WORDS; i += SC_NT) {
        const int pr = i / SC_RAW_WORDS, k = i - pr * SC_RAW_WORDS;   // pr = plane * SC_IH + row
        const int pl = pr >= SC_IH, r = pr - pl * SC_IH;
        if (r >= rows) continue;
        const uint8_t* frame = pl ? fr_b : fr_a;
        const uint8_t* row = frame + ((size_t)(y0 + r) * W + x0) * 3;
        const int off = (int)((uintptr_t)row & 3);
        if (4 * k >= off + cols * 3) continue;
        s_raw[pr * SC_RAW_LD + k] = load_word_inside(row - off + 4 * k, frame, frame + frame_bytes);
    }
    __syncthreads();
    // 2. gray = (c0 + c1 + c2) / 3; outside the frame 0 (only map positions that are not stored read those)
    for (int i = tid; i < 2 * SC_IH * SC_IW; i += SC_NT) {
        const int pr = i / SC_IW, c = i - pr * SC_IW;
        const int pl = pr >= SC_IH, r = pr - pl * SC_IH;
        uint8_t g = 0;
        if (r < rows && c < cols) {
            const uint8_t* row = (pl ? fr_b : fr_a) + ((size_t)(y0 + r) * W + x0) * 3;
            const uint8_t* b = reinterpret_cast<const uint8_t*>(&s_raw[pr * SC_RAW_LD]) + ((uintptr_t)row & 3) + 3 * c;
            g = (uint8_t)(((int)b[0] + b[1] + b[2]) / 3);
        }
        s_g[pr * SC_GLD + c] = g;
    }
    __syncthreads();
    // 3. eight map rows down one column
    const int col = tid & 63, wv = tid >> 6;
    const bool col_ok = x0 + col < W - 6;
    const int oy0 = y0 + wv * SC_ROWS;
    double acc = 0.0;
    if (oy0 < H - 6) {                                                // wave-uniform
        int ring[7][5];
        int v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0;
#pragma unroll
        for (int r = 0; r < SC_ROWS + 6; ++r) {
            const uint8_t* pa = &s_g[(wv * SC_ROWS + r) * SC_GLD + col];
            const uint8_t* pb = pa + SC_IH * SC_GLD;
            int h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const int a = pa[k], b = pb[k];
                h0 += a;
                h1 += b;
                h2 += a * a;
                h3 += b * b;
                h4 += a * b;
            }
            if (r >= 7) {
                v0 -= ring[r % 7][0];
                v1 -= ring[r % 7][1];
                v2 -= ring[r % 7][2];
                v3 -= ring[r % 7][3];
                v4 -= ring[r % 7][4];
            }
            ring[r % 7][0] = h0;
            ring[r % 7][1] = h1;
            ring[r % 7][2] = h2;
            ring[r % 7][3] = h3;
            ring[r % 7][4] = h4;
            v0 += h0;
            v1 += h1;
            v2 += h2;
            v3 += h3;
            v4 += h4;
            if (r >= 6) {
                const int mxx = 49 * v2 - v0 * v0, myy = 49 * v3 - v1 * v1, mxy = 49 * v4 - v0 * v1;
                const double a1 = (double)(2 * v0 * v1) + SC_K1, a2 = (double)(2 * mxy) + SC_K2;
                const double b1 = (double)(v0 * v0 + v1 * v1) + SC_K1, b2 = (double)(mxx + myy) + SC_K2;
                const double s = (a1 * a2) / (b1 * b2);
                if (col_ok && oy0 + (r - 6) < H - 6) acc += s;
            }
        }
    }
    acc = wave_sum(acc);                                              // only lane 0 of a wave stores its sum
    if (col == 0) s_part[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = s_part[0];
#pragma unroll
        for (int w = 1; w < SC_WAVES; ++w) t += s_part[w];
        partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// one wave per pair: the pair's `tiles` partials in a fixed order, over N
__global__ __launch_bounds__(64) void scene_ssim_finish_kernel(const double* __restrict__ partial, int tiles, double n, double* __restrict__ ssim) {
    const double* p = partial + (size_t)blockIdx.x * tiles;
    double t = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 64) t += p[i];
    t = wave_sum(t);                                                  // only lane 0 stores
    if (threadIdx.x == 0) ssim[blockIdx.x] = t / n;
}

__global__ __launch_bounds__(HS_NT) void hist64x3_kernel(const uint8_t* __restrict__ frames, long n_pix, uint32_t* hist) {
    __shared__ uint32_t s_hist[HS_WAVES][192];
    const int tid = threadIdx.x;
    const uint8_t* frame = frames + (size_t)blockIdx.y * n_pix * 3;
    for (int i = tid; i < HS_WAVES * 192; i += HS_NT) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    uint32_t* my = s_hist[tid >> 6];
    const long p0 = (long)blockIdx.x * HS_PIX, p1 = min(p0 + HS_PIX, n_pix);
    if (((uintptr_t)frame & 3) == 0) {                                // block-uniform: four pixels = three aligned words per lane
        for (long p = p0 + 4 * tid; p < p1; p += 4 * HS_NT) {
            if (p + 4 <= p1) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(frame + p * 3);
                const uint32_t w[3] = {q[0], q[1], q[2]};
#pragma unroll
                for (int k = 0; k < 12; ++k) atomicAdd(&my[(k % 3) * 64 + (((w[k >> 2] >> (8 * (k & 3))) & 255u) >> 2)], 1u);
            } else {
                for (long i = p * 3; i < p1 * 3; ++i) atomicAdd(&my[(int)(i % 3) * 64 + (frame[i] >> 2)], 1u);
            }
        }
    } else {
        for (long p = p0 + tid; p < p1; p += HS_NT) {
            const uint8_t* q = frame + p * 3;
            atomicAdd(&my[q[0] >> 2], 1u);
            atomicAdd(&my[64 + (q[1] >> 2)], 1u);
            atomicAdd(&my[128 + (q[2] >> 2)], 1u);
        }
    }
    __syncthreads();
    if (tid < 192) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < HS_WAVES; ++w) v += s_hist[w][tid];
        if (v) atomicAdd(&hist[(size_t)blockIdx.y * 192 + tid], v);
    }
}

// tiles of one pair's map, 0 for a size the kernel does not take
size_t sc_tiles(int pairs, int H, int W) {
    if (pairs < 1 || pairs > 65535 || H < 7 || W < 7 || (long)H * W > (1L << 30)) return 0;
    const size_t ty = (H - 6 + SC_TH - 1) / SC_TH, tx = (W - 6 + SC_TW - 1) / SC_TW;
    return ty > 65535 ? 0 : tx * ty;
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

size_t fw_scene_ssim_workspace_bytes(int pairs, int height, int width) {
    return sc_tiles(pairs, height, width) * (size_t)(pairs > 0 ? pairs : 0) * sizeof(double);
}

int fw_scene_ssim_u8(const uint8_t* frames_a, const uint8_t* frames_b, int64_t frame_stride_bytes, int pairs, int height, int width,
                     double* ssim, void* workspace, void* stream) {
    if (!frames_a || !frames_b || !ssim || !workspace) return fail(FW_ERR_INVALID, "fw_scene_ssim_u8: null pointer");
    if (pairs < 1 || pairs > 65535) return fail(FW_ERR_INVALID, "fw_scene_ssim_u8: 1 .. 65535 pairs per call expected");
    if (height < 7 || width < 7)
        return fail(FW_ERR_INVALID, "fw_scene_ssim_u8: the 7 x 7 window exceeds the image (the caller falls back to the histogram test)");
    const size_t tiles = sc_tiles(pairs, height, width);
    if (tiles == 0) return fail(FW_ERR_INVALID, "fw_scene_ssim_u8: bad frame size");
    if (frame_stride_bytes < 0 || (pairs > 1 && frame_stride_bytes == 0))
        return fail(FW_ERR_INVALID, "fw_scene_ssim_u8: bad frame stride");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const dim3 grid((width - 6 + SC_TW - 1) / SC_TW, (height - 6 + SC_TH - 1) / SC_TH, pairs);
        hipLaunchKernelGGL(scene_ssim_tile_kernel, grid, dim3(SC_NT), 0, st, frames_a, frames_b, (long)frame_stride_bytes, height, width,
                           (double*)workspace);
        FW_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(scene_ssim_finish_kernel, dim3(pairs), dim3(64), 0, st, (const double*)workspace, (int)tiles,
                           (double)((long)(height - 6) * (width - 6)), ssim);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_hist64x3_u8(const uint8_t* frames, int count, int height, int width, uint32_t* hist, void* stream) {
    if (!frames || !hist) return fail(FW_ERR_INVALID, "fw_hist64x3_u8: null pointer");
    if (count < 1 || count > 65535) return fail(FW_ERR_INVALID, "fw_hist64x3_u8: 1 .. 65535 frames per call expected");
    if (height < 1 || width < 1 || (long)height * width > (1L << 30)) return fail(FW_ERR_INVALID, "fw_hist64x3_u8: bad frame size");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const long n_pix = (long)height * width;
        FW_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)count * 192 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(hist64x3_kernel, dim3((unsigned)((n_pix + HS_PIX - 1) / HS_PIX), count), dim3(HS_NT), 0, st, frames, n_pix, hist);
        FW_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
