// The frame path of the reference's frame quality scorer (src/framewright/processors/frame_quality_scorer.py: `score_frame` with
// `_calculate_sharpness`, `_calculate_noise`, `_calculate_exposure`, `_detect_blocking`, `_detect_banding`, `_detect_interlacing`,
// `_check_duplicate`, `_check_corrupted`) on uint8 BGR frames that are already in HBM.  Every measure the scorer takes is a short-stencil
// statistic of the gray plane or of L of Lab; one pass over the frame's bytes forms all of them as integers, and the host (quality.py)
// turns the integers into the scores.  tests/quality_ref.frame_statistics is the contract, held integer for integer.
//
//   fw_quality_scratch_bytes  what a call needs for its workgroups' partial sums and histograms
//   fw_quality_stats_u8   per frame: 11 int64 sums, the 256-bin histograms of gray and of all 3 H W bytes, the sum of |row i - row i-1|
//                         of gray for every i in range(8, H - 8, 8) and the same for columns, and the 32 x 32 thumbnail of gray.
//
// What the planes are (cv2's own bytes are unpinned, DESIGN K19): gray is the 14-bit form of stage_common.h; L is the L of
// tests/flicker_ref.bgr_to_lab_gamma - the sRGB decode table, the Y row of the 2^20 matrix and one look-up of f(t) (lab_tables.h);
// every stencil reads its plane with BORDER_REFLECT_101, and since both planes are pointwise functions of the pixel, the reflected
// plane is the plane of the reflected pixel.
//
// Kernel shape.  A workgroup of 256 lanes takes tiles of 32 rows x 64 columns (the height a multiple of 8, so the upper neighbour of a
// block-boundary row is in the tile or its halo).  It forms gray of the tile with a halo of 2 (the 5 x 5 blur) and L with a halo of 1
// (the Sobel) once per pixel into two byte planes in LDS (36 x 68 and 34 x 66 bytes), taking the byte sums and both histograms of the
// tile's own pixels on the way; then a wave owns 8 rows of the tile - lane = column, so adjacent lanes read adjacent LDS bytes, four
// to a bank word, which the LDS broadcasts - reads the 12 plane rows they reach once, evaluates every stencil from those registers and
// accumulates per lane.  The sum of a block-boundary row
// is one wave_sum; a block-boundary column is a lane's own sum over its 8 rows of the tile; both leave as integer atomic adds onto sums
// the entry has zeroed (a handful per tile, and an address is shared only by the tiles of one tile row or column).  A workgroup walks
// tiles with a stride of the grid (at most 1024 workgroups a frame, fewer per frame in a batch), keeps its histograms in LDS, and at its
// end reduces the lanes with wave_sum and leaves its 11 sums and 512 bins as a partial in the caller's scratch with plain stores.  A
// second, tiny launch adds the partials of a frame - adjacent lanes take adjacent bins, so the loads coalesce - and forms the
// thumbnail, four gray taps per output straight from the frame.  Everything is an integer, so no order matters and two runs give the same numbers.  (A first
// form added every workgroup's sums and bins with atomics: 4096 atomics on each of 11 addresses cost 0.4 ms a call, whatever the
// frame's size.)
//
// Accumulator widths, from the worst case of a 0 / 255 checkerboard at 16384 x 16384 (N = 2^28 pixels, 3 N bytes):
//   |lap| <= 4 * 255 = 1020       sum lap^2   <= 1020^2 * 2^28 = 2.8e14   int64 (the sum of lap itself is signed, |.| <= 2.8e11)
//   d = |gray - blur| <= 255      sum d^2     <= 255^2 * 2^28  = 1.7e13   int64
//   |sobel_xy| <= 2 * 255         its sum     <= 510 * 2^28    = 1.4e11   int64
//   row / column pair differences  each sum   <= 255 * 2^27    = 3.4e10   int64
//   bytes                          sum v^2    <= 255^2 * 3 * 2^28 = 5.2e13 int64;  sum v <= 2.1e11
//   gradient counts <= 2^28, histogram bins <= 3 * 2^28 = 8.1e8 < 2^32    uint32 bins; the counts travel with the int64 sums
//   a block-boundary row or column <= 255 * 16384 = 4.2e6                 uint32
// Every lane accumulator is 64 bits wide, so no bound depends on how many tiles a workgroup walks; a workgroup's LDS bin holds at most
// its own share of 3 N bytes, below 2^32.
#include "lab_tables.h"
#include "stage_common.h"

#include <cmath>

namespace fw {
namespace {

constexpr int QS_NT = 256;
constexpr int QS_FT = 1024;                                          // lanes of the finishing workgroup
constexpr int QS_BATCH = 32;
constexpr int QS_TH = 32, QS_TW = 64;                                 // the tile: a wave is a tile row
constexpr int QS_GH = QS_TH + 4, QS_GW = QS_TW + 4;                   // gray with a halo of 2
constexpr int QS_LH = QS_TH + 2, QS_LW = QS_TW + 2;                   // L with a halo of 1
constexpr int QS_BLOCKS = 1024;                                       // workgroups a frame, at most
constexpr int QS_STAGE = 5;                                           // positions a lane stages at a time
constexpr int QS_SUMS = 12;                                           // int64 a frame: 11 used
constexpr int QS_THUMB = 32;
enum { S_LAP, S_LAP2, S_NOISE, S_NOISE2, S_EDGE, S_STRONG, S_WEAK, S_ROWPAIR, S_COLPAIR, S_BYTES, S_BYTES2 };

struct QsFrames {
    const uint8_t* p[QS_BATCH];
};
struct QsDecode {
    uint16_t v[256];
};
struct QsThumb {
    int xofs[QS_THUMB], yofs[QS_THUMB];
    short ia[2 * QS_THUMB], ib[2 * QS_THUMB];
    int mode;                                                         // 0 the same size: a copy, 1 an exact halving: the 2 x 2 mean, 2 linear
};

// the index into f(t) of the Y row, (coef . decoded + 2^19) >> 20: 0 .. 65280 (the row sums to 2^20)
__device__ __forceinline__ int qs_y_index(uint32_t b, uint32_t g, uint32_t r, const uint16_t* dec, const LabFwd& k) {
    const unsigned long long s = (unsigned long long)(uint32_t)k.coef[3] * dec[b] + (unsigned long long)(uint32_t)k.coef[4] * dec[g] +
                                 (unsigned long long)(uint32_t)k.coef[5] * dec[r] + (1ull << (COEF_BITS - 1));
    return (int)(s >> COEF_BITS);
}

__device__ __forceinline__ int qs_l_of_fy(int fy, const LabFwd& k) {
    constexpr int sh = F_BITS + L_SCALE_BITS;
    return min(max((k.l_scale * fy - k.l_offset + (1 << (sh - 1))) >> sh, 0), 255);
}

__global__ __launch_bounds__(QS_NT) void qs_stats_kernel(const QsFrames frames, int H, int W, int tiles_x, int tiles, const QsDecode dec_arg,
                                                         const LabFwd kf, const int* __restrict__ cbrt_tab, long long* part_sums,
                                                         uint32_t* part_hists, uint32_t* blocks, int nbr, int nbc) {
    __shared__ uint8_t gp[QS_GH][QS_GW];
    __shared__ uint8_t lp[QS_LH][QS_LW];
    __shared__ uint32_t hist[512];                                    // gray, then bytes
    __shared__ uint16_t dec[256];
    __shared__ long long wave_sums[QS_NT / 64][QS_SUMS];
    const int tid = threadIdx.x, f = blockIdx.y;
    const uint8_t* img = frames.p[f];
    uint32_t* frame_blocks = blocks + (long)f * (nbr + nbc);
    dec[tid] = dec_arg.v[tid];
    hist[tid] = 0, hist[256 + tid] = 0;
    __syncthreads();
    long long acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int lx = tid & 63, wave = tid >> 6;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * QS_TH, tx0 = (tile % tiles_x) * QS_TW;
        // both planes of the tile, once per pixel; what lies further outside the frame than a stencil of a pixel inside reaches is left.
        // Five positions a lane at a time, in three steps - the pixels, the f(t) look-ups, the planes and sums - so that five loads of a
        // kind are in flight where a loop over single positions would wait for each in turn.
        for (int i0 = tid; i0 < QS_GH * QS_GW; i0 += QS_NT * QS_STAGE) {
            uint32_t pix[QS_STAGE];
            int fy[QS_STAGE];
            bool ok[QS_STAGE];
#pragma unroll
            for (int j = 0; j < QS_STAGE; ++j) {
                const int i = i0 + j * QS_NT, py = i / QS_GW, px = i - py * QS_GW;
                const int y = ty0 + py - 2, x = tx0 + px - 2;
                ok[j] = i < QS_GH * QS_GW && y < H + 2 && x < W + 2;
                pix[j] = 0;
                if (ok[j]) {
                    const uint8_t* p = img + ((long)reflect101(y, H) * W + reflect101(x, W)) * 3;
                    pix[j] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
                }
            }
#pragma unroll
            for (int j = 0; j < QS_STAGE; ++j) {
                const int i = i0 + j * QS_NT, py = i / QS_GW, px = i - py * QS_GW;
                fy[j] = 0;
                if (ok[j] && py >= 1 && py < QS_GH - 1 && px >= 1 && px < QS_GW - 1)
                    fy[j] = cbrt_tab[qs_y_index(pix[j] & 255u, (pix[j] >> 8) & 255u, pix[j] >> 16, dec, kf)];
            }
#pragma unroll
            for (int j = 0; j < QS_STAGE; ++j) {
                if (!ok[j]) continue;
                const int i = i0 + j * QS_NT, py = i / QS_GW, px = i - py * QS_GW;
                const int y = ty0 + py - 2, x = tx0 + px - 2;
                const uint32_t b = pix[j] & 255u, g = (pix[j] >> 8) & 255u, r = pix[j] >> 16;
                const int gv = (int)((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14);
                gp[py][px] = (uint8_t)gv;
                if (py >= 1 && py < QS_GH - 1 && px >= 1 && px < QS_GW - 1) lp[py - 1][px - 1] = (uint8_t)qs_l_of_fy(fy[j], kf);
                if (py >= 2 && py < QS_GH - 2 && px >= 2 && px < QS_GW - 2 && y < H && x < W) {
                    acc[S_BYTES] += b + g + r;
                    acc[S_BYTES2] += b * b + g * g + r * r;
                    atomicAdd(&hist[gv], 1u);
                    atomicAdd(&hist[256 + b], 1u), atomicAdd(&hist[256 + g], 1u), atomicAdd(&hist[256 + r], 1u);
                }
            }
        }
        __syncthreads();
        // a wave takes 8 consecutive rows of the tile, a lane one column of them: the 12 plane rows they reach are read once - five
        // bytes a row for the blur's row sum, of which the middle three serve the 3 x 3 stencils - and shared by the 8 pixels
        const int x = tx0 + lx, r0 = wave * 8;
        const bool col_line = (x & 7) == 0 && x >= 8 && x < W - 8;
        uint32_t col_acc = 0;                                         // at most 255 * 8
        int rsum[12], gl[12], gc[12], gr[12], ldf[10];
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const uint8_t* row = &gp[r0 + q][lx];
            gl[q] = row[1], gc[q] = row[2], gr[q] = row[3];
            rsum[q] = row[0] + 4 * gl[q] + 6 * gc[q] + 4 * gr[q] + row[4];
        }
#pragma unroll
        for (int q = 0; q < 10; ++q) ldf[q] = (int)lp[r0 + q][lx + 2] - (int)lp[r0 + q][lx];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int y = ty0 + r0 + k;
            const bool in = y < H && x < W;
            const int c = gc[k + 2], up = gc[k + 1], down = gc[k + 3], left = gl[k + 2], right = gr[k + 2];
            if (in) {
                const int lap = up + down + left + right - 4 * c;
                acc[S_LAP] += lap, acc[S_LAP2] += lap * lap;
                const int blur = rsum[k] + 4 * rsum[k + 1] + 6 * rsum[k + 2] + 4 * rsum[k + 3] + rsum[k + 4];
                const int d = abs(c - ((blur + 128) >> 8));
                acc[S_NOISE] += d, acc[S_NOISE2] += d * d;
                acc[S_EDGE] += abs(gl[k + 1] - gr[k + 1] - gl[k + 3] + gr[k + 3]);
                const int grad = abs(ldf[k] + 2 * ldf[k + 1] + ldf[k + 2]);
                acc[S_STRONG] += grad > 30, acc[S_WEAK] += grad > 5 && grad <= 30;
                if (!(y & 1)) acc[S_ROWPAIR] += abs(c - down);        // H is even: row y + 1 is a row of the frame
                if (!(x & 1)) acc[S_COLPAIR] += abs(c - right);
                if (col_line) col_acc += (uint32_t)abs(c - left);
            }
            if (k == 0 && y >= 8 && y < H - 8) {                      // y is a multiple of 8 there; the same for all 64 lanes of the wave
                const uint32_t s = wave_sum(in ? (uint32_t)abs(c - up) : 0u);   // at most 255 * 64
                if (lx == 0) atomicAdd(frame_blocks + (y / 8 - 1), s);
            }
        }
        if (col_line && col_acc) atomicAdd(frame_blocks + nbr + (x / 8 - 1), col_acc);
        __syncthreads();
    }
    // the workgroup's partial: [frame][workgroup][12] sums and [frame][workgroup][512] bins
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const long long s = wave_sum(acc[k]);
        if (lx == 0) wave_sums[wave][k] = s;
    }
    __syncthreads();
    const long slot = (long)f * gridDim.x + blockIdx.x;
    if (tid < QS_SUMS) part_sums[slot * QS_SUMS + tid] = tid < 11 ? wave_sums[0][tid] + wave_sums[1][tid] + wave_sums[2][tid] + wave_sums[3][tid] : 0;
    part_hists[slot * 512 + tid] = hist[tid];
    part_hists[slot * 512 + 256 + tid] = hist[256 + tid];
}

// One workgroup of 1024 lanes a frame: adds the frame's partials, and forms cv2.resize(gray, (32, 32)) as oracle/face_ref.resize_linear_u8
// states it; gray is formed from the frame at each of the four taps.  The partials are added by four lanes a bin and 64 lanes a sum, each
// over every fourth or 64th workgroup with its loads unrolled, and joined through LDS: one lane a bin over 1024 partials is a chain
// of 1024 load latencies (measured: 0.36 ms, the whole cost of a 1080p call).
__global__ __launch_bounds__(QS_FT) void qs_finish_kernel(const QsFrames frames, int H, int W, const QsThumb t, const long long* __restrict__ part_sums,
                                                          const uint32_t* __restrict__ part_hists, int groups, long long* sums, uint32_t* hists,
                                                          uint8_t* thumbs) {
    __shared__ uint32_t bins[QS_FT / 256][512];
    __shared__ long long parts[QS_FT / 16][QS_SUMS];
    const uint8_t* img = frames.p[blockIdx.x];
    const int tid = threadIdx.x;
    const long first = (long)blockIdx.x * groups;
    {
        const int bin = tid & 255, part = tid >> 8;
        uint32_t lo = 0, hi = 0;                                      // a bin of a frame: at most 3 * 2^28
#pragma unroll 8
        for (int g = part; g < groups; g += QS_FT / 256) lo += part_hists[(first + g) * 512 + bin], hi += part_hists[(first + g) * 512 + 256 + bin];
        bins[part][bin] = lo, bins[part][256 + bin] = hi;
        const int k = tid & 15, slice = tid >> 4;
        long long s = 0;
        if (k < QS_SUMS) {
#pragma unroll 4
            for (int g = slice; g < groups; g += QS_FT / 16) s += part_sums[(first + g) * QS_SUMS + k];
            parts[slice][k] = s;
        }
    }
    __syncthreads();
    if (tid < 512) hists[(long)blockIdx.x * 512 + tid] = bins[0][tid] + bins[1][tid] + bins[2][tid] + bins[3][tid];
    if (tid < QS_SUMS) {
        long long s = 0;
        for (int j = 0; j < QS_FT / 16; ++j) s += parts[j][tid];
        sums[(long)blockIdx.x * QS_SUMS + tid] = s;
    }
    for (int i = threadIdx.x; i < QS_THUMB * QS_THUMB; i += QS_FT) {
        const int dy = i >> 5, dx = i & 31;
        const auto g = [&](int y, int x) { return gray_bgr<3>(img + ((long)y * W + x) * 3); };
        int v;
        if (t.mode == 0) {
            v = g(dy, dx);
        } else if (t.mode == 1) {
            v = (g(2 * dy, 2 * dx) + g(2 * dy, 2 * dx + 1) + g(2 * dy + 1, 2 * dx) + g(2 * dy + 1, 2 * dx + 1) + 2) >> 2;
        } else {
            const int sx = t.xofs[dx], sy = t.yofs[dy];
            const int sx1 = min(sx + 1, W - 1), sy1 = min(sy + 1, H - 1);
            const int a0 = t.ia[2 * dx], a1 = t.ia[2 * dx + 1], b0 = t.ib[2 * dy], b1 = t.ib[2 * dy + 1];
            const int h0 = g(sy, sx) * a0 + g(sy, sx1) * a1, h1 = g(sy1, sx) * a0 + g(sy1, sx1) * a1;
            v = min(max((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 0), 255);
        }
        thumbs[(long)blockIdx.x * (QS_THUMB * QS_THUMB) + i] = (uint8_t)v;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// OpenCV's table of the 8-bit linear resize, as frame_ops.hip and oracle/face_ref.py build it: float fx from a double product, both
// borders clamped with fx = 0, 11-bit coefficients rounded half to even
void qs_linear_table(int ssize, int* ofs, short* coef) {
    const double inv_scale = (double)QS_THUMB / ssize, scale = 1. / inv_scale;
    for (int d = 0; d < QS_THUMB; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s0 = (int)std::floor(f);
        f -= s0;
        if (s0 < 0) f = 0.f, s0 = 0;
        if (s0 >= ssize - 1) f = 0.f, s0 = ssize - 1;
        ofs[d] = s0;
        coef[2 * d] = (short)std::lrintf((1.f - f) * 2048.f);
        coef[2 * d + 1] = (short)std::lrintf(f * 2048.f);
    }
}

const QsDecode& qs_decode() {
    static const QsDecode d = [] {
        QsDecode r{};
        int32_t v[256];
        (void)fw_gamma_lab_tables(0, v, 256);
        for (int i = 0; i < 256; ++i) r.v[i] = (uint16_t)v[i];
        return r;
    }();
    return d;
}

int qs_lines(int length) { return length > 16 ? (length - 9) / 8 : 0; }   // len(range(8, length - 8, 8))

int qs_tiles(int height, int width) { return ((width + QS_TW - 1) / QS_TW) * ((height + QS_TH - 1) / QS_TH); }

// workgroups a frame: a tile each up to 1024 for a single frame, about 2048 a launch for a batch, never fewer than 64
int qs_groups(int n, int height, int width) { return std::min(qs_tiles(height, width), std::min(QS_BLOCKS, std::max(64, 2 * QS_BLOCKS / n))); }

constexpr size_t QS_PARTIAL = sizeof(int64_t) * QS_SUMS + sizeof(uint32_t) * 512;   // bytes a workgroup leaves

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

size_t fw_quality_scratch_bytes(int n, int height, int width) {
    if (n < 1 || n > QS_BATCH || height < 1 || height > MAX_FRAME_SIDE || width < 1 || width > MAX_FRAME_SIDE) return 0;
    return (size_t)n * qs_groups(n, height, width) * QS_PARTIAL;
}

int fw_quality_stats_u8(const void* const* frames, int n, int height, int width, void* scratch, int64_t* sums, uint32_t* histograms,
                        uint32_t* block_sums, uint8_t* thumbnails, void* stream) {
    const char* fn = "fw_quality_stats_u8";
    if (const int s = check_side_and_channels(fn, height, width, 3)) return s;
    if ((height | width) & 1) return invalid(fn, "an even number of rows and of columns expected");
    if (const int s = check_pointer_table(fn, frames, n, QS_BATCH)) return s;
    if (!scratch || !sums || !histograms || !block_sums || !thumbnails) return invalid(fn, "null pointer");
    if ((uintptr_t)scratch % 8 || (uintptr_t)sums % 8) return invalid(fn, "scratch and sums must be 8-byte aligned");
    const int nbr = qs_lines(height), nbc = qs_lines(width), groups = qs_groups(n, height, width);
    const size_t frame_bytes = (size_t)height * width * 3;
    const size_t out_bytes[5] = {sizeof(int64_t) * QS_SUMS * n, sizeof(uint32_t) * 512 * n, sizeof(uint32_t) * (size_t)(nbr + nbc) * n,
                                 (size_t)QS_THUMB * QS_THUMB * n, (size_t)n * groups * QS_PARTIAL};
    const void* outs[5] = {sums, histograms, block_sums, thumbnails, scratch};
    for (int k = 0; k < 5; ++k)                                       // an output inside a frame would be read as pixels
        for (int i = 0; i < n && out_bytes[k]; ++i)
            if ((uintptr_t)outs[k] < (uintptr_t)frames[i] + frame_bytes && (uintptr_t)frames[i] < (uintptr_t)outs[k] + out_bytes[k])
                return invalid(fn, "an output or the scratch overlaps a frame of the call");
    for (int k = 0; k < 4; ++k)                                       // the partials are read while the outputs are written
        if (out_bytes[k] && (uintptr_t)outs[k] < (uintptr_t)scratch + out_bytes[4] && (uintptr_t)scratch < (uintptr_t)outs[k] + out_bytes[k])
            return invalid(fn, "an output overlaps the scratch");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const LabTables& tables = lab_tables();
        const DeviceLab lab = device_lab();
        QsFrames t{};
        for (int i = 0; i < n; ++i) t.p[i] = (const uint8_t*)frames[i];
        QsThumb th{};
        th.mode = (height == QS_THUMB && width == QS_THUMB) ? 0 : (height == 2 * QS_THUMB && width == 2 * QS_THUMB) ? 1 : 2;
        qs_linear_table(width, th.xofs, th.ia);
        qs_linear_table(height, th.yofs, th.ib);
        long long* part_sums = (long long*)scratch;
        uint32_t* part_hists = (uint32_t*)((char*)scratch + sizeof(int64_t) * QS_SUMS * (size_t)n * groups);
        if (out_bytes[2]) FW_HIP_CHECK(hipMemsetAsync(block_sums, 0, out_bytes[2], st));
        const int tiles_x = (width + QS_TW - 1) / QS_TW, tiles = qs_tiles(height, width);
        hipLaunchKernelGGL(qs_stats_kernel, dim3((unsigned)groups, (unsigned)n), dim3(QS_NT), 0, st, t, height, width, tiles_x, tiles, qs_decode(),
                           tables.fwd, lab.cbrt_tab, part_sums, part_hists, block_sums, nbr, nbc);
        FW_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(qs_finish_kernel, dim3((unsigned)n), dim3(QS_FT), 0, st, t, height, width, th, part_sums, part_hists, groups,
                           (long long*)sums, histograms, thumbnails);
        FW_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
