// The two frame hashes of the reference's `FrameDeduplicator` (src/framewright/processors/deduplication.py:106-164) on the device,
// on uint8 BGR frames that are already in HBM.  Both are Pillow thumbnails, and Pillow's 8-bit resampler is integer arithmetic on a
// table of 22-bit coefficients, so the contract (tests/dedup_ref.py, held byte for byte against Pillow on the CPU) is byte equality:
//
//   fw_pil_lanczos_taps   HOST: the integer tap table of one resampling pass, Pillow's float64 arithmetic with libm's sin
//   fw_pil_thumb_u8       n frames -> n thumbnails: `convert('L')` and `resize((out_w, out_h), LANCZOS)` in either order
//   fw_dhash_pack_u8      the dHash bits px[r][c + 1] > px[r][c] of n (hs + 1) x hs thumbnails, packed first bit most significant
//
// Horizontal pass.  A workgroup of 256 threads walks rows y = blockIdx.x, blockIdx.x + gridDim.x, ... of one frame (frame =
// blockIdx.y).  A lane reads the 12 bytes of four pixels as the aligned 32-bit words that cover them (a frame of a contiguous clip
// may start at any byte: H W 3 can be odd) and leaves the gray row, or the three channel rows, in LDS.  Each wave then takes output
// columns in turn: its lanes stride the window (about 678 taps at 1920 -> 17), multiply bytes from LDS by taps from LDS, and a
// shuffle tree adds the 64 partial sums.  The taps stay in LDS for the whole walk when they fit (17 x 679 x 4 B does); at 8K width
// they do not and come through L2.  The 17 or 3 x 64 bytes of a row go to the workspace, planar per channel.
// Vertical pass.  One workgroup per output row and frame; wave per column, lanes stride the window down the workspace (a few KB, in
// L2 from the pass before), the same reduction, then the gray conversion when it comes second.
// A pass whose size does not change is left out, as Pillow leaves it out: the kernels copy.
//
// Every sum is uint32 with wrap-around, so any order of the additions gives Pillow's int32 result; no atomics anywhere.  A frame's
// thumbnail depends on its bytes and the sizes alone, not on the run, the batch it is in or where the frame lies.
#include "stage_common.h"

#include <math.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace fw {

// ---- host: Pillow's coefficients (ImagingResample's precompute_coeffs + normalize_coeffs_8bpc, restated) ----------------------------
// Compiled with -ffp-contract=off (build.py): w * 2^22 + 0.5 must round twice, as it does in Pillow.
namespace {

constexpr int PIL_PRECISION_BITS = 22;

double pil_sinc(double t) {
    if (t == 0.0) return 1.0;
    t = t * M_PI;
    return sin(t) / t;
}

double pil_lanczos(double t) {
    if (-3.0 <= t && t < 3.0) return pil_sinc(t) * pil_sinc(t / 3);
    return 0.0;
}

}  // namespace

int pil_lanczos_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(3.0 * fs) * 2 + 1;
}

void pil_lanczos_fill(int in_size, int out_size, int32_t* xmin, int32_t* count, int32_t* taps) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * fs;
    const int ks = pil_lanczos_ksize(in_size, out_size);
    std::vector<double> w((size_t)ks);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = pil_lanczos((x + lo - center + 0.5) / fs);
            ww += w[x];
        }
        int32_t* row = taps + (size_t)xx * ks;
        for (int x = 0; x < ks; ++x) {
            if (x >= n) {
                row[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            row[x] = v < 0 ? (int32_t)(v * (double)(1 << PIL_PRECISION_BITS) - 0.5) : (int32_t)(v * (double)(1 << PIL_PRECISION_BITS) + 0.5);
        }
        xmin[xx] = lo;
        count[xx] = n;
    }
}

namespace {

constexpr int PT_NT = 256, PT_WAVES = PT_NT / 64;
constexpr int PT_MAX_OUT = 65, PT_MAX_SIDE = 16384;
constexpr size_t PT_LDS_BUDGET = 60 * 1024;                           // dynamic LDS of the horizontal kernel
constexpr int PT_ROW_BLOCKS = 1024;                                   // workgroups of one horizontal launch, about

__device__ __forceinline__ uint32_t pil_clip8(uint32_t sum) {
    const int v = (int)(sum + (1u << (PIL_PRECISION_BITS - 1))) >> PIL_PRECISION_BITS;
    return (uint32_t)min(max(v, 0), 255);
}

__device__ __forceinline__ uint32_t pil_gray(uint32_t b, uint32_t g, uint32_t r) {
    return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
}

// tmp[frame][c][y][xx], c < C: C = 1 the resampled gray row, C = 3 the resampled B, G, R rows.  `table` = xmin[out_w], count[out_w],
// taps[out_w][ksize] in device memory, or null when out_w == W (the pass is left out: the rows are only converted).
template <bool LDS_TAPS>
__global__ __launch_bounds__(PT_NT) void pil_hpass_kernel(const uint8_t* __restrict__ frames, long stride, int H, int W, int out_w, int C,
                                                          const int32_t* __restrict__ table, int ksize, uint8_t* __restrict__ tmp) {
    extern __shared__ uint32_t s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Wp = (W + 3) & ~3;
    int32_t* s_xmin = reinterpret_cast<int32_t*>(s_mem);
    int32_t* s_count = s_xmin + out_w;
    int32_t* s_taps = s_count + out_w;
    uint8_t* s_px = reinterpret_cast<uint8_t*>(s_taps + (LDS_TAPS ? out_w * ksize : 0));    // C planes of Wp bytes
    const uint8_t* frame = frames + (size_t)blockIdx.y * stride;
    const uint8_t* frame_end = frame + (size_t)H * W * 3;
    uint8_t* out = tmp + (size_t)blockIdx.y * C * H * out_w;

    if (table) {
        for (int i = tid; i < 2 * out_w; i += PT_NT) s_xmin[i] = table[i];
        if (LDS_TAPS)
            for (int i = tid; i < out_w * ksize; i += PT_NT) s_taps[i] = table[2 * out_w + i];
    }
    const int32_t* taps = LDS_TAPS ? s_taps : table + 2 * out_w;

    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        __syncthreads();                                              // the row before has been read (first turn: the tables are stored)
        const uint8_t* row = frame + (size_t)y * W * 3;
        const uint32_t off = (uint32_t)((uintptr_t)row & 3);
        for (int q = tid; q < Wp / 4; q += PT_NT) {                   // four pixels: bytes [12 q, 12 q + 12) of the row
            const uint8_t* p = row - off + 12 * q;
            const uint32_t w0 = load_word_inside(p, frame, frame_end), w1 = load_word_inside(p + 4, frame, frame_end);
            const uint32_t w2 = load_word_inside(p + 8, frame, frame_end);
            const uint32_t w3 = off ? load_word_inside(p + 12, frame, frame_end) : 0u;
            const uint32_t d[3] = {__builtin_amdgcn_alignbyte(w1, w0, off), __builtin_amdgcn_alignbyte(w2, w1, off),
                                   __builtin_amdgcn_alignbyte(w3, w2, off)};
            uint32_t px[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) px[i] = (d[i >> 2] >> (8 * (i & 3))) & 255u;
            if (C == 1) {
                uint32_t g = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) g |= pil_gray(px[3 * j], px[3 * j + 1], px[3 * j + 2]) << (8 * j);
                reinterpret_cast<uint32_t*>(s_px)[q] = g;
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    reinterpret_cast<uint32_t*>(s_px + c * Wp)[q] = px[c] | (px[3 + c] << 8) | (px[6 + c] << 16) | (px[9 + c] << 24);
            }
        }
        __syncthreads();
        if (!table) {
            for (int i = tid; i < C * W; i += PT_NT) {
                const int c = i / W, x = i - c * W;
                out[((size_t)c * H + y) * out_w + x] = s_px[c * Wp + x];
            }
            continue;
        }
        for (int item = wv; item < C * out_w; item += PT_WAVES) {     // wave-uniform
            const int c = item / out_w, xx = item - c * out_w;
            const int cnt = s_count[xx];
            const uint8_t* px = s_px + c * Wp + s_xmin[xx];
            const int32_t* tp = taps + (size_t)xx * ksize;
            uint32_t s = 0;
            for (int k = lane; k < cnt; k += 64) s += (uint32_t)px[k] * (uint32_t)tp[k];
            s = wave_sum(s);
            if (lane == 0) out[((size_t)c * H + y) * out_w + xx] = (uint8_t)pil_clip8(s);
        }
    }
}

// thumbs[frame][yy][xx] from tmp[frame][c][y][xx]; `table` for H -> out_h, or null when out_h == H.  C = 3: the gray conversion follows.
__global__ __launch_bounds__(PT_NT) void pil_vpass_kernel(const uint8_t* __restrict__ tmp, int H, int out_w, int out_h, int C,
                                                          const int32_t* __restrict__ table, int ksize, uint8_t* __restrict__ thumbs) {
    __shared__ uint8_t s_res[3 * PT_MAX_OUT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int yy = blockIdx.x;
    const uint8_t* src = tmp + (size_t)blockIdx.y * C * H * out_w;
    const int lo = table ? table[yy] : yy, cnt = table ? table[out_h + yy] : 1;
    const int32_t* tp = table ? table + 2 * out_h + (size_t)yy * ksize : nullptr;
    for (int item = wv; item < C * out_w; item += PT_WAVES) {
        const int c = item / out_w, xx = item - c * out_w;
        const uint8_t* p = src + ((size_t)c * H + lo) * out_w + xx;
        if (!table) {
            if (lane == 0) s_res[item] = p[0];
            continue;
        }
        uint32_t s = 0;
        for (int k = lane; k < cnt; k += 64) s += (uint32_t)p[(size_t)k * out_w] * (uint32_t)tp[k];
        s = wave_sum(s);
        if (lane == 0) s_res[item] = (uint8_t)pil_clip8(s);
    }
    __syncthreads();
    if (tid < out_w) {
        const uint32_t v = C == 1 ? s_res[tid] : pil_gray(s_res[tid], s_res[out_w + tid], s_res[2 * out_w + tid]);
        thumbs[((size_t)blockIdx.y * out_h + yy) * out_w + tid] = (uint8_t)v;
    }
}

// One thread per output byte: bit i of a frame (row-major over hs x hs) sits `pad + i` bits from the top of its nbytes.
__global__ __launch_bounds__(PT_NT) void dhash_pack_kernel(const uint8_t* __restrict__ thumbs, int n, int hs, uint8_t* __restrict__ bits) {
    const int nbytes = (hs * hs + 7) / 8, pad = 8 * nbytes - hs * hs;
    const long i = (long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= (long)n * nbytes) return;
    const int b = (int)(i % nbytes);
    const uint8_t* t = thumbs + (size_t)(i / nbytes) * hs * (hs + 1);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = 8 * b + j - pad;
        uint32_t bit = 0;
        if (p >= 0) {
            const int r = p / hs, c = p - r * hs;
            bit = t[r * (hs + 1) + c + 1] > t[r * (hs + 1) + c];
        }
        v = (v << 1) | bit;
    }
    bits[i] = (uint8_t)v;
}

std::mutex g_mutex;
std::map<std::tuple<int, int, int>, int32_t*> g_tables;               // (device, in, out) -> xmin[out], count[out], taps[out][ksize]

// The table of one pass on the current device; the first call for a size allocates and copies (blocking), later calls look it up.
const int32_t* device_table(int in_size, int out_size) {
    int dev = 0;
    FW_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_mutex);
    int32_t*& d = g_tables[std::make_tuple(dev, in_size, out_size)];
    if (!d) {
        const int ks = pil_lanczos_ksize(in_size, out_size);
        std::vector<int32_t> v((size_t)out_size * (2 + ks));
        pil_lanczos_fill(in_size, out_size, v.data(), v.data() + out_size, v.data() + 2 * out_size);
        int32_t* p = nullptr;
        FW_HIP_CHECK(hipMalloc((void**)&p, v.size() * sizeof(int32_t)));
        FW_HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        d = p;
    }
    return d;
}

bool thumb_args_ok(int n, int H, int W, int out_w, int out_h) {
    return n >= 1 && n <= 65535 && H >= 1 && W >= 1 && H <= PT_MAX_SIDE && W <= PT_MAX_SIDE && out_w >= 1 && out_h >= 1 &&
           out_w <= PT_MAX_OUT && out_h <= PT_MAX_OUT;
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_pil_lanczos_taps(int in_size, int out_size, int32_t* xmin, int32_t* count, int32_t* taps, int capacity) {
    if (in_size < 1 || out_size < 1 || in_size > 65536 || out_size > 65536) return 0;
    const int ks = pil_lanczos_ksize(in_size, out_size);
    if (!xmin && !count && !taps) return ks;
    if (!xmin || !count || !taps || (long)capacity < (long)out_size * ks) return 0;
    pil_lanczos_fill(in_size, out_size, xmin, count, taps);
    return ks;
}

size_t fw_pil_thumb_workspace_bytes(int n, int height, int width, int out_w, int out_h, int gray_first) {
    if (!thumb_args_ok(n, height, width, out_w, out_h)) return 0;
    return (size_t)n * (gray_first ? 1 : 3) * height * out_w;
}

int fw_pil_thumb_u8(const uint8_t* frames_bgr, int64_t frame_stride_bytes, int n, int height, int width, int out_w, int out_h,
                    int gray_first, uint8_t* thumbs, void* workspace, void* stream) {
    if (!frames_bgr || !thumbs || !workspace) return fail(FW_ERR_INVALID, "fw_pil_thumb_u8: null pointer");
    if (!thumb_args_ok(n, height, width, out_w, out_h))
        return fail(FW_ERR_INVALID, "fw_pil_thumb_u8: 1 .. 65535 frames of 1 .. 16384 pixels a side and thumbnails of 1 .. 65 a side expected");
    if (frame_stride_bytes < 0 || (n > 1 && frame_stride_bytes == 0)) return fail(FW_ERR_INVALID, "fw_pil_thumb_u8: bad frame stride");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const int C = gray_first ? 1 : 3;
        const int32_t* ht = width != out_w ? device_table(width, out_w) : nullptr;
        const int32_t* vt = height != out_h ? device_table(height, out_h) : nullptr;
        const int hk = ht ? pil_lanczos_ksize(width, out_w) : 0, vk = vt ? pil_lanczos_ksize(height, out_h) : 0;
        const size_t planes = (size_t)C * ((width + 3) & ~3), small = (size_t)2 * out_w * sizeof(int32_t);
        const size_t with_taps = small + (size_t)out_w * hk * sizeof(int32_t) + planes;
        const bool lds_taps = ht && with_taps <= PT_LDS_BUDGET;
        const int row_blocks = std::min(height, std::max(1, PT_ROW_BLOCKS / n));
        const dim3 grid(row_blocks, n);
        if (lds_taps)
            hipLaunchKernelGGL(pil_hpass_kernel<true>, grid, dim3(PT_NT), with_taps, st, frames_bgr, (long)frame_stride_bytes, height, width,
                               out_w, C, ht, hk, (uint8_t*)workspace);
        else
            hipLaunchKernelGGL(pil_hpass_kernel<false>, grid, dim3(PT_NT), small + planes, st, frames_bgr, (long)frame_stride_bytes, height,
                               width, out_w, C, ht, hk, (uint8_t*)workspace);
        FW_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(pil_vpass_kernel, dim3(out_h, n), dim3(PT_NT), 0, st, (const uint8_t*)workspace, height, out_w, out_h, C, vt, vk,
                           thumbs);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_dhash_pack_u8(const uint8_t* thumbs, int n, int hash_size, uint8_t* bits, void* stream) {
    if (!thumbs || !bits) return fail(FW_ERR_INVALID, "fw_dhash_pack_u8: null pointer");
    if (n < 1 || n > 65535 || hash_size < 2 || hash_size > 64)
        return fail(FW_ERR_INVALID, "fw_dhash_pack_u8: 1 .. 65535 thumbnails and a hash size of 2 .. 64 expected");
    return guarded([&] {
        const long total = (long)n * ((hash_size * hash_size + 7) / 8);
        hipLaunchKernelGGL(dhash_pack_kernel, dim3((unsigned)((total + PT_NT - 1) / PT_NT)), dim3(PT_NT), 0, (hipStream_t)stream, thumbs, n,
                           hash_size, bits);
        FW_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
