// Flicker reduction of the classical temporal denoise on the device, gfx950: the reference's Python path,
// `FlickerReducer._apply_python_deflicker` (temporal_denoise.py:764-836) - per frame, L of 8-bit gamma Lab (cv2.COLOR_BGR2LAB) is
// shifted by half of clip(target - mean L, -20, 20) and the frame goes back through COLOR_LAB2BGR.
//
// The contract is tests/flicker_ref.py (the sRGB and CIE Lab formulas in fixed point; cv2 parity unpinned) and the bar is
// bit-exactness: everything behind the construction of the tables is integer arithmetic.  The transforms are those of nlmeans.hip
// (lab_tables.h) with a 256-entry sRGB decode to the 0 .. 65280 scale in front of the 2^20-row matrix, and behind the inverse matrix -
// kept at 16 bits, clamped to 0 .. 65280 - an sRGB encode: a monotone 65281-entry table in the contract, 255 thresholds and an
// eight-step branchless search here.
//
//   fw_lab_l_sums_u8      sum of L per frame (frame = grid.z): decode, the Y row, one f(t) look-up; lane partials reduced across the
//                         wave by shuffles, one 64-bit vector atomic per wave.  Integer atomics commute.
//   fw_deflicker_lab_u8   BGR -> Lab -> L = lut[frame][L] -> BGR in one kernel: one read and one write of the frame.
//   fw_bgr_to_lab_u8 / fw_lab_to_bgr_u8   the two transforms alone, interleaved bytes (the same kernel, other modes).
//
// A lane takes four pixels as three aligned dwords where source and destination share their alignment: a frame's first
// (address & 3) pixels and its last (n - head) % 4 go byte by byte.  Every lane reads its pixels before it writes them and no
// other lane touches those bytes, so dst may alias src.  The small tables (decode, fy / Y / a / b, thresholds, the frame's LUT:
// 5.4 KiB) are copied to LDS per workgroup; the 65281-entry f(t) table (255 KiB) is gathered from global memory, where it stays in L2.
#include "stage_common.h"
#include "gamma_lab.h"

#include <cmath>
#include <map>
#include <mutex>
#include <vector>

namespace fw {
namespace {

constexpr int FK_NT = 256;
enum { MODE_FWD = 0, MODE_INV = 1, MODE_DEFLICKER = 2 };

// The per-pixel transforms (bgr_to_lab_px, lab_to_bgr_px, l_of_px) and SmallTables are gamma_lab.h's: t256 is read by MODE_INV and
// MODE_DEFLICKER, dec by MODE_FWD and MODE_DEFLICKER, lut by MODE_DEFLICKER.
// small_g: decode[256], thresholds[256] as int
template <int MODE>
__device__ __forceinline__ void load_small(SmallTables& s, const int* __restrict__ t256_g, const int* __restrict__ small_g,
                                           const uint8_t* __restrict__ lut_g) {
    const int tid = threadIdx.x;
    if (MODE != MODE_INV) s.dec[tid] = (uint16_t)small_g[tid];
    if (MODE != MODE_FWD) {
        s.thr[tid] = (uint16_t)small_g[256 + tid];
#pragma unroll
        for (int q = 0; q < 4; ++q) s.t256[q * 256 + tid] = t256_g[q * 256 + tid];
    }
    if (MODE == MODE_DEFLICKER) s.lut[tid] = lut_g[tid];
    __syncthreads();
}

template <int MODE>
__device__ __forceinline__ uint32_t map_px(uint32_t p, const SmallTables& s, const LabFwd& kf, const LabInv& ki,
                                           const int* __restrict__ cbrt_tab) {
    if (MODE == MODE_FWD) return bgr_to_lab_px(p, s, kf, cbrt_tab);
    if (MODE == MODE_INV) return lab_to_bgr_px(p, s, ki);
    const uint32_t lab = bgr_to_lab_px(p, s, kf, cbrt_tab);
    return lab_to_bgr_px((lab & 0xffff00u) | s.lut[lab & 255u], s, ki);
}

// How a frame of n pixels at address a splits: `head` pixels byte by byte, then `groups` of four pixels as three aligned dwords, then
// the rest byte by byte.  3 head = -head (mod 4), so head = a & 3 aligns the first group.  vec = 0: everything byte by byte.
struct Split {
    long head, groups, tail0, scalar;
};
__device__ __forceinline__ Split split_frame(const uint8_t* a, long n, int vec) {
    Split s;
    s.head = vec ? min((long)((uintptr_t)a & 3), n) : n;
    s.groups = (n - s.head) / 4;
    s.tail0 = s.head + s.groups * 4;
    s.scalar = s.head + (n - s.tail0);
    return s;
}

__device__ __forceinline__ uint32_t load_px(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }

// src and dst may be the same buffer: no __restrict__ on them
template <int MODE>
__global__ __launch_bounds__(FK_NT) void gamma_map_kernel(const uint8_t* src, uint8_t* dst, long npx, int vec, LabFwd kf, LabInv ki,
                                                          const int* __restrict__ cbrt_tab, const int* __restrict__ t256_g,
                                                          const int* __restrict__ small_g, const uint8_t* __restrict__ luts) {
    __shared__ SmallTables s;
    const int f = blockIdx.z;
    load_small<MODE>(s, t256_g, small_g, MODE == MODE_DEFLICKER ? luts + (size_t)f * 256 : nullptr);
    const size_t base = (size_t)f * (size_t)npx * 3;
    const uint8_t* sp = src + base;
    uint8_t* dp = dst + base;
    const Split sl = split_frame(sp, npx, vec);
    const long tid = (long)blockIdx.x * FK_NT + threadIdx.x, step = (long)gridDim.x * FK_NT;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sp + 3 * sl.head);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dp + 3 * sl.head);
    for (long g = tid; g < sl.groups; g += step) {
        const uint32_t w0 = sw[3 * g], w1 = sw[3 * g + 1], w2 = sw[3 * g + 2];
        const uint32_t o0 = map_px<MODE>(w0 & 0xffffffu, s, kf, ki, cbrt_tab);
        const uint32_t o1 = map_px<MODE>((w0 >> 24) | (w1 & 0xffffu) << 8, s, kf, ki, cbrt_tab);
        const uint32_t o2 = map_px<MODE>((w1 >> 16) | (w2 & 0xffu) << 16, s, kf, ki, cbrt_tab);
        const uint32_t o3 = map_px<MODE>(w2 >> 8, s, kf, ki, cbrt_tab);
        dw[3 * g] = o0 | o1 << 24;
        dw[3 * g + 1] = o1 >> 8 | o2 << 16;
        dw[3 * g + 2] = o2 >> 16 | o3 << 8;
    }
    for (long i = tid; i < sl.scalar; i += step) {
        const long p = i < sl.head ? i : sl.tail0 + (i - sl.head);
        const uint32_t o = map_px<MODE>(load_px(sp + 3 * p), s, kf, ki, cbrt_tab);
        dp[3 * p] = (uint8_t)o;
        dp[3 * p + 1] = (uint8_t)(o >> 8);
        dp[3 * p + 2] = (uint8_t)(o >> 16);
    }
}

__global__ __launch_bounds__(FK_NT) void l_sums_kernel(const uint8_t* __restrict__ frames, long npx, int vec, LabFwd kf,
                                                       const int* __restrict__ cbrt_tab, const int* __restrict__ small_g,
                                                       unsigned long long* l_sums) {
    __shared__ uint16_t dec[256];
    dec[threadIdx.x] = (uint16_t)small_g[threadIdx.x];
    __syncthreads();
    const int f = blockIdx.z;
    const uint8_t* sp = frames + (size_t)f * (size_t)npx * 3;
    const Split sl = split_frame(sp, npx, vec);
    const long tid = (long)blockIdx.x * FK_NT + threadIdx.x, step = (long)gridDim.x * FK_NT;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sp + 3 * sl.head);
    unsigned long long sum = 0;
    for (long g = tid; g < sl.groups; g += step) {
        const uint32_t w0 = sw[3 * g], w1 = sw[3 * g + 1], w2 = sw[3 * g + 2];
        sum += l_of_px(w0 & 0xffffffu, dec, kf, cbrt_tab) + l_of_px((w0 >> 24) | (w1 & 0xffffu) << 8, dec, kf, cbrt_tab) +
               l_of_px((w1 >> 16) | (w2 & 0xffu) << 16, dec, kf, cbrt_tab) + l_of_px(w2 >> 8, dec, kf, cbrt_tab);
    }
    for (long i = tid; i < sl.scalar; i += step) {
        const long p = i < sl.head ? i : sl.tail0 + (i - sl.head);
        sum += l_of_px(load_px(sp + 3 * p), dec, kf, cbrt_tab);
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(&l_sums[f], sum);
}

// ---- the tables this file adds (host, float64), operation for operation as tests/flicker_ref.py builds them ----
struct GammaTables {
    std::vector<int> decode, encode, thresholds;      // [256], [65281], [255]
};

const GammaTables& gamma_tables() {
    static const GammaTables t = [] {
        GammaTables r;
        r.decode.resize(256);
        for (int i = 0; i < 256; ++i) {
            const double x = (double)i / 255.0;
            const double lin = x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4);
            r.decode[i] = (int)std::nearbyint((double)LIN_MAX * lin);
        }
        r.encode.resize(LIN_MAX + 1);
        for (int i = 0; i <= LIN_MAX; ++i) {
            const double x = (double)i / (double)LIN_MAX;
            const double e = x <= 0.0031308 ? 12.92 * x : 1.055 * std::pow(x, 1.0 / 2.4) - 0.055;
            r.encode[i] = (int)std::nearbyint(255.0 * e);
        }
        r.thresholds.resize(255);
        int i = 0;
        for (int k = 0; k < 255; ++k) {                   // the first index whose entry exceeds k (the table is monotone)
            while (i <= LIN_MAX && r.encode[i] <= k) ++i;
            r.thresholds[k] = i;
        }
        return r;
    }();
    return t;
}

std::mutex g_mutex;
std::map<int, int*> g_small;          // per device: decode[256], thresholds[256] ([255] = 0xffff)

}  // namespace

int* device_gamma_small() {
    int dev = 0;
    FW_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_mutex);
    int*& d = g_small[dev];
    if (!d) {
        const GammaTables& t = gamma_tables();
        std::vector<int> v(t.decode);
        v.insert(v.end(), t.thresholds.begin(), t.thresholds.end());
        v.push_back(0xffff);
        int* p = nullptr;
        FW_HIP_CHECK(hipMalloc((void**)&p, v.size() * sizeof(int)));
        FW_HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
        d = p;
    }
    return d;
}

namespace {

constexpr long MAX_PIXELS = 1L << 30;

// workgroups per frame: a lane takes four pixels per step, and a workgroup stays long enough to pay for its copy of the tables
unsigned blocks_for(long npx, unsigned cap) {
    const long b = (npx + 4 * FK_NT - 1) / (4 * FK_NT);
    return (unsigned)(b < 1 ? 1 : b > (long)cap ? (long)cap : b);
}

template <int MODE>
void launch_map(const uint8_t* src, uint8_t* dst, int count, long npx, const uint8_t* luts, hipStream_t st) {
    const LabTables& t = lab_tables();
    const DeviceLab lab = device_lab();
    const int* small = device_gamma_small();
    const int vec = (((uintptr_t)src ^ (uintptr_t)dst) & 3) == 0;
    const dim3 grid(blocks_for(npx, 1024), 1, (unsigned)count);
    hipLaunchKernelGGL((gamma_map_kernel<MODE>), grid, dim3(FK_NT), 0, st, src, dst, npx, vec, t.fwd, t.inv, lab.cbrt_tab, lab.t256, small, luts);
    FW_HIP_CHECK(hipGetLastError());
}

std::string check_frames(const char* fn, int count, int height, int width) {
    const std::string p = std::string(fn) + ": ";
    if (count < 1 || count > 65535) return p + "1 .. 65535 frames per call expected";
    if (height < 1 || width < 1 || (long)height * width > MAX_PIXELS) return p + "bad frame size";
    return "";
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_bgr_to_lab_u8(const uint8_t* src_bgr, int64_t n_pixels, uint8_t* dst_lab, void* stream) {
    if (!src_bgr || !dst_lab) return fail(FW_ERR_INVALID, "fw_bgr_to_lab_u8: null pointer");
    if (n_pixels < 1 || n_pixels > MAX_PIXELS) return fail(FW_ERR_INVALID, "fw_bgr_to_lab_u8: 1 .. 2^30 pixels expected");
    return guarded([&] { launch_map<MODE_FWD>(src_bgr, dst_lab, 1, (long)n_pixels, nullptr, (hipStream_t)stream); });
}

int fw_lab_to_bgr_u8(const uint8_t* src_lab, int64_t n_pixels, uint8_t* dst_bgr, void* stream) {
    if (!src_lab || !dst_bgr) return fail(FW_ERR_INVALID, "fw_lab_to_bgr_u8: null pointer");
    if (n_pixels < 1 || n_pixels > MAX_PIXELS) return fail(FW_ERR_INVALID, "fw_lab_to_bgr_u8: 1 .. 2^30 pixels expected");
    return guarded([&] { launch_map<MODE_INV>(src_lab, dst_bgr, 1, (long)n_pixels, nullptr, (hipStream_t)stream); });
}

int fw_lab_l_sums_u8(const uint8_t* frames_bgr, int count, int height, int width, int64_t* l_sums, void* stream) {
    if (!frames_bgr || !l_sums) return fail(FW_ERR_INVALID, "fw_lab_l_sums_u8: null pointer");
    const std::string bad = check_frames("fw_lab_l_sums_u8", count, height, width);
    if (!bad.empty()) return fail(FW_ERR_INVALID, bad);
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const LabTables& t = lab_tables();
        const DeviceLab lab = device_lab();
        const int* small = device_gamma_small();
        const long npx = (long)height * width;
        FW_HIP_CHECK(hipMemsetAsync(l_sums, 0, (size_t)count * sizeof(int64_t), st));
        const dim3 grid(blocks_for(npx, 256), 1, (unsigned)count);
        hipLaunchKernelGGL(l_sums_kernel, grid, dim3(FK_NT), 0, st, frames_bgr, npx, 1, t.fwd, lab.cbrt_tab, small, (unsigned long long*)l_sums);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_deflicker_lab_u8(const uint8_t* frames_bgr, int count, int height, int width, const uint8_t* l_luts, uint8_t* dst_bgr, void* stream) {
    if (!frames_bgr || !l_luts || !dst_bgr) return fail(FW_ERR_INVALID, "fw_deflicker_lab_u8: null pointer");
    const std::string bad = check_frames("fw_deflicker_lab_u8", count, height, width);
    if (!bad.empty()) return fail(FW_ERR_INVALID, bad);
    return guarded([&] { launch_map<MODE_DEFLICKER>(frames_bgr, dst_bgr, count, (long)height * width, l_luts, (hipStream_t)stream); });
}

int fw_gamma_lab_tables(int which, int32_t* out, int capacity) {
    const GammaTables& t = gamma_tables();
    if (which < 0 || which > 2) {
        last_error_ref() = "fw_gamma_lab_tables: which must be 0 .. 2";
        return 0;
    }
    const std::vector<int>& v = which == 0 ? t.decode : which == 1 ? t.encode : t.thresholds;
    if (out) {
        if (capacity < (int)v.size()) {
            last_error_ref() = "fw_gamma_lab_tables: capacity too small";
            return 0;
        }
        memcpy(out, v.data(), v.size() * sizeof(int));
    }
    return (int)v.size();
}

}  // extern "C"
