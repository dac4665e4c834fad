// SDR to HDR conversion of final frames on the device, gfx950: the frame path of the reference's `HDRConverter.convert_frame`
// (src/framewright/processors/hdr_conversion.py:573-882) on uint8 / uint16 BGR frames that are already in HBM, to uint16 PQ or HLG.
// The contract is tests/hdr_ref.py, byte for byte (cv2's CLAHE, addWeighted, Lab and HSV as that file restates them; cv2 parity
// unpinned), and float32 bit for bit for the planes in front of the first quantisation under the three rational curves.
//
// Per pixel, steps 1 - 3 (`tone_px`): the gamma table built by the caller (256 or 65536 float32 entries: numpy's pow, evaluated
// once per code), the Rec.709 -> BT.2020 matrix as one rounded product and two fused multiply-adds per row (what the reference's
// float32 `np.dot` does; `__fmaf_rn`), the luminance, the curve and the scale, every operation rounded once: this file is compiled
// with contraction off and divides with `__fdiv_rn`.  Every constant that the reference writes as a Python float arrives in
// `fw_hdr_params` already rounded to float32 by the caller, so no decimal literal is rounded here a second time.
//
//   fw_hdr_convert      the whole conversion of n frames.
//     With a quantising step (local contrast, or a saturation boost): at most two passes over the frame and one small launch.
//       pass A (local contrast only)  tone map -> bytes -> Lab L; the 8 x 8 x 256 CLAHE tile histograms of the frame as padded by
//                reflect-101, eight tiles (one tile row, 8 KiB) in LDS per workgroup, then one global atomic per bin that is not zero.
//       small launch                  clip, redistribute, cumulate: 64 byte LUTs a frame.
//       pass B   the bytes again from the input (not stored: 3 B read beside 6 B written) -> Lab, CLAHE interpolation of L, the
//                half-and-half blend, Lab -> BGR -> integer HSV, the boost, float32 HSV -> BGR -> highlight flag -> the 2 x 256
//                tail table (transfer function and 16-bit quantisation of every byte, built by the caller) -> uint16.
//     Without one: one pass, the PQ / HLG transfer evaluated per pixel in float32 (powf / logf: DESIGN K20 has the error bound).
//   fw_hdr_tonemap_f32, fw_hdr_quantise_u8, fw_hdr_clahe_u8, fw_hdr_saturation_u8, fw_hdr_transfer_f32   the stages alone.
//
// A lane takes four pixels: three (uint8) or six (uint16) aligned dwords in, six dwords out, when source and destination start on
// a dword; else, and for the last n % 4 pixels, sample by sample.  No full-size float plane goes to memory.  Integer atomics only,
// so two runs give the same bytes.
#include "stage_common.h"
#include "gamma_lab.h"
#include "clahe.h"
#include "hsv_sat.h"

#include <cmath>

#pragma clang fp contract(off)

namespace fw {
namespace {

constexpr int HD_NT = 256;
constexpr int HD_MAX_FRAMES = 32;
constexpr int HD_MIN_SIDE = 8;
constexpr int HD_GRID = CL_GRID, HD_HIST = CL_HIST;              // clahe.h: tiles a side, bins a frame
constexpr int HD_BLOCKS = 2048;

struct Frames {
    const void* src[HD_MAX_FRAMES];
    void* dst[HD_MAX_FRAMES];
};

using Geo = ClaheGeo;

Geo geometry(int H, int W) { return clahe_geometry(H, W, clahe_limit(2.0, H, W)); }

__device__ __forceinline__ float curve_lum(const fw_hdr_params& P, float lum) {
    const float* k = P.curve_k;
    if (P.curve == 0) {                                           // REINHARD: k0 = (peak / 100)^2
        const float t = lum * (1.0f + __fdiv_rn(lum, k[0]));
        return __fdiv_rn(t, 1.0f + lum);
    }
    const float x = lum * k[0];                                   // the others: k0 = peak / 100
    if (P.curve == 1) {                                           // ACES: k1 .. k5 = a b c d e
        const float num = x * (k[1] * x + k[2]);
        const float den = x * (k[3] * x + k[4]) + k[5];
        return clipf(__fdiv_rn(num, den), 0.0f, 1.0f);
    }
    if (P.curve == 2) {                                           // HABLE: k1 A, k2 C B, k3 D E, k4 B, k5 D F, k6 E / F, k7 white scale
        const float num = x * (k[1] * x + k[2]) + k[3];
        const float den = x * (k[1] * x + k[4]) + k[5];
        return (__fdiv_rn(num, den) - k[6]) * k[7];
    }
    if (x <= k[1]) return x;                                      // MOBIUS: k1 transition, k2 1 - transition, k3 -slope
    const float e = expf(__fdiv_rn(k[3] * (x - k[1]), k[2]));
    return k[1] + k[2] * (1.0f - e);
}

// steps 1 - 3 on the linear samples: o = clip(c * scale, 0, 1) in stored order (B, G, R)
__device__ __forceinline__ void tone_px(const fw_hdr_params& P, float b, float g, float r, float* o) {
    if (P.use_matrix) {
        float m[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float t = P.matrix[3 * i] * r;
            t = __fmaf_rn(P.matrix[3 * i + 1], g, t);
            m[i] = __fmaf_rn(P.matrix[3 * i + 2], b, t);
        }
        r = m[0], g = m[1], b = m[2];
    }
    float lum = P.lum_weights[0] * b + P.lum_weights[1] * g;
    lum = lum + P.lum_weights[2] * r;
    lum = lum > P.lum_floor ? lum : P.lum_floor;
    const float lh = curve_lum(P, lum);
    const float scale = lum > P.lum_floor ? __fdiv_rn(lh, lum) : 1.0f;
    o[0] = clipf(b * scale, 0.0f, 1.0f);
    o[1] = clipf(g * scale, 0.0f, 1.0f);
    o[2] = clipf(r * scale, 0.0f, 1.0f);
}

__device__ __forceinline__ uint32_t quantise_px(const float* o) {
    return (uint32_t)(o[0] * 255.0f) | (uint32_t)(o[1] * 255.0f) << 8 | (uint32_t)(o[2] * 255.0f) << 16;
}

// the gamma table: LDS for the 256 codes of uint8 input, global (256 KiB, L2) for uint16
template <typename T>
__device__ __forceinline__ const float* stage_gamma(float* s_gamma, const float* __restrict__ gamma_g) {
    if (sizeof(T) == 1) {
        s_gamma[threadIdx.x] = gamma_g[threadIdx.x];
        return s_gamma;
    }
    return gamma_g;
}

// ---- how a lane walks a frame: four pixels as dwords where both ends are aligned ---------------------------------------------------
// body(p, c, o): pixel p with its samples c[3] (stored order) -> NOUT output samples o[] of type D
template <typename T, typename D, typename Body>
__device__ __forceinline__ void walk_pixels(const T* src, D* dst, long npx, Body body) {
    const long tid = (long)blockIdx.x * HD_NT + threadIdx.x, step = (long)gridDim.x * HD_NT;
    const bool vec = ((((uintptr_t)src) | ((uintptr_t)dst)) & 3) == 0;
    const long groups = vec ? npx / 4 : 0;
    constexpr int SW = 3 * sizeof(T), DW = 3 * sizeof(D);        // dwords of four pixels
    for (long g = tid; g < groups; g += step) {
        uint32_t w[SW], ow[DW];
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(src) + g * SW;
#pragma unroll
        for (int k = 0; k < SW; ++k) w[k] = sp[k];
        uint32_t c[12], o[12];
#pragma unroll
        for (int i = 0; i < 12; ++i)
            c[i] = sizeof(T) == 1 ? (w[i / 4] >> (8 * (i & 3))) & 255u : (w[i / 2] >> (16 * (i & 1))) & 65535u;
#pragma unroll
        for (int j = 0; j < 4; ++j) body(4 * g + j, c + 3 * j, o + 3 * j);
#pragma unroll
        for (int k = 0; k < DW; ++k) {
            if (sizeof(D) == 1) ow[k] = o[4 * k] | o[4 * k + 1] << 8 | o[4 * k + 2] << 16 | o[4 * k + 3] << 24;
            else if (sizeof(D) == 2) ow[k] = o[2 * k] | o[2 * k + 1] << 16;
            else ow[k] = o[k];
        }
        uint32_t* dp = reinterpret_cast<uint32_t*>(dst) + g * DW;
#pragma unroll
        for (int k = 0; k < DW; ++k) dp[k] = ow[k];
    }
    for (long p = 4 * groups + tid; p < npx; p += step) {
        uint32_t c[3], o[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = src[3 * p + i];
        body(p, c, o);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (sizeof(D) == 4) reinterpret_cast<uint32_t*>(dst)[3 * p + i] = o[i];
            else dst[3 * p + i] = (D)o[i];
        }
    }
}

unsigned walk_blocks(long npx) {
    const long b = (npx / 4 + HD_NT - 1) / HD_NT;
    return (unsigned)std::min<long>(std::max<long>(b, 1), HD_BLOCKS);
}

// ---- the stages alone -----------------------------------------------------------------------------------------------------------------
// OUT 0: the tone-mapped float32 plane (with `recover`, times the highlight gain where the flag is set); OUT 1: its bytes
template <typename T, int OUT>
__global__ __launch_bounds__(HD_NT) void front_kernel(const T* src, void* dst, long npx, fw_hdr_params P, const float* __restrict__ gamma_g,
                                                      int recover) {
    __shared__ float s_gamma[256];
    const float* gm = stage_gamma<T>(s_gamma, gamma_g);
    __syncthreads();
    auto tone = [&](const uint32_t* c, float* o) { tone_px(P, gm[c[0]], gm[c[1]], gm[c[2]], o); };
    if (OUT == 0) {
        walk_pixels<T, float>(src, (float*)dst, npx, [&](long, const uint32_t* c, uint32_t* out) {
            float o[3];
            tone(c, o);
            const bool flag = recover && (c[0] >= (uint32_t)P.clip_code || c[1] >= (uint32_t)P.clip_code || c[2] >= (uint32_t)P.clip_code);
#pragma unroll
            for (int i = 0; i < 3; ++i) out[i] = __float_as_uint(flag ? o[i] * P.recover_gain : o[i]);
        });
    } else {
        walk_pixels<T, uint8_t>(src, (uint8_t*)dst, npx, [&](long, const uint32_t* c, uint32_t* out) {
            float o[3];
            tone(c, o);
            const uint32_t q = quantise_px(o);
            out[0] = q & 255u, out[1] = (q >> 8) & 255u, out[2] = q >> 16;
        });
    }
}

// ---- CLAHE ---------------------------------------------------------------------------------------------------------------------------
// SRC 0 / 1: the L of the tone-mapped bytes of a uint8 / uint16 BGR frame; SRC 2: a given L plane.  grid (row chunks, 8 tile rows, n)
template <int SRC>
__global__ __launch_bounds__(HD_NT) void hist_kernel(Frames fr, Geo G, int rows_per_block, fw_hdr_params P, const float* __restrict__ gamma_g,
                                                     LabFwd kf, const int* __restrict__ cbrt_tab, const int* __restrict__ small_g,
                                                     uint32_t* __restrict__ hist_g) {
    __shared__ uint32_t s_hist[HD_GRID * 256];
    __shared__ float s_gamma[256];
    __shared__ uint16_t s_dec[256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < HD_GRID; ++k) s_hist[k * 256 + tid] = 0;
    const float* gm = gamma_g;
    if (SRC == 0) s_gamma[tid] = gamma_g[tid], gm = s_gamma;
    if (SRC != 2) s_dec[tid] = (uint16_t)small_g[tid];
    __syncthreads();
    const int f = blockIdx.z;
    clahe_count_rows(s_hist, G, rows_per_block, hist_g + (size_t)f * HD_HIST, [&](long p) -> uint32_t {
        if (SRC == 2) return static_cast<const uint8_t*>(fr.src[f])[p];
        uint32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            c[k] = SRC == 0 ? static_cast<const uint8_t*>(fr.src[f])[3 * p + k] : static_cast<const uint16_t*>(fr.src[f])[3 * p + k];
        float o[3];
        tone_px(P, gm[c[0]], gm[c[1]], gm[c[2]], o);
        return l_of_px(quantise_px(o), s_dec, kf, cbrt_tab);
    });
}

// the half-and-half blend of L with its CLAHE (clahe.h)
__device__ __forceinline__ uint32_t blend_half(uint32_t a, uint32_t b) {      // cv2.addWeighted(a, 0.5, b, 0.5, 0)
    return (uint32_t)__float2int_rn((float)a * 0.5f + (float)b * 0.5f);       // exact products and sum; at most 255
}

__global__ __launch_bounds__(HD_NT) void clahe_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, Geo G,
                                                            const uint8_t* __restrict__ luts) {
    const long npx = (long)G.H * G.W;
    for (long p = (long)blockIdx.x * HD_NT + threadIdx.x; p < npx; p += (long)gridDim.x * HD_NT) {
        const int y = (int)(p / G.W), x = (int)(p - (long)y * G.W);
        dst[p] = (uint8_t)clahe_px(luts, G, x, y, src[p]);
    }
}

// ---- HSV (the pixel body is hsv_sat.h's) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HD_NT) void saturation_kernel(const uint8_t* src, uint8_t* dst, long npx, const int* __restrict__ div_g,
                                                           float boost, float hue_scale) {
    __shared__ int s_div[512];
    s_div[threadIdx.x] = div_g[threadIdx.x], s_div[256 + threadIdx.x] = div_g[256 + threadIdx.x];
    __syncthreads();
    walk_pixels<uint8_t, uint8_t>(src, dst, npx, [&](long, const uint32_t* c, uint32_t* o) {
        const uint32_t q = saturate_px(c[0] | c[1] << 8 | c[2] << 16, s_div, boost, hue_scale);
        o[0] = q & 255u, o[1] = (q >> 8) & 255u, o[2] = q >> 16;
    });
}

// ---- the transfer functions in float32 (the path without a quantising step) --------------------------------------------------------
// PQ: k0 peak / 10000, k1 m1, k2 m2, k3 c1, k4 c2, k5 c3.  HLG: k0 1 / 12, k1 a, k2 b, k3 c.  -> trunc(clip(y * 65535, 0, 65535))
__device__ __forceinline__ uint32_t transfer_px(const fw_hdr_params& P, float x) {
    const float* k = P.transfer_k;
    const float e = clipf(x, 0.0f, 1.0f);
    float y;
    if (P.transfer == 0) {
        const float lm = powf(e * k[0], k[1]);
        y = powf(__fdiv_rn(k[3] + k[4] * lm, 1.0f + k[5] * lm), k[2]);
    } else {
        y = e <= k[0] ? __fsqrt_rn(3.0f * e) : k[1] * logf(12.0f * e - k[2]) + k[3];
    }
    return (uint32_t)clipf(clipf(y, 0.0f, 1.0f) * 65535.0f, 0.0f, 65535.0f);
}

__global__ __launch_bounds__(HD_NT) void transfer_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, long count, fw_hdr_params P) {
    for (long i = (long)blockIdx.x * HD_NT + threadIdx.x; i < count; i += (long)gridDim.x * HD_NT) dst[i] = (uint16_t)transfer_px(P, src[i]);
}

// ---- the frame -----------------------------------------------------------------------------------------------------------------------
// LC: local contrast (reads the frame's LUTs); SAT: the saturation boost; neither: the float path.  grid (blocks, 1, n)
template <typename T, bool LC, bool SAT>
__global__ __launch_bounds__(HD_NT) void final_kernel(Frames fr, Geo G, fw_hdr_params P, const float* __restrict__ gamma_g,
                                                      const uint16_t* __restrict__ tail_g, const int* __restrict__ div_g, LabFwd kf, LabInv ki,
                                                      const int* __restrict__ cbrt_tab, const int* __restrict__ t256_g,
                                                      const int* __restrict__ small_g, const uint8_t* __restrict__ luts_g) {
    __shared__ float s_gamma[256];
    __shared__ uint16_t s_tail[512];
    __shared__ int s_div[SAT ? 512 : 1];
    __shared__ SmallTables s_lab;
    const int tid = threadIdx.x, f = blockIdx.z;
    const float* gm = stage_gamma<T>(s_gamma, gamma_g);
    if (LC || SAT) s_tail[tid] = tail_g[tid], s_tail[256 + tid] = tail_g[256 + tid];
    if (SAT) s_div[tid] = div_g[tid], s_div[256 + tid] = div_g[256 + tid];
    if (LC) {
        s_lab.dec[tid] = (uint16_t)small_g[tid];
        s_lab.thr[tid] = (uint16_t)small_g[256 + tid];
#pragma unroll
        for (int q = 0; q < 4; ++q) s_lab.t256[q * 256 + tid] = t256_g[q * 256 + tid];
    }
    __syncthreads();
    const uint8_t* luts = LC ? luts_g + (size_t)f * HD_HIST : nullptr;
    const uint32_t clip_code = P.recover ? (uint32_t)P.clip_code : 0xffffffffu;
    walk_pixels<T, uint16_t>(static_cast<const T*>(fr.src[f]), static_cast<uint16_t*>(fr.dst[f]), (long)G.H * G.W,
                             [&](long p, const uint32_t* c, uint32_t* out) {
        float o[3];
        tone_px(P, gm[c[0]], gm[c[1]], gm[c[2]], o);
        const bool flag = c[0] >= clip_code || c[1] >= clip_code || c[2] >= clip_code;
        if (!LC && !SAT) {
#pragma unroll
            for (int i = 0; i < 3; ++i) out[i] = transfer_px(P, flag ? o[i] * P.recover_gain : o[i]);
            return;
        }
        uint32_t q = quantise_px(o);
        if (LC) {
            const uint32_t lab = bgr_to_lab_px(q, s_lab, kf, cbrt_tab);
            const int y = (int)(p / G.W), x = (int)(p - (long)y * G.W);
            const uint32_t L = lab & 255u;
            q = lab_to_bgr_px((lab & 0xffff00u) | blend_half(L, clahe_px(luts, G, x, y, L)), s_lab, ki);
        }
        if (SAT) q = saturate_px(q, s_div, P.saturation_boost, P.hue_scale);
        const uint16_t* tail = s_tail + (flag ? 256 : 0);
        out[0] = tail[q & 255u], out[1] = tail[(q >> 8) & 255u], out[2] = tail[q >> 16];
    });
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
int check_params(const char* fn, const fw_hdr_params* P) {
    if (!P) return invalid(fn, "null pointer");
    if (P->curve < 0 || P->curve > 3) return invalid(fn, "curve 0 (reinhard) .. 3 (mobius) expected");
    if (P->transfer < 0 || P->transfer > 1) return invalid(fn, "transfer 0 (PQ) or 1 (HLG) expected");
    if (P->clip_code < 0 || P->clip_code > 65536) return invalid(fn, "bad clip code");
    return FW_OK;
}

int check_frame(const char* fn, int H, int W, int sample_bytes) {
    if (H < HD_MIN_SIDE || H > MAX_FRAME_SIDE || W < HD_MIN_SIDE || W > MAX_FRAME_SIDE) return invalid(fn, "8 .. 16384 pixels a side expected");
    if (sample_bytes != 1 && sample_bytes != 2) return invalid(fn, "1 (uint8) or 2 (uint16) bytes a sample expected");
    return FW_OK;
}

template <int SRC>
void launch_hist(const Frames& fr, int n, const Geo& G, const fw_hdr_params& P, const float* gamma, uint32_t* hist, hipStream_t st) {
    const LabTables& t = lab_tables();
    const DeviceLab lab = device_lab();
    const int* small = device_gamma_small();
    const int rows = clahe_hist_rows_per_block(G);
    const dim3 grid(clahe_hist_chunks(G), HD_GRID, (unsigned)n);
    hipLaunchKernelGGL((hist_kernel<SRC>), grid, dim3(HD_NT), 0, st, fr, G, rows, P, gamma, t.fwd, lab.cbrt_tab, small, hist);
    FW_HIP_CHECK(hipGetLastError());
}

void launch_luts(int n, const Geo& G, const uint32_t* hist, uint8_t* luts, hipStream_t st) {
    hipLaunchKernelGGL(clahe_lut_kernel, dim3(HD_GRID * HD_GRID, (unsigned)n), dim3(CL_NT), 0, st, hist, luts, G.limit, G.lut_scale);
    FW_HIP_CHECK(hipGetLastError());
}

template <typename T>
void launch_final(const Frames& fr, int n, const Geo& G, const fw_hdr_params& P, const float* gamma, const uint16_t* tail, const int* div,
                  const uint8_t* luts, hipStream_t st) {
    const LabTables& t = lab_tables();
    const DeviceLab lab = device_lab();
    const int* small = device_gamma_small();
    const dim3 grid(walk_blocks((long)G.H * G.W), 1, (unsigned)n);
    const bool lc = P.local_contrast != 0, sat = P.saturation != 0;
#define FW_HDR_FINAL(LC, SAT)                                                                                                              \
    hipLaunchKernelGGL((final_kernel<T, LC, SAT>), grid, dim3(HD_NT), 0, st, fr, G, P, gamma, tail, div, t.fwd, t.inv, lab.cbrt_tab, lab.t256, \
                       small, luts)
    if (lc && sat) FW_HDR_FINAL(true, true);
    else if (lc) FW_HDR_FINAL(true, false);
    else if (sat) FW_HDR_FINAL(false, true);
    else FW_HDR_FINAL(false, false);
#undef FW_HDR_FINAL
    FW_HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

size_t fw_hdr_scratch_bytes(int n) {
    if (n < 1 || n > HD_MAX_FRAMES) return 0;
    return (size_t)n * HD_HIST * (sizeof(uint32_t) + 1);
}

int fw_hdr_convert(const void* const* frames, void* const* dst, int n, int height, int width, int sample_bytes, const fw_hdr_params* params,
                   const float* gamma, const uint16_t* tail, const int32_t* hsv_div, void* scratch, void* stream) {
    const char* fn = "fw_hdr_convert";
    if (const int st = check_pointer_table(fn, frames, n, HD_MAX_FRAMES)) return st;
    if (const int st = check_pointer_table(fn, (const void* const*)dst, n, HD_MAX_FRAMES)) return st;
    if (const int st = check_frame(fn, height, width, sample_bytes)) return st;
    if (const int st = check_params(fn, params)) return st;
    if (!gamma) return invalid(fn, "null pointer");
    const bool lc = params->local_contrast != 0, sat = params->saturation != 0;
    if ((lc || sat) && !tail) return invalid(fn, "null pointer");
    if (sat && !hsv_div) return invalid(fn, "null pointer");
    if (lc && (!scratch || ((uintptr_t)scratch & 3))) return invalid(fn, "a 4-byte aligned scratch of fw_hdr_scratch_bytes(n) expected");
    const size_t in_bytes = (size_t)height * width * 3 * sample_bytes, out_bytes = (size_t)height * width * 6;
    Frames fr;
    for (int i = 0; i < n; ++i) {
        if (((uintptr_t)frames[i] & (sample_bytes - 1)) || ((uintptr_t)dst[i] & 1)) return invalid(fn, "16-bit frames start on even addresses");
        fr.src[i] = frames[i], fr.dst[i] = dst[i];
        for (int j = 0; j < n; ++j) {
            const uintptr_t d = (uintptr_t)dst[i], s = (uintptr_t)frames[j], d2 = (uintptr_t)dst[j];
            if ((d < s + in_bytes && s < d + out_bytes) || (i != j && d < d2 + out_bytes && d2 < d + out_bytes))
                return invalid(fn, "a destination overlaps a frame or another destination of the call");
        }
    }
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const Geo G = geometry(height, width);
        uint8_t* luts = nullptr;
        if (lc) {
            uint32_t* hist = static_cast<uint32_t*>(scratch);
            luts = reinterpret_cast<uint8_t*>(hist + (size_t)n * HD_HIST);
            FW_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n * HD_HIST * sizeof(uint32_t), st));
            if (sample_bytes == 1) launch_hist<0>(fr, n, G, *params, gamma, hist, st);
            else launch_hist<1>(fr, n, G, *params, gamma, hist, st);
            launch_luts(n, G, hist, luts, st);
        }
        if (sample_bytes == 1) launch_final<uint8_t>(fr, n, G, *params, gamma, tail, hsv_div, luts, st);
        else launch_final<uint16_t>(fr, n, G, *params, gamma, tail, hsv_div, luts, st);
    });
}

int fw_hdr_tonemap_f32(const void* frame, int height, int width, int sample_bytes, const fw_hdr_params* params, const float* gamma,
                       int recover, float* dst, void* stream) {
    const char* fn = "fw_hdr_tonemap_f32";
    if (!frame || !gamma || !dst) return invalid(fn, "null pointer");
    if (const int st = check_frame(fn, height, width, sample_bytes)) return st;
    if (const int st = check_params(fn, params)) return st;
    if (((uintptr_t)frame & (sample_bytes - 1)) || ((uintptr_t)dst & 3)) return invalid(fn, "misaligned frame or destination");
    const long npx = (long)height * width;
    const dim3 grid(walk_blocks(npx));
    if (sample_bytes == 1)
        hipLaunchKernelGGL((front_kernel<uint8_t, 0>), grid, dim3(HD_NT), 0, (hipStream_t)stream, (const uint8_t*)frame, (void*)dst, npx, *params, gamma, recover);
    else
        hipLaunchKernelGGL((front_kernel<uint16_t, 0>), grid, dim3(HD_NT), 0, (hipStream_t)stream, (const uint16_t*)frame, (void*)dst, npx, *params, gamma, recover);
    return hip_status(fn, hipGetLastError());
}

int fw_hdr_quantise_u8(const void* frame, int height, int width, int sample_bytes, const fw_hdr_params* params, const float* gamma,
                       uint8_t* dst, void* stream) {
    const char* fn = "fw_hdr_quantise_u8";
    if (!frame || !gamma || !dst) return invalid(fn, "null pointer");
    if (const int st = check_frame(fn, height, width, sample_bytes)) return st;
    if (const int st = check_params(fn, params)) return st;
    if ((uintptr_t)frame & (sample_bytes - 1)) return invalid(fn, "16-bit frames start on even addresses");
    const long npx = (long)height * width;
    const dim3 grid(walk_blocks(npx));
    if (sample_bytes == 1)
        hipLaunchKernelGGL((front_kernel<uint8_t, 1>), grid, dim3(HD_NT), 0, (hipStream_t)stream, (const uint8_t*)frame, (void*)dst, npx, *params, gamma, 0);
    else
        hipLaunchKernelGGL((front_kernel<uint16_t, 1>), grid, dim3(HD_NT), 0, (hipStream_t)stream, (const uint16_t*)frame, (void*)dst, npx, *params, gamma, 0);
    return hip_status(fn, hipGetLastError());
}

int fw_hdr_clahe_u8(const uint8_t* plane, int height, int width, void* scratch, uint8_t* dst, void* stream) {
    const char* fn = "fw_hdr_clahe_u8";
    if (!plane || !dst) return invalid(fn, "null pointer");
    if (const int st = check_frame(fn, height, width, 1)) return st;
    if (!scratch || ((uintptr_t)scratch & 3)) return invalid(fn, "a 4-byte aligned scratch of fw_hdr_scratch_bytes(1) expected");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const Geo G = geometry(height, width);
        uint32_t* hist = static_cast<uint32_t*>(scratch);
        uint8_t* luts = reinterpret_cast<uint8_t*>(hist + HD_HIST);
        FW_HIP_CHECK(hipMemsetAsync(hist, 0, HD_HIST * sizeof(uint32_t), st));
        Frames fr{};
        fr.src[0] = plane;
        fw_hdr_params none{};
        launch_hist<2>(fr, 1, G, none, nullptr, hist, st);
        launch_luts(1, G, hist, luts, st);
        const long blocks = std::min<long>(((long)height * width + HD_NT - 1) / HD_NT, HD_BLOCKS);
        hipLaunchKernelGGL(clahe_apply_kernel, dim3((unsigned)blocks), dim3(HD_NT), 0, st, plane, dst, G, (const uint8_t*)luts);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_hdr_saturation_u8(const uint8_t* bgr, int64_t n_pixels, const int32_t* hsv_div, float boost, float hue_scale, uint8_t* dst, void* stream) {
    const char* fn = "fw_hdr_saturation_u8";
    if (!bgr || !hsv_div || !dst) return invalid(fn, "null pointer");
    if (n_pixels < 1 || n_pixels > (int64_t)MAX_FRAME_SIDE * MAX_FRAME_SIDE) return invalid(fn, "1 .. 2^28 pixels expected");
    hipLaunchKernelGGL(saturation_kernel, dim3(walk_blocks((long)n_pixels)), dim3(HD_NT), 0, (hipStream_t)stream, bgr, dst, (long)n_pixels, hsv_div,
                       boost, hue_scale);
    return hip_status(fn, hipGetLastError());
}

int fw_hdr_transfer_f32(const float* plane, int64_t count, const fw_hdr_params* params, uint16_t* dst, void* stream) {
    const char* fn = "fw_hdr_transfer_f32";
    if (!plane || !dst) return invalid(fn, "null pointer");
    if (const int st = check_params(fn, params)) return st;
    if (count < 1 || count > 3ll * MAX_FRAME_SIDE * MAX_FRAME_SIDE) return invalid(fn, "1 .. 3 x 2^28 values expected");
    if (((uintptr_t)plane & 3) || ((uintptr_t)dst & 1)) return invalid(fn, "misaligned plane or destination");
    const long blocks = std::min<long>((count + HD_NT - 1) / HD_NT, HD_BLOCKS);
    hipLaunchKernelGGL(transfer_kernel, dim3((unsigned)blocks), dim3(HD_NT), 0, (hipStream_t)stream, plane, dst, (long)count, *params);
    return hip_status(fn, hipGetLastError());
}

}  // extern "C"
