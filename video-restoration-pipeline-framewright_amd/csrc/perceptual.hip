// Perceptual tuning of final frames on the device (kernel set K24), gfx950: the frame path of the reference's
// `PerceptualTuner.apply_to_frame` (src/framewright/processors/perceptual_tuning.py:254-322) on uint8 BGR H x W x 3 frames that are
// already in HBM.  tests/perceptual_ref.py is the contract, byte for byte.  The steps, each optional, in the reference's order:
//
//   denoise   fastNlMeansDenoisingColored(x, None, h, h, 7, 21): fw_nlmeans_colored_u8, as it is
//   sharpen   blur = GaussianBlur(x, (0, 0), 3), 19 taps in 8-bit fixed point (rows into 16 bits, columns into 32, (v + 2^15) >> 16,
//             reflect-101 as often as it takes); x = addWeighted(x, w_src, blur, w_blur)
//   colour    BGR -> HSV, s = trunc(clip(s * boost, 0, 255)), HSV -> BGR (hsv_sat.h)
//   detail    BGR -> Lab, L = CLAHE(limit, 8 x 8)(L), Lab -> BGR (gamma_lab.h, clahe.h): L is replaced, not blended
//   grain     g = gray(ORIGINAL frame); grain = max(g - GaussianBlur(g, (5, 5), 0), 0); x = addWeighted(x, 1.0, grain, amount)
//
// One kernel template does every per-pixel and stencil step: `ptune_kernel<SHARPEN, COLOUR, DETAIL, GRAIN>`.  A workgroup of 256
// threads owns a 64 x 32 tile of the output.
//   sharpen   the tile and its 9-pixel reflect-101 halo as bytes in LDS (50 x 82 pixels), the 19 taps along rows into a 16-bit LDS
//             plane (50 x 64 x 3), the 19 taps along columns from it, `aw_byte` per channel.  The table is a constant array whose taps
//             fold into the unrolled loops (the outermost two are 0).  No intermediate plane in HBM.
//   grain     the gray of the original's tile and its 2-pixel halo in LDS (36 x 68), 1 4 6 4 1 along rows into 16 bits, along columns,
//             (v + 128) >> 8, the saturating difference, `aw_byte(x, 1.0f, grain, amount)`: the product and the sum each round once
//             (this file is compiled with contraction off; one fused multiply-add here changes bytes).
//   A thread finishes eight pixels of its column; colour and detail are per pixel between the two.
//
// fw_ptune_apply_u8, behind the optional denoise launch:
//   detail off  one launch, src -> dst (nothing on: one copy).
//   detail on   pass A  sharpen and colour -> bytes in scratch (left out where neither runs);
//               the 8 x 8 x 256 histograms of their Lab L over the frame as padded by reflect-101 (a launch of its own over the stored
//               bytes, clahe.h's tile-row loop: a 64 x 32 stencil tile cuts across CLAHE tiles - on a small frame it holds all 64 -
//               so counting inside pass A would take 64 KiB of LDS histograms beside the stencil planes, or one global atomic a pixel);
//               clip, redistribute, cumulate: 64 LUTs;
//               pass B  bytes -> Lab, L through the LUTs, Lab -> BGR, the grain stencil of the original, the final addWeighted.
//   No float plane and no Lab plane goes to memory.  Integer atomics only, so two runs give the same bytes.
#include "stage_common.h"
#include "gamma_lab.h"
#include "add_weighted.h"
#include "clahe.h"
#include "hsv_sat.h"

#include <cmath>

#pragma clang fp contract(off)

namespace fw {
namespace {

// tests/perceptual_ref.gauss19_table(): exp(-x^2 / 18) over its sum, 8 fractional bits, the rounding error carried from both ends
#define PT_K19_VALUES 0, 1, 3, 4, 9, 14, 20, 28, 32, 34, 32, 28, 20, 14, 9, 4, 3, 1, 0

constexpr int PT_TW = 64, PT_TH = 32, PT_NT = 256, PT_ROWS = PT_TH / (PT_NT / 64);      // 8 output rows per thread
constexpr int PT_TAPS = 19, PT_R = PT_TAPS / 2;
constexpr int PT_SW = PT_TW + 2 * PT_R, PT_SH = PT_TH + 2 * PT_R;                       // 82 x 50 staged pixels
constexpr int PT_SLD = PT_SW * 3 + 2;                                                   // bytes per staged row
constexpr int PT_HLD = PT_TW * 3;                                                       // 16-bit values per row-pass row
constexpr int PT_GW = PT_TW + 4, PT_GH = PT_TH + 4;                                     // 68 x 36 gray pixels
constexpr int PT_BLOCKS = 2048;
constexpr int PT_MIN_SIDE = 3;
constexpr size_t PT_ALIGN = 256;

struct Consts {
    float w_src, w_blur, boost, hue_scale, amount;
};

template <bool SHARPEN, bool COLOUR, bool DETAIL, bool GRAIN>
__global__ __launch_bounds__(PT_NT) void ptune_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ orig, uint8_t* __restrict__ out,
                                                      int H, int W, Consts c, ClaheGeo geo, const uint8_t* __restrict__ luts,
                                                      const int* __restrict__ div_g, LabFwd kf, LabInv ki, const int* __restrict__ cbrt_tab,
                                                      const int* __restrict__ t256_g, const int* __restrict__ small_g) {
    __shared__ uint8_t s_src[SHARPEN ? PT_SH * PT_SLD : 4];
    __shared__ uint16_t s_h[SHARPEN ? PT_SH * PT_HLD : 2];
    __shared__ uint8_t s_g[GRAIN ? PT_GH * PT_GW : 4];
    __shared__ uint16_t s_gh[GRAIN ? PT_GH * PT_TW : 2];
    __shared__ int s_div[COLOUR ? 512 : 1];
    __shared__ SmallTables s_lab;
    constexpr int k19[PT_TAPS] = {PT_K19_VALUES};
    const int tid = threadIdx.x, x0 = blockIdx.x * PT_TW, y0 = blockIdx.y * PT_TH;

    static_assert(PT_NT == 256, "one thread per table entry");
    if (COLOUR) s_div[tid] = div_g[tid], s_div[256 + tid] = div_g[256 + tid];
    if (DETAIL) {
        s_lab.dec[tid] = (uint16_t)small_g[tid];
        s_lab.thr[tid] = (uint16_t)small_g[256 + tid];
#pragma unroll
        for (int q = 0; q < 4; ++q) s_lab.t256[q * 256 + tid] = t256_g[q * 256 + tid];
    }
    // 1. the tile and its halo: every staged position is a pixel of the frame (reflect-101, as often as it takes)
    if (SHARPEN) {
        for (int i = tid; i < PT_SH * PT_SW; i += PT_NT) {
            const int r = i / PT_SW, cx = i - r * PT_SW;
            const uint8_t* p = in + ((size_t)reflect101(y0 - PT_R + r, H) * W + reflect101(x0 - PT_R + cx, W)) * 3;
            uint8_t* s = &s_src[r * PT_SLD + cx * 3];
            s[0] = p[0], s[1] = p[1], s[2] = p[2];
        }
    }
    if (GRAIN) {
        for (int i = tid; i < PT_GH * PT_GW; i += PT_NT) {
            const int r = i / PT_GW, cx = i - r * PT_GW;
            s_g[i] = (uint8_t)gray_bgr<3>(orig + ((size_t)reflect101(y0 - 2 + r, H) * W + reflect101(x0 - 2 + cx, W)) * 3);
        }
    }
    __syncthreads();
    // 2. along rows: at most 255 * 256 (16 bits) / 16 * 255
    if (SHARPEN) {
        for (int i = tid; i < PT_SH * PT_HLD; i += PT_NT) {
            const int r = i / PT_HLD, j = i - r * PT_HLD;
            const uint8_t* s = &s_src[r * PT_SLD + j];
            int acc = 0;
#pragma unroll
            for (int t = 0; t < PT_TAPS; ++t)
                if (k19[t]) acc += k19[t] * s[3 * t];
            s_h[i] = (uint16_t)acc;
        }
    }
    if (GRAIN) {
        for (int i = tid; i < PT_GH * PT_TW; i += PT_NT) {
            const uint8_t* g = &s_g[(i / PT_TW) * PT_GW + (i % PT_TW)];
            s_gh[i] = (uint16_t)(g[0] + 4 * g[1] + 6 * g[2] + 4 * g[3] + g[4]);
        }
    }
    __syncthreads();
    // 3. along columns, and the pixel steps: eight pixels down one column
    const int tx = tid & 63, wv = tid >> 6, x = x0 + tx;
    if (x >= W) return;
#pragma unroll 2
    for (int j = 0; j < PT_ROWS; ++j) {
        const int ty = wv * PT_ROWS + j, y = y0 + ty;
        if (y >= H) break;
        const size_t pix = (size_t)y * W + x;
        uint32_t q;
        if (SHARPEN) {
            q = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const uint16_t* h = &s_h[ty * PT_HLD + tx * 3 + ch];
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t < PT_TAPS; ++t)
                    if (k19[t]) v += (uint32_t)k19[t] * h[t * PT_HLD];
                const uint32_t blur = (v + (1u << 15)) >> 16;
                q |= aw_byte(s_src[(ty + PT_R) * PT_SLD + (tx + PT_R) * 3 + ch], c.w_src, blur, c.w_blur) << (8 * ch);
            }
        } else {
            const uint8_t* p = in + pix * 3;
            q = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        }
        if (COLOUR) q = saturate_px(q, s_div, c.boost, c.hue_scale);
        if (DETAIL) {
            const uint32_t lab = bgr_to_lab_px(q, s_lab, kf, cbrt_tab);
            q = lab_to_bgr_px((lab & 0xffff00u) | clahe_px(luts, geo, x, y, lab & 255u), s_lab, ki);
        }
        if (GRAIN) {
            const uint16_t* gh = &s_gh[ty * PT_TW + tx];
            const int blur = (gh[0] + 4 * gh[PT_TW] + 6 * gh[2 * PT_TW] + 4 * gh[3 * PT_TW] + gh[4 * PT_TW] + 128) >> 8;
            const uint32_t grain = (uint32_t)max((int)s_g[(ty + 2) * PT_GW + tx + 2] - blur, 0);      // cv2.subtract saturates
            q = aw_byte(q & 255u, 1.0f, grain, c.amount) | aw_byte((q >> 8) & 255u, 1.0f, grain, c.amount) << 8 |
                aw_byte(q >> 16, 1.0f, grain, c.amount) << 16;
        }
        uint8_t* o = out + pix * 3;
        o[0] = (uint8_t)q, o[1] = (uint8_t)(q >> 8), o[2] = (uint8_t)(q >> 16);
    }
}

// the tile-row histograms of a byte plane (BGR false) or of the Lab L of a BGR frame (BGR true); grid (row chunks, 8 tile rows)
template <bool BGR>
__global__ __launch_bounds__(CL_NT) void ptune_hist_kernel(const uint8_t* __restrict__ src, ClaheGeo G, int rows_per_block, LabFwd kf,
                                                           const int* __restrict__ cbrt_tab, const int* __restrict__ small_g,
                                                           uint32_t* __restrict__ hist_g) {
    __shared__ uint32_t s_hist[CL_GRID * 256];
    __shared__ uint16_t s_dec[256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < CL_GRID; ++k) s_hist[k * 256 + tid] = 0;
    if (BGR) s_dec[tid] = (uint16_t)small_g[tid];
    __syncthreads();
    clahe_count_rows(s_hist, G, rows_per_block, hist_g, [&](long p) -> uint32_t {
        if (!BGR) return src[p];
        const uint8_t* px = src + 3 * p;
        return l_of_px((uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16, s_dec, kf, cbrt_tab);
    });
}

__global__ __launch_bounds__(PT_NT) void ptune_clahe_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, ClaheGeo G,
                                                                  const uint8_t* __restrict__ luts) {
    const long npx = (long)G.H * G.W;
    for (long p = (long)blockIdx.x * PT_NT + threadIdx.x; p < npx; p += (long)gridDim.x * PT_NT) {
        const int y = (int)(p / G.W), x = (int)(p - (long)y * G.W);
        dst[p] = (uint8_t)clahe_px(luts, G, x, y, src[p]);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
int check_sides(const char* fn, int H, int W, bool detail) {
    if (H > MAX_FRAME_SIDE || W > MAX_FRAME_SIDE || H < PT_MIN_SIDE || W < PT_MIN_SIDE)
        return invalid(fn, "3 .. 16384 pixels a side expected (the 5 x 5 blur reflects two pixels)");
    if (detail && (H < CL_MIN_SIDE || W < CL_MIN_SIDE)) return invalid(fn, "8 .. 16384 pixels a side expected with detail recovery (8 x 8 CLAHE tiles)");
    return FW_OK;
}

int check_disjoint(const char* fn, const void* dst, std::initializer_list<const void*> srcs, size_t bytes) {
    FrameMarks marks = {{(uintptr_t)dst, 0}};
    for (const void* s : srcs) marks.push_back({(uintptr_t)s, 1});
    if (frames_overlap(marks, bytes)) return invalid(fn, "dst overlaps a source frame (every output reads a neighbourhood)");
    return FW_OK;
}

size_t round_up(size_t v) { return (v + PT_ALIGN - 1) / PT_ALIGN * PT_ALIGN; }

struct Layout {
    size_t hist, luts, buf_a, buf_n, nlm, total;
};

Layout layout(int H, int W) {
    Layout l;
    const size_t frame = round_up((size_t)H * W * 3);
    l.hist = 0;
    l.luts = l.hist + CL_HIST * sizeof(uint32_t);
    l.buf_a = round_up(l.luts + CL_HIST);
    l.buf_n = l.buf_a + frame;
    l.nlm = l.buf_n + frame;
    l.total = l.nlm + round_up(fw_nlmeans_scratch_bytes(H, W, 21));
    return l;
}

void launch_step(unsigned mask, const uint8_t* in, const uint8_t* orig, uint8_t* out, int H, int W, const Consts& c, const ClaheGeo& geo,
                 const uint8_t* luts, const int32_t* div, hipStream_t st) {
    const dim3 grid((unsigned)((W + PT_TW - 1) / PT_TW), (unsigned)((H + PT_TH - 1) / PT_TH));
    const bool detail = (mask & 4u) != 0;
    const LabTables* t = detail ? &lab_tables() : nullptr;
    const DeviceLab lab = detail ? device_lab() : DeviceLab{};
    const int* small = detail ? device_gamma_small() : nullptr;
    const LabFwd kf = detail ? t->fwd : LabFwd{};
    const LabInv ki = detail ? t->inv : LabInv{};
#define FW_PT_LAUNCH(S, C, D, G)                                                                                                            \
    hipLaunchKernelGGL((ptune_kernel<S, C, D, G>), grid, dim3(PT_NT), 0, st, in, orig, out, H, W, c, geo, luts, (const int*)div, kf, ki, \
                       (const int*)lab.cbrt_tab, (const int*)lab.t256, small)
    // bit 0 sharpen, 1 colour, 2 detail, 3 grain.  Detail comes alone or with grain: its maps are of the frame BEHIND sharpen and colour,
    // which no single launch can know, so 5, 6, 7, 13, 14, 15 have no kernel (fw_ptune_apply_u8 runs those steps as pass A first).
    switch (mask) {
        case 1: FW_PT_LAUNCH(true, false, false, false); break;
        case 2: FW_PT_LAUNCH(false, true, false, false); break;
        case 3: FW_PT_LAUNCH(true, true, false, false); break;
        case 4: FW_PT_LAUNCH(false, false, true, false); break;
        case 8: FW_PT_LAUNCH(false, false, false, true); break;
        case 9: FW_PT_LAUNCH(true, false, false, true); break;
        case 10: FW_PT_LAUNCH(false, true, false, true); break;
        case 11: FW_PT_LAUNCH(true, true, false, true); break;
        case 12: FW_PT_LAUNCH(false, false, true, true); break;
        default: throw Error(FW_ERR_INTERNAL, "perceptual: no kernel for this set of steps");
    }
#undef FW_PT_LAUNCH
    FW_HIP_CHECK(hipGetLastError());
}

// the 64 tile maps of `src` (a byte plane, or the Lab L of a BGR frame) into scratch: hist at 0, the maps behind it
const uint8_t* launch_luts(const uint8_t* src, bool bgr, const ClaheGeo& G, void* scratch, hipStream_t st) {
    uint32_t* hist = static_cast<uint32_t*>(scratch);
    uint8_t* luts = reinterpret_cast<uint8_t*>(hist + CL_HIST);
    FW_HIP_CHECK(hipMemsetAsync(hist, 0, CL_HIST * sizeof(uint32_t), st));
    const int rows = clahe_hist_rows_per_block(G);
    const dim3 grid(clahe_hist_chunks(G), CL_GRID);
    if (bgr) {
        const LabTables& t = lab_tables();
        const DeviceLab lab = device_lab();
        hipLaunchKernelGGL((ptune_hist_kernel<true>), grid, dim3(CL_NT), 0, st, src, G, rows, t.fwd, (const int*)lab.cbrt_tab,
                           (const int*)device_gamma_small(), hist);
    } else {
        hipLaunchKernelGGL((ptune_hist_kernel<false>), grid, dim3(CL_NT), 0, st, src, G, rows, LabFwd{}, (const int*)nullptr, (const int*)nullptr, hist);
    }
    FW_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(clahe_lut_kernel, dim3(CL_GRID * CL_GRID, 1), dim3(CL_NT), 0, st, (const uint32_t*)hist, luts, G.limit, G.lut_scale);
    FW_HIP_CHECK(hipGetLastError());
    return luts;
}

int check_scratch(const char* fn, const void* scratch) {
    if (!scratch || ((uintptr_t)scratch & 3)) return invalid(fn, "a 4-byte aligned scratch of fw_ptune_scratch_bytes(height, width, params) expected");
    return FW_OK;
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_ptune_gauss19_table(int32_t* out19) {
    if (!out19) return invalid("fw_ptune_gauss19_table", "null pointer");
    constexpr int k19[PT_TAPS] = {PT_K19_VALUES};
    for (int i = 0; i < PT_TAPS; ++i) out19[i] = k19[i];
    return FW_OK;
}

size_t fw_ptune_scratch_bytes(int height, int width, const fw_ptune_params* params) {
    if (height < PT_MIN_SIDE || height > MAX_FRAME_SIDE || width < PT_MIN_SIDE || width > MAX_FRAME_SIDE) return 0;
    const Layout L = layout(height, width);
    if (!params) return L.buf_a;                                      // fw_ptune_clahe_u8, fw_ptune_detail_u8: the histograms and the maps
    if (params->denoise_h > 0) return L.total;                        // the denoised frame and the non-local means' own planes lie last
    if (!params->detail) return 0;
    return (params->sharpen || params->colour) ? L.buf_n : L.buf_a;   // pass A's bytes behind the histograms and the maps
}

int fw_ptune_unsharp_u8(const uint8_t* src, uint8_t* dst, int height, int width, float w_src, float w_blur, void* stream) {
    const char* fn = "fw_ptune_unsharp_u8";
    if (!src || !dst) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, false)) return st;
    if (!std::isfinite(w_src) || !std::isfinite(w_blur)) return invalid(fn, "finite weights expected");
    if (const int st = check_disjoint(fn, dst, {src}, (size_t)height * width * 3)) return st;
    return guarded([&] { launch_step(1, src, src, dst, height, width, Consts{w_src, w_blur, 0, 0, 0}, ClaheGeo{}, nullptr, nullptr, (hipStream_t)stream); });
}

int fw_ptune_grain_u8(const uint8_t* result, const uint8_t* original, uint8_t* dst, int height, int width, float amount, void* stream) {
    const char* fn = "fw_ptune_grain_u8";
    if (!result || !original || !dst) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, false)) return st;
    if (!std::isfinite(amount)) return invalid(fn, "a finite grain amount expected");
    if (const int st = check_disjoint(fn, dst, {result, original}, (size_t)height * width * 3)) return st;
    return guarded([&] { launch_step(8, result, original, dst, height, width, Consts{0, 0, 0, 0, amount}, ClaheGeo{}, nullptr, nullptr, (hipStream_t)stream); });
}

int fw_ptune_clahe_u8(const uint8_t* plane, uint8_t* dst, int height, int width, int limit, void* scratch, void* stream) {
    const char* fn = "fw_ptune_clahe_u8";
    if (!plane || !dst) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, true)) return st;
    if (limit < 1) return invalid(fn, "a clip limit of at least 1 count expected");
    if (const int st = check_scratch(fn, scratch)) return st;
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const ClaheGeo G = clahe_geometry(height, width, limit);
        const uint8_t* luts = launch_luts(plane, false, G, scratch, st);
        const long blocks = std::min<long>(((long)height * width + PT_NT - 1) / PT_NT, PT_BLOCKS);
        hipLaunchKernelGGL(ptune_clahe_apply_kernel, dim3((unsigned)blocks), dim3(PT_NT), 0, st, plane, dst, G, luts);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_ptune_detail_u8(const uint8_t* src, uint8_t* dst, int height, int width, int limit, void* scratch, void* stream) {
    const char* fn = "fw_ptune_detail_u8";
    if (!src || !dst) return invalid(fn, "null pointer");
    if (const int st = check_sides(fn, height, width, true)) return st;
    if (limit < 1) return invalid(fn, "a clip limit of at least 1 count expected");
    if (const int st = check_scratch(fn, scratch)) return st;
    if (const int st = check_disjoint(fn, dst, {src}, (size_t)height * width * 3)) return st;
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const ClaheGeo G = clahe_geometry(height, width, limit);
        const uint8_t* luts = launch_luts(src, true, G, scratch, st);
        launch_step(4, src, src, dst, height, width, Consts{}, G, luts, nullptr, st);
    });
}

int fw_ptune_apply_u8(const uint8_t* src, uint8_t* dst, int height, int width, const fw_ptune_params* params, void* scratch, void* stream) {
    const char* fn = "fw_ptune_apply_u8";
    if (!src || !dst || !params) return invalid(fn, "null pointer");
    const fw_ptune_params& P = *params;
    const bool sharpen = P.sharpen != 0, colour = P.colour != 0, detail = P.detail != 0, grain = P.grain != 0, denoise = P.denoise_h > 0;
    if (const int st = check_sides(fn, height, width, detail)) return st;
    if (P.denoise_h < 0 || P.denoise_h > 100) return invalid(fn, "a denoise h of 0 (off) .. 100 expected");
    if ((sharpen && (!std::isfinite(P.w_src) || !std::isfinite(P.w_blur))) || (colour && !std::isfinite(P.boost)) || (grain && !std::isfinite(P.grain_amount)))
        return invalid(fn, "finite weights expected");
    if (colour && !P.hsv_div) return invalid(fn, "null pointer");
    if (detail && P.clahe_limit < 1) return invalid(fn, "a clip limit of at least 1 count expected");
    if (denoise || detail)
        if (const int st = check_scratch(fn, scratch)) return st;
    const size_t bytes = (size_t)height * width * 3;
    if (const int st = check_disjoint(fn, dst, {src}, bytes)) return st;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = layout(height, width);
    uint8_t* base = static_cast<uint8_t*>(scratch);
    const unsigned front = (sharpen ? 1u : 0u) | (colour ? 2u : 0u), tail = grain ? 8u : 0u;
    const uint8_t* cur = src;
    if (denoise) {
        uint8_t* to = (front || detail || tail) ? base + L.buf_n : dst;
        if (const int e = fw_nlmeans_colored_u8(cur, height, width, (double)P.denoise_h, (double)P.denoise_h, 7, 21, base + L.nlm, to, stream)) return e;
        cur = to;
    }
    return guarded([&] {
        const Consts c{P.w_src, P.w_blur, P.boost, P.hue_scale, P.grain_amount};
        if (!detail) {
            if (front | tail) launch_step(front | tail, cur, src, dst, height, width, c, ClaheGeo{}, nullptr, P.hsv_div, st);
            else if (cur == src) FW_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
            return;
        }
        if (front) {
            launch_step(front, cur, src, base + L.buf_a, height, width, c, ClaheGeo{}, nullptr, P.hsv_div, st);
            cur = base + L.buf_a;
        }
        const ClaheGeo G = clahe_geometry(height, width, P.clahe_limit);
        const uint8_t* luts = launch_luts(cur, true, G, scratch, st);
        launch_step(4u | tail, cur, src, dst, height, width, c, G, luts, nullptr, st);
    });
}

}  // extern "C"
