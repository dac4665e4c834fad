// cv2's CLAHE on a byte plane with an 8 x 8 tile grid, as tests/hdr_ref.py states it (clahe_geometry, clahe_luts, clahe_interpolate),
// shared by hdr.hip (local contrast, clip limit 2.0, blended half and half) and perceptual.hip (detail recovery, the clip limit of the
// profile, L replaced): the geometry of a frame, the tile-row histogram loop, the clip / redistribute / cumulate kernel and the
// bilinear interpolation between the four nearest tile maps.  The integer `limit` of a tile is the caller's: max(int(clip * area /
// 256), 1) in double.  The float arithmetic here is the interpolation's (products and sums rounded one by one): the including file is
// compiled with contraction off.  Every including file gets its own copy of the kernel.
#pragma once
#include "stage_common.h"

#pragma clang fp contract(off)

namespace fw {
namespace {

constexpr int CL_GRID = 8;                                       // CLAHE tiles a side
constexpr int CL_HIST = CL_GRID * CL_GRID * 256;                 // bins a frame
constexpr int CL_NT = 256;                                       // threads of the histogram and of the LUT kernel
constexpr int CL_MIN_SIDE = 8;

struct ClaheGeo {
    int H, W, Hp, Wp, th, tw, limit;
    float inv_th, inv_tw, lut_scale;
};

inline int clahe_tile_area(int H, int W) {
    const bool whole = H % CL_GRID == 0 && W % CL_GRID == 0;
    const int Hp = whole ? H : H + CL_GRID - H % CL_GRID, Wp = whole ? W : W + CL_GRID - W % CL_GRID;
    return (Hp / CL_GRID) * (Wp / CL_GRID);
}

inline int clahe_limit(double clip_limit, int H, int W) { return std::max((int)(clip_limit * clahe_tile_area(H, W) / 256), 1); }

inline ClaheGeo clahe_geometry(int H, int W, int limit) {
    ClaheGeo g;
    g.H = H, g.W = W;
    const bool whole = H % CL_GRID == 0 && W % CL_GRID == 0;
    g.Hp = whole ? H : H + CL_GRID - H % CL_GRID;
    g.Wp = whole ? W : W + CL_GRID - W % CL_GRID;
    g.th = g.Hp / CL_GRID, g.tw = g.Wp / CL_GRID;
    const int area = g.th * g.tw;
    g.limit = limit;
    g.inv_th = (float)(1.0 / g.th), g.inv_tw = (float)(1.0 / g.tw);
    g.lut_scale = (float)(255.0 / area);
    return g;
}

// rows of one tile row a workgroup of the histogram kernel takes; grid (clahe_hist_chunks, 8 tile rows, frames)
inline int clahe_hist_rows_per_block(const ClaheGeo& G) { return std::max(1, 16384 / G.Wp); }
inline unsigned clahe_hist_chunks(const ClaheGeo& G) {
    const int rows = clahe_hist_rows_per_block(G);
    return (unsigned)((G.th + rows - 1) / rows);
}

// The body of a histogram kernel: the workgroup (CL_NT threads; blockIdx.x the row chunk, blockIdx.y the tile row) counts its rows
// of the frame as padded by reflect-101 into s_hist[8 * 256], which the caller has zeroed and synchronised, then adds every bin
// that is not zero to `hist_frame` (the frame's 64 x 256 counts).  l_of(p): the byte at pixel index p of the frame.
template <typename LOf>
__device__ __forceinline__ void clahe_count_rows(uint32_t* s_hist, const ClaheGeo& G, int rows_per_block, uint32_t* __restrict__ hist_frame, LOf l_of) {
    const int tid = threadIdx.x, ty = blockIdx.y;
    const int r0 = ty * G.th + blockIdx.x * rows_per_block;
    const int r1 = min(r0 + rows_per_block, (ty + 1) * G.th);
    const long count = (long)max(r1 - r0, 0) * G.Wp;
    for (long i = tid; i < count; i += CL_NT) {
        const int yp = r0 + (int)(i / G.Wp), xp = (int)(i % G.Wp);
        const long p = (long)reflect101(yp, G.H) * G.W + reflect101(xp, G.W);          // the padding is the frame mirrored
        atomicAdd(&s_hist[(xp / G.tw) * 256 + l_of(p)], 1u);
    }
    __syncthreads();
    uint32_t* out = hist_frame + (size_t)ty * CL_GRID * 256;
#pragma unroll
    for (int k = 0; k < CL_GRID; ++k) {
        const uint32_t v = s_hist[k * 256 + tid];
        if (v) atomicAdd(&out[k * 256 + tid], v);
    }
}

// one workgroup per tile: grid (64, n).  lane i holds bin i
__global__ __launch_bounds__(CL_NT) void clahe_lut_kernel(const uint32_t* __restrict__ hist_g, uint8_t* __restrict__ luts, int limit, float lut_scale) {
    __shared__ int s_scan[256];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x;
    const size_t base = ((size_t)blockIdx.y * CL_GRID * CL_GRID + blockIdx.x) * 256;
    int h = (int)hist_g[base + tid];
    const int over = wave_sum(max(h - limit, 0));
    if ((tid & 63) == 0) s_wave[tid >> 6] = over;
    __syncthreads();
    const int excess = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    h = min(h, limit) + excess / 256;
    const int residual = excess % 256;
    if (residual) {
        const int step = max(256 / residual, 1);
        if (tid % step == 0 && tid / step < residual) ++h;
    }
    s_scan[tid] = h;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                              // inclusive scan: integers, any order gives the same sums
        const int add = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const int v = __float2int_rn((float)s_scan[tid] * lut_scale);
    luts[base + tid] = (uint8_t)min(max(v, 0), 255);
}

// cv2's CLAHE interpolation of value v at (x, y) between the four nearest tile LUTs of frame `luts`
__device__ __forceinline__ uint32_t clahe_px(const uint8_t* __restrict__ luts, const ClaheGeo& G, int x, int y, uint32_t v) {
    const float txf = (float)x * G.inv_tw - 0.5f, tyf = (float)y * G.inv_th - 0.5f;
    const float fx = floorf(txf), fy = floorf(tyf);
    const float xa = txf - fx, ya = tyf - fy;
    const int tx1 = min(max((int)fx, 0), CL_GRID - 1), tx2 = min(max((int)fx + 1, 0), CL_GRID - 1);
    const int ty1 = min(max((int)fy, 0), CL_GRID - 1), ty2 = min(max((int)fy + 1, 0), CL_GRID - 1);
    const float xb = 1.0f - xa, yb = 1.0f - ya;
    const float l11 = luts[(ty1 * CL_GRID + tx1) * 256 + v], l12 = luts[(ty1 * CL_GRID + tx2) * 256 + v];
    const float l21 = luts[(ty2 * CL_GRID + tx1) * 256 + v], l22 = luts[(ty2 * CL_GRID + tx2) * 256 + v];
    const float top = l11 * xb + l12 * xa, bottom = l21 * xb + l22 * xa;
    const float res = top * yb + bottom * ya;
    return (uint32_t)min(max(__float2int_rn(res), 0), 255);
}

}  // namespace
}  // namespace fw
