// The reference's colour grade (src/framewright/integration/lut.py: `LUTManager.apply_to_image_fast`, step 7c of core/restorer.py) on
// uint8 / uint16 three-channel frames that are already in HBM.  The reference is a fixed sequence of NumPy operations, each rounded
// on its own, so the contract (tests/color_lut_ref.py, held byte for byte against the reference's own function on the CPU) is byte
// equality:
//
//   fw_lut3d_apply_u8 / _u16   n frames through a size^3 table of float32 RGB triples, order [r][g][b][rgb], trilinear
//   fw_table3_apply_u8         n frames through three 256-byte tables, one per stored channel (a 1D LUT on 8-bit input)
//
// Arithmetic per sample v of a pixel (maxv = 255 or 65535).  In float32: x = v / maxv (IEEE division), s = x * (size - 1),
// lo = floor(s), hi = min(lo + 1, size - 1).  From here on FLOAT64, because NumPy's `scaled - indices_low` subtracts an int32 array
// from a float32 one and that promotes to float64: f = s - lo (exact), the eight float32 corners widened; four lerps along r, two
// along g, one along b, each a * (1 - f) + b * f as two products and a sum (this file is compiled with -ffp-contract=off); clip to
// [0, 1], * maxv, truncate.  The same lerps in float32 change about one 8-bit colour in 65 000 under the autumn table and one
// 16-bit pixel in 200; a reciprocal instead of the division changes s for half the byte values.  The domain fields of a LUT play
// no part, as in `apply_to_image_fast`.
//
// A frame is H W pixels without row padding and may start at any byte (a batch of 3 x 5 frames has its second frame on byte 45): a
// lane takes four pixels, reads the aligned 32-bit words that cover their 12 (uint8) or 24 (uint16) bytes - only words and bytes
// inside the frame are touched - and writes them back as words when the destination is aligned and the four pixels are whole, else
// sample by sample.  In place (dst == src, equal strides) is allowed: a lane writes exactly the samples it has read.
// The table: up to 17^3 (59 KiB) it is copied into LDS by every workgroup, two workgroups per CU; larger tables (the default 33^3 is
// 431 KiB, 65^3 3.3 MB) are read through L2.  Either way the b and b + 1 corners of one (r, g) are six consecutive floats and come
// as one load (at the last plane, where hi == lo, the pair one step back is loaded and its upper entry serves as both).
// The 8-bit s values are a 256-entry table in LDS, one division per entry and workgroup; 16-bit samples are divided as they come.
// No atomics, no scratch; a frame's result depends on its bytes and the table alone, not on the run, the batch or its address.
#include "stage_common.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace fw {
namespace {

constexpr int CL_NT = 256;
constexpr int CL_MIN_SIZE = 2, CL_MAX_SIZE = 65;
constexpr int CL_LDS_MAX_SIZE = 17;                                   // 17^3 * 12 B = 58956 B of dynamic LDS
constexpr int CL_MAX_SIDE = 16384;
constexpr int CL_BLOCKS_LDS = 512, CL_BLOCKS = 2048;                  // workgroups of one launch, all frames together, about

struct __attribute__((packed, aligned(4))) Corner2 {                  // table[r][g][b] and table[r][g][b + 1]
    float v[6];
};

// Four pixels per lane and turn: op(v, o) maps the 12 samples v (stored order) of pixels 4 g .. 4 g + 3 to the 12 samples o.
// Samples behind the frame's last pixel read as 0 and are not written.
template <typename T, typename Op>
__device__ __forceinline__ void for_pixel_groups(const uint8_t* fs, uint8_t* fd, long npix, Op op) {
    constexpr int B = sizeof(T), NW = 3 * B, GB = 12 * B;
    const uint8_t* fs_end = fs + (size_t)npix * 3 * B;
    const uint32_t soff = (uint32_t)((uintptr_t)fs & 3), doff = (uint32_t)((uintptr_t)fd & 3);
    const long groups = (npix + 3) >> 2;
    for (long g = (long)blockIdx.x * CL_NT + threadIdx.x; g < groups; g += (long)gridDim.x * CL_NT) {
        const uint8_t* p = fs + g * GB - soff;
        uint32_t w[NW + 1];
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = load_word_inside(p + 4 * k, fs, fs_end);
        w[NW] = soff ? load_word_inside(p + 4 * NW, fs, fs_end) : 0u;
        uint32_t v[12], o[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int k = i * B / 4;
            const uint32_t d = __builtin_amdgcn_alignbyte(w[k + 1], w[k], soff);
            v[i] = B == 1 ? (d >> (8 * (i & 3))) & 255u : (d >> (16 * (i & 1))) & 65535u;
        }
        op(v, o);
        const long left = npix - 4 * g;
        uint8_t* q = fd + g * GB;
        if (doff == 0 && left >= 4) {
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                const uint32_t word = B == 1 ? o[4 * k] | (o[4 * k + 1] << 8) | (o[4 * k + 2] << 16) | (o[4 * k + 3] << 24)
                                             : o[2 * k] | (o[2 * k + 1] << 16);
                reinterpret_cast<uint32_t*>(q)[k] = word;
            }
        } else {
            const int ns = left >= 4 ? 12 : 3 * (int)left;
#pragma unroll
            for (int i = 0; i < 12; ++i)
                if (i < ns) reinterpret_cast<T*>(q)[i] = (T)o[i];
        }
    }
}

__device__ __forceinline__ double lerp_np(double a, double b, double f, double omf) {
    const double x = a * omf;
    const double y = b * f;
    return x + y;                                                     // two products and a sum, each rounded (no contraction)
}

template <typename T, bool LDS_TABLE>
__global__ __launch_bounds__(CL_NT) void lut3d_kernel(const uint8_t* src, long src_stride, long npix, const float* __restrict__ lut,
                                                      int size, int bgr, uint8_t* dst, long dst_stride) {
    extern __shared__ float s_lut[];                                  // LDS_TABLE: size^3 x 3 floats
    __shared__ float s_scale[256];                                    // uint8: s of every byte value
    constexpr float maxv = sizeof(T) == 1 ? 255.0f : 65535.0f;
    const int tid = threadIdx.x;
    const float smax = (float)(size - 1);
    if (sizeof(T) == 1) s_scale[tid] = __fdiv_rn((float)tid, maxv) * smax;
    if (LDS_TABLE) {
        const int nfl = size * size * size * 3;
        for (int i = tid; i < nfl; i += CL_NT) s_lut[i] = lut[i];
    }
    __syncthreads();
    const int last = size - 1;

    auto grade = [&](uint32_t vr, uint32_t vg, uint32_t vb, uint32_t& o_r, uint32_t& o_g, uint32_t& o_b) {
        float s[3];
        double f[3], omf[3];
        int lo[3];
        const uint32_t vv[3] = {vr, vg, vb};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[c] = sizeof(T) == 1 ? s_scale[vv[c]] : __fdiv_rn((float)vv[c], maxv) * smax;
            lo[c] = min((int)s[c], last);                             // s >= 0: the cast is the floor; s <= size - 1 already
            f[c] = (double)s[c] - (double)lo[c];
            omf[c] = 1.0 - f[c];
        }
        const int r0 = lo[0], g0 = lo[1], b0 = lo[2];
        const int r1 = min(r0 + 1, last), g1 = min(g0 + 1, last);
        const bool top = b0 == last;                                  // hi == lo: both b corners are the table's last plane
        const int bb = b0 - (top ? 1 : 0);                            // size >= 2: never negative, bb + 1 <= size - 1
        float c0[4][3], c1[4][3];                                     // [r g corner: 00, 01 (g1), 10 (r1), 11][rgb] at b0 and b1
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = k & 2 ? r1 : r0, g = k & 1 ? g1 : g0;
            const int e = ((r * size + g) * size + bb) * 3;
            Corner2 pr;
            if (LDS_TABLE) pr = *reinterpret_cast<const Corner2*>(s_lut + e);
            else pr = *reinterpret_cast<const Corner2*>(lut + e);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                c0[k][c] = top ? pr.v[3 + c] : pr.v[c];
                c1[k][c] = pr.v[3 + c];
            }
        }
        uint32_t out[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double c00 = lerp_np(c0[0][c], c0[2][c], f[0], omf[0]);    // c000, c100
            const double c01 = lerp_np(c1[0][c], c1[2][c], f[0], omf[0]);    // c001, c101
            const double c10 = lerp_np(c0[1][c], c0[3][c], f[0], omf[0]);    // c010, c110
            const double c11 = lerp_np(c1[1][c], c1[3][c], f[0], omf[0]);    // c011, c111
            const double d0 = lerp_np(c00, c10, f[1], omf[1]);
            const double d1 = lerp_np(c01, c11, f[1], omf[1]);
            const double res = lerp_np(d0, d1, f[2], omf[2]);
            out[c] = (uint32_t)(fmin(fmax(res, 0.0), 1.0) * (double)maxv);
        }
        o_r = out[0];
        o_g = out[1];
        o_b = out[2];
    };

    const uint8_t* fs = src + (size_t)blockIdx.y * src_stride;
    uint8_t* fd = dst + (size_t)blockIdx.y * dst_stride;
    for_pixel_groups<T>(fs, fd, npix, [&](const uint32_t* v, uint32_t* o) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t o_r, o_g, o_b;
            grade(bgr ? v[3 * j + 2] : v[3 * j], v[3 * j + 1], bgr ? v[3 * j] : v[3 * j + 2], o_r, o_g, o_b);
            o[3 * j] = bgr ? o_b : o_r;
            o[3 * j + 1] = o_g;
            o[3 * j + 2] = bgr ? o_r : o_b;
        }
    });
}

__global__ __launch_bounds__(CL_NT) void table3_kernel(const uint8_t* src, long src_stride, long npix, const uint8_t* __restrict__ tables,
                                                       uint8_t* dst, long dst_stride) {
    __shared__ uint8_t s_tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += CL_NT) s_tab[i] = tables[i];
    __syncthreads();
    const uint8_t* fs = src + (size_t)blockIdx.y * src_stride;
    uint8_t* fd = dst + (size_t)blockIdx.y * dst_stride;
    for_pixel_groups<uint8_t>(fs, fd, npix, [&](const uint32_t* v, uint32_t* o) {
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = s_tab[(i % 3) * 256 + v[i]];
    });
}

// 0 when the frame arguments are usable, else the status of the refusal (message set)
int cl_check_frames(const char* fn, const void* src, int64_t src_stride, int n, int H, int W, const void* dst, int64_t dst_stride, int bytes) {
    if (!src || !dst) return invalid(fn, "null pointer");
    if (n < 1 || n > 65535 || H < 1 || W < 1 || H > CL_MAX_SIDE || W > CL_MAX_SIDE)
        return invalid(fn, "1 .. 65535 frames of 1 .. 16384 pixels a side expected");
    if (src_stride < 0 || dst_stride < 0 || (n > 1 && (src_stride == 0 || dst_stride == 0))) return invalid(fn, "bad frame stride");
    if (bytes == 2 && (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)src_stride | (uintptr_t)dst_stride) & 1))
        return invalid(fn, "16-bit frames start on even addresses");
    return FW_OK;
}

dim3 cl_grid(long npix, int n, int cap) {
    const long per_frame = std::max(1L, (long)cap / n);
    const long blocks = std::min(per_frame, ((npix + 3) / 4 + CL_NT - 1) / CL_NT);
    return dim3((unsigned)std::max(1L, blocks), (unsigned)n);
}

template <typename T>
int lut3d_apply(const char* fn, const void* src, int64_t src_stride, int n, int H, int W, const float* lut, int size, int bgr, void* dst,
                int64_t dst_stride, void* stream) {
    if (const int st = cl_check_frames(fn, src, src_stride, n, H, W, dst, dst_stride, (int)sizeof(T))) return st;
    if (!lut) return invalid(fn, "null pointer");
    if (size < CL_MIN_SIZE || size > CL_MAX_SIZE) return invalid(fn, "a table size of 2 .. 65 expected");
    const long npix = (long)H * W;
    const long ss = n > 1 ? (long)src_stride : 0, ds = n > 1 ? (long)dst_stride : 0;
    hipStream_t st = (hipStream_t)stream;
    if (size <= CL_LDS_MAX_SIZE) {
        const size_t lds = (size_t)size * size * size * 3 * sizeof(float);
        hipLaunchKernelGGL((lut3d_kernel<T, true>), cl_grid(npix, n, CL_BLOCKS_LDS), dim3(CL_NT), lds, st, (const uint8_t*)src, ss, npix, lut,
                           size, bgr ? 1 : 0, (uint8_t*)dst, ds);
    } else {
        hipLaunchKernelGGL((lut3d_kernel<T, false>), cl_grid(npix, n, CL_BLOCKS), dim3(CL_NT), 0, st, (const uint8_t*)src, ss, npix, lut, size,
                           bgr ? 1 : 0, (uint8_t*)dst, ds);
    }
    return hip_status(fn, hipGetLastError());
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_lut3d_apply_u8(const uint8_t* src, int64_t src_stride_bytes, int n, int height, int width, const float* lut_f32, int size, int bgr,
                      uint8_t* dst, int64_t dst_stride_bytes, void* stream) {
    return lut3d_apply<uint8_t>("fw_lut3d_apply_u8", src, src_stride_bytes, n, height, width, lut_f32, size, bgr, dst, dst_stride_bytes, stream);
}

int fw_lut3d_apply_u16(const uint16_t* src, int64_t src_stride_bytes, int n, int height, int width, const float* lut_f32, int size, int bgr,
                       uint16_t* dst, int64_t dst_stride_bytes, void* stream) {
    return lut3d_apply<uint16_t>("fw_lut3d_apply_u16", src, src_stride_bytes, n, height, width, lut_f32, size, bgr, dst, dst_stride_bytes, stream);
}

int fw_table3_apply_u8(const uint8_t* src, int64_t src_stride_bytes, int n, int height, int width, const uint8_t* tables, uint8_t* dst,
                       int64_t dst_stride_bytes, void* stream) {
    const char* fn = "fw_table3_apply_u8";
    if (const int st = cl_check_frames(fn, src, src_stride_bytes, n, height, width, dst, dst_stride_bytes, 1)) return st;
    if (!tables) return invalid(fn, "null pointer");
    const long npix = (long)height * width;
    const long ss = n > 1 ? (long)src_stride_bytes : 0, ds = n > 1 ? (long)dst_stride_bytes : 0;
    hipLaunchKernelGGL(table3_kernel, cl_grid(npix, n, CL_BLOCKS), dim3(CL_NT), 0, (hipStream_t)stream, src, ss, npix, tables, dst, ds);
    return hip_status(fn, hipGetLastError());
}

}  // extern "C"
