// The frame path of the reference's aspect processor (src/framewright/processors/format/aspect.py: `analyze_frame` / `analyze` with
// `_detect_horizontal_bars` and `_detect_vertical_bars`, `crop_letterbox`, `convert_aspect` with `_crop_to_ratio`, `_pad_to_ratio`,
// `_apply_blur_fill` and `_apply_mirror_fill`) on uint8 frames that are already in HBM.  tests/aspect_ref.py is the contract, held byte
// for byte against the reference's own methods on the CPU.
//
// What runs here and what on the host.  The reference takes np.mean of every gray row and column until one exceeds the threshold; for
// uint8 values that is sum > threshold * length in integers.  The device forms every row sum and every column sum of the gray image
// in one pass over the frame, the host walks the few hundred sums (aspect.py), and the device crops or pads:
//   fw_aspect_bar_sums_u8   uint32 row sums [n][H] and column sums [n][W] of gray, exact: at most 255 * 16384
//   fw_aspect_crop_u8       frames[i][y : y + h, x : x + w] into contiguous destinations, as it is or with its columns or rows reversed
//                           (the reversal makes the strip of a mirror fill that has to be stretched)
//   fw_aspect_pad_u8        every byte of the output frame in one launch: the source at (x_offset, y_offset), outside it the fill
//                           colour, the mirror fill, or the bytes of a prepared background of the output size (the blur fill)
//   fw_aspect_gauss99_u8    cv2.GaussianBlur(src, (99, 99), 0) on uint8 in fixed point: rows into uint16, columns into uint8
//
// Mirror fill.  A bar no wider than the source is the source's edge strip reversed: out[x] = src[x_offset - 1 - x] on the left,
// src[W - 1 - j] for the j-th column of the right bar, the same for rows.  A bar wider than the source is the whole source reversed and
// stretched with cv2's linear resize: the caller forms that strip with fw_aspect_crop_u8 (reversed) and fw_resize_linear_u8 - the one
// copy of that arithmetic - and hands it in; the kernel takes its bytes.  The four strips span the source only, the corners keep the
// fill colour, as in the reference.
//
// Kernel shape.  Integers only, so every result is the same in every run and no floating-point flag matters.  All four are bound by
// one read and one write of the frame (the blur by its 99 taps, which hit the L1 / L2).  The statistics kernel gives a workgroup 256
// columns and a band of 32 rows: a lane keeps its column's sum in a register, a wave reduces its 64 gray values of a row with
// shuffles, and both go out as integer atomic adds - one per wave and row, one per lane and band - onto sums the entry has zeroed.
// Crop and pad take 16 bytes a lane when the frames, the rows and the offsets are 16-byte aligned (a letterbox of a 1080p or 8K
// frame is: its rows are whole and 5760 or 23040 bytes long), else one byte a lane, so frames may start at any byte.  Up to 32 frames
// share a launch; their pointers travel by value in the kernel arguments, so a batch needs no table in device memory and the entry
// checks every pointer.  Left out: 16-byte loads in the statistics (BGR pixels straddle them), an LDS tile for the blur.
#include "stage_common.h"

namespace fw {
namespace {

constexpr int AS_NT = 256;
constexpr int AS_BATCH = 32;
constexpr int AS_BAND = 32;                                           // rows of one workgroup of the statistics
constexpr int AS_BLOCKS = 4096;
constexpr int AS_TAPS = 99;

struct AsFrames {
    const uint8_t* p[AS_BATCH];
};

struct AsPairs {
    const uint8_t* src[AS_BATCH];
    uint8_t* dst[AS_BATCH];
};

struct AsPad {
    const uint8_t* src[AS_BATCH];
    uint8_t* dst[AS_BATCH];
    const uint8_t* back[AS_BATCH];                                    // mode 2: the background, of the output size
    const uint8_t* strip[AS_BATCH][4];                                // mode 1: left, right, top, bottom where the bar is wider than the source
    int H, W, OH, OW, x_off, y_off, mode;
    uint8_t color[4];
};

struct AsGauss {
    uint16_t k[AS_TAPS + 1];
};

// ---- statistics: row and column sums of gray --------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(AS_NT) void as_bar_sums_kernel(const AsFrames frames, int H, int W, uint32_t* row_sums, uint32_t* col_sums) {
    const int f = blockIdx.z;
    const uint8_t* img = frames.p[f];
    const int x = blockIdx.x * AS_NT + threadIdx.x;
    const int y0 = blockIdx.y * AS_BAND, y1 = min(H, y0 + AS_BAND);
    const bool in = x < W;
    uint32_t col = 0;                                                 // at most 255 * 32
    for (int y = y0; y < y1; ++y) {
        const uint32_t g = in ? (uint32_t)gray_bgr<C>(img + ((long)y * W + x) * C) : 0u;
        col += g;
        const uint32_t r = wave_sum(g);                               // at most 255 * 64
        if ((threadIdx.x & 63) == 0 && blockIdx.x * AS_NT + (int)(threadIdx.x & ~63u) < W) atomicAdd(row_sums + (long)f * H + y, r);
    }
    if (in) atomicAdd(col_sums + (long)f * W + x, col);
}

// ---- crop: dst[yy][xx] = src[y + yy][x + xx], flip 1: columns reversed, flip 2: rows reversed -------------------------------------------
template <int C>
__global__ __launch_bounds__(AS_NT) void as_crop_kernel(const AsPairs t, int W, int x0, int y0, int w, int h, int flip) {
    const uint8_t* src = t.src[blockIdx.y];
    uint8_t* dst = t.dst[blockIdx.y];
    const long total = (long)h * w * C;
    const int rb = w * C;
    for (long i = (long)blockIdx.x * AS_NT + threadIdx.x; i < total; i += (long)gridDim.x * AS_NT) {
        const int yy = (int)(i / rb), xb = (int)(i - (long)yy * rb);
        const int xx = xb / C, c = xb - xx * C;
        const int sy = y0 + (flip == 2 ? h - 1 - yy : yy), sx = x0 + (flip == 1 ? w - 1 - xx : xx);
        dst[i] = src[((long)sy * W + sx) * C + c];
    }
}

// 16 bytes a lane: the rows of both, the crop's first byte and every pointer are 16-byte aligned, nothing is reversed
__global__ __launch_bounds__(AS_NT) void as_crop16_kernel(const AsPairs t, long src_row_bytes, long first_byte, int row_chunks, int h) {
    const uint8_t* src = t.src[blockIdx.y] + first_byte;
    uint8_t* dst = t.dst[blockIdx.y];
    const long total = (long)h * row_chunks;
    for (long i = (long)blockIdx.x * AS_NT + threadIdx.x; i < total; i += (long)gridDim.x * AS_NT) {
        const int yy = (int)(i / row_chunks), ch = (int)(i - (long)yy * row_chunks);
        *reinterpret_cast<uint4*>(dst + i * 16) = *reinterpret_cast<const uint4*>(src + yy * src_row_bytes + ch * 16L);
    }
}

// ---- pad ----------------------------------------------------------------------------------------------------------------------------------
// the byte of output pixel (y, x), channel c, of frame f
template <int C>
__device__ __forceinline__ uint8_t as_pad_byte(const AsPad& p, int f, int y, int x, int c) {
    const int sy = y - p.y_off, sx = x - p.x_off;
    const bool in_rows = (unsigned)sy < (unsigned)p.H, in_cols = (unsigned)sx < (unsigned)p.W;
    const uint8_t* src = p.src[f];
    if (in_rows && in_cols) return src[((long)sy * p.W + sx) * C + c];
    if (p.mode == 2) return p.back[f][((long)y * p.OW + x) * C + c];
    if (p.mode == 1) {
        if (in_rows && sx < 0) {                                      // left bar, p.x_off columns
            if (p.x_off <= p.W) return src[((long)sy * p.W + (p.x_off - 1 - x)) * C + c];
            return p.strip[f][0][((long)sy * p.x_off + x) * C + c];
        }
        if (in_rows) {                                                // right bar
            const int bar = p.OW - p.x_off - p.W, j = sx - p.W;
            if (bar <= p.W) return src[((long)sy * p.W + (p.W - 1 - j)) * C + c];
            return p.strip[f][1][((long)sy * bar + j) * C + c];
        }
        if (in_cols && sy < 0) {                                      // top bar, p.y_off rows
            if (p.y_off <= p.H) return src[((long)(p.y_off - 1 - y) * p.W + sx) * C + c];
            return p.strip[f][2][((long)y * p.W + sx) * C + c];
        }
        if (in_cols) {                                                // bottom bar
            const int bar = p.OH - p.y_off - p.H, j = sy - p.H;
            if (bar <= p.H) return src[((long)(p.H - 1 - j) * p.W + sx) * C + c];
            return p.strip[f][3][((long)j * p.W + sx) * C + c];
        }
    }
    return p.color[c];
}

template <int C>
__global__ __launch_bounds__(AS_NT) void as_pad_kernel(const AsPad p) {
    const int f = blockIdx.y;
    uint8_t* dst = p.dst[f];
    const int rb = p.OW * C;
    const long total = (long)p.OH * rb;
    for (long i = (long)blockIdx.x * AS_NT + threadIdx.x; i < total; i += (long)gridDim.x * AS_NT) {
        const int y = (int)(i / rb), xb = (int)(i - (long)y * rb);
        const int x = xb / C;
        dst[i] = as_pad_byte<C>(p, f, y, x, xb - x * C);
    }
}

// 16 bytes a lane (the output rows and dst are 16-byte aligned): a chunk that lies inside the source and is aligned there is one load
template <int C>
__global__ __launch_bounds__(AS_NT) void as_pad16_kernel(const AsPad p) {
    const int f = blockIdx.y;
    uint8_t* dst = p.dst[f];
    const int rb = p.OW * C, row_chunks = rb >> 4;
    const long total = (long)p.OH * row_chunks;
    for (long i = (long)blockIdx.x * AS_NT + threadIdx.x; i < total; i += (long)gridDim.x * AS_NT) {
        const int y = (int)(i / row_chunks), xb0 = (int)(i - (long)y * row_chunks) << 4;
        const int sy = y - p.y_off, sb0 = xb0 - p.x_off * C;
        uint4 v;
        const bool inside = (unsigned)sy < (unsigned)p.H && sb0 >= 0 && sb0 + 16 <= p.W * C;
        const uintptr_t s = inside ? (uintptr_t)p.src[f] + (uintptr_t)((long)sy * p.W * C + sb0) : 1;
        if ((s & 15) == 0) {
            v = *reinterpret_cast<const uint4*>(s);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int xb = xb0 + j, x = xb / C;
                w[j >> 2] |= (uint32_t)as_pad_byte<C>(p, f, y, x, xb - x * C) << (8 * (j & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(dst + i * 16) = v;
    }
}

// ---- the 99-tap blur: rows into uint16 (at most 255 * 256), columns into uint8 = (sum + 2^15) >> 16 ---------------------------------
__global__ __launch_bounds__(AS_NT) void as_gauss_rows_kernel(const uint8_t* __restrict__ src, int H, int W, int C, const AsGauss g, uint16_t* __restrict__ tmp) {
    const int rb = W * C;
    const long total = (long)H * rb;
    for (long i = (long)blockIdx.x * AS_NT + threadIdx.x; i < total; i += (long)gridDim.x * AS_NT) {
        const int y = (int)(i / rb), xb = (int)(i - (long)y * rb);
        const int x = xb / C, c = xb - x * C;
        const uint8_t* row = src + (long)y * rb + c;
        uint32_t s = 0;
        if (x >= AS_TAPS / 2 && x + AS_TAPS / 2 < W) {
#pragma unroll 9
            for (int t = 0; t < AS_TAPS; ++t) s += (uint32_t)row[(x + t - AS_TAPS / 2) * C] * g.k[t];
        } else {
            for (int t = 0; t < AS_TAPS; ++t) s += (uint32_t)row[reflect101(x + t - AS_TAPS / 2, W) * C] * g.k[t];
        }
        tmp[i] = (uint16_t)s;
    }
}

__global__ __launch_bounds__(AS_NT) void as_gauss_columns_kernel(const uint16_t* __restrict__ tmp, int H, int W, int C, const AsGauss g, uint8_t* __restrict__ dst) {
    const int rb = W * C;
    const long total = (long)H * rb;
    for (long i = (long)blockIdx.x * AS_NT + threadIdx.x; i < total; i += (long)gridDim.x * AS_NT) {
        const int y = (int)(i / rb), xb = (int)(i - (long)y * rb);
        uint32_t s = 0;                                               // at most 255 * 256 * 256
        if (y >= AS_TAPS / 2 && y + AS_TAPS / 2 < H) {
#pragma unroll 9
            for (int t = 0; t < AS_TAPS; ++t) s += (uint32_t)tmp[(long)(y + t - AS_TAPS / 2) * rb + xb] * g.k[t];
        } else {
            for (int t = 0; t < AS_TAPS; ++t) s += (uint32_t)tmp[(long)reflect101(y + t - AS_TAPS / 2, H) * rb + xb] * g.k[t];
        }
        dst[i] = (uint8_t)((s + (1u << 15)) >> 16);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct AsRange {
    uintptr_t lo, hi;
};

// true when a written range shares a byte with a read range or with another written range
bool as_overlap(const std::vector<AsRange>& writes, const std::vector<AsRange>& reads) {
    for (size_t i = 0; i < writes.size(); ++i) {
        for (const AsRange& r : reads)
            if (writes[i].lo < r.hi && r.lo < writes[i].hi) return true;
        for (size_t j = i + 1; j < writes.size(); ++j)
            if (writes[i].lo < writes[j].hi && writes[j].lo < writes[i].hi) return true;
    }
    return false;
}

void as_add(std::vector<AsRange>& v, const void* p, size_t bytes) { v.push_back({(uintptr_t)p, (uintptr_t)p + bytes}); }

unsigned as_grid(long work_items, int frames) {
    const long per_frame = std::max(1L, (long)AS_BLOCKS / std::max(1, frames));
    return (unsigned)std::max(1L, std::min(per_frame, (work_items + AS_NT - 1) / AS_NT));
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_aspect_bar_sums_u8(const void* const* frames, int n, int height, int width, int channels, uint32_t* row_sums, uint32_t* column_sums,
                          void* stream) {
    const char* fn = "fw_aspect_bar_sums_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (const int s = check_pointer_table(fn, frames, n, AS_BATCH)) return s;
    if (!row_sums || !column_sums) return invalid(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (const int s = hip_status(fn, hipMemsetAsync(row_sums, 0, sizeof(uint32_t) * (size_t)n * height, st))) return s;
    if (const int s = hip_status(fn, hipMemsetAsync(column_sums, 0, sizeof(uint32_t) * (size_t)n * width, st))) return s;
    AsFrames t{};
    for (int i = 0; i < n; ++i) t.p[i] = (const uint8_t*)frames[i];
    const dim3 grid((unsigned)((width + AS_NT - 1) / AS_NT), (unsigned)((height + AS_BAND - 1) / AS_BAND), (unsigned)n);
    if (channels == 3) hipLaunchKernelGGL(as_bar_sums_kernel<3>, grid, dim3(AS_NT), 0, st, t, height, width, row_sums, column_sums);
    else hipLaunchKernelGGL(as_bar_sums_kernel<1>, grid, dim3(AS_NT), 0, st, t, height, width, row_sums, column_sums);
    return hip_status(fn, hipGetLastError());
}

int fw_aspect_crop_u8(const void* const* src, void* const* dst, int n, int height, int width, int channels, int x, int y, int crop_width,
                      int crop_height, int flip, void* stream) {
    const char* fn = "fw_aspect_crop_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (const int s = check_pointer_table(fn, src, n, AS_BATCH)) return s;
    if (const int s = check_pointer_table(fn, (const void* const*)dst, n, AS_BATCH)) return s;
    if (x < 0 || y < 0 || crop_width < 1 || crop_height < 1 || (long)x + crop_width > width || (long)y + crop_height > height)
        return invalid(fn, "a crop of at least one row and one column inside the frame expected");
    if (flip < 0 || flip > 2) return invalid(fn, "flip 0 (none), 1 (columns reversed) or 2 (rows reversed) expected");
    const size_t src_bytes = (size_t)height * width * channels, dst_bytes = (size_t)crop_height * crop_width * channels;
    std::vector<AsRange> writes, reads;
    AsPairs t{};
    uintptr_t any = 0;
    for (int i = 0; i < n; ++i) {
        t.src[i] = (const uint8_t*)src[i], t.dst[i] = (uint8_t*)dst[i];
        as_add(reads, src[i], src_bytes), as_add(writes, dst[i], dst_bytes);
        any |= (uintptr_t)src[i] | (uintptr_t)dst[i];
    }
    if (as_overlap(writes, reads)) return invalid(fn, "a dst overlaps a source frame or another dst of the call");
    const long src_row = (long)width * channels, row = (long)crop_width * channels, first = ((long)y * width + x) * channels;
    if (flip == 0 && ((any | (uintptr_t)src_row | (uintptr_t)row | (uintptr_t)first) & 15) == 0) {
        const dim3 grid(as_grid((long)crop_height * (row >> 4), n), (unsigned)n);
        hipLaunchKernelGGL(as_crop16_kernel, grid, dim3(AS_NT), 0, (hipStream_t)stream, t, src_row, first, (int)(row >> 4), crop_height);
    } else {
        const dim3 grid(as_grid((long)dst_bytes, n), (unsigned)n);
        if (channels == 3) hipLaunchKernelGGL(as_crop_kernel<3>, grid, dim3(AS_NT), 0, (hipStream_t)stream, t, width, x, y, crop_width, crop_height, flip);
        else hipLaunchKernelGGL(as_crop_kernel<1>, grid, dim3(AS_NT), 0, (hipStream_t)stream, t, width, x, y, crop_width, crop_height, flip);
    }
    return hip_status(fn, hipGetLastError());
}

int fw_aspect_pad_u8(const void* const* src, void* const* dst, int n, int height, int width, int channels, int out_height, int out_width,
                     int x_offset, int y_offset, int mode, const uint8_t* color, const void* const* background, const void* const* strips,
                     void* stream) {
    const char* fn = "fw_aspect_pad_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (const int s = check_side_and_channels(fn, out_height, out_width, channels)) return s;
    if (const int s = check_pointer_table(fn, src, n, AS_BATCH)) return s;
    if (const int s = check_pointer_table(fn, (const void* const*)dst, n, AS_BATCH)) return s;
    if (x_offset < 0 || y_offset < 0 || (long)x_offset + width > out_width || (long)y_offset + height > out_height)
        return invalid(fn, "the source at (x_offset, y_offset) must lie inside the output frame");
    if (mode < 0 || mode > 2) return invalid(fn, "mode 0 (colour), 1 (mirror) or 2 (background) expected");
    if (!color) return invalid(fn, "null pointer");
    if (mode == 2)
        if (const int s = check_pointer_table(fn, background, n, AS_BATCH)) return s;
    const int bars[4] = {x_offset, out_width - x_offset - width, y_offset, out_height - y_offset - height};
    const int extent[4] = {width, width, height, height};
    const size_t strip_bytes[4] = {(size_t)height * bars[0] * channels, (size_t)height * bars[1] * channels, (size_t)bars[2] * width * channels,
                                   (size_t)bars[3] * width * channels};
    const size_t src_bytes = (size_t)height * width * channels, dst_bytes = (size_t)out_height * out_width * channels;
    std::vector<AsRange> writes, reads;
    AsPad p{};
    p.H = height, p.W = width, p.OH = out_height, p.OW = out_width, p.x_off = x_offset, p.y_off = y_offset, p.mode = mode;
    for (int c = 0; c < 3; ++c) p.color[c] = color[c];
    uintptr_t any = (uintptr_t)((long)out_width * channels);
    for (int i = 0; i < n; ++i) {
        p.src[i] = (const uint8_t*)src[i], p.dst[i] = (uint8_t*)dst[i];
        as_add(reads, src[i], src_bytes), as_add(writes, dst[i], dst_bytes);
        any |= (uintptr_t)dst[i];
        if (mode == 2) p.back[i] = (const uint8_t*)background[i], as_add(reads, background[i], dst_bytes);
        for (int k = 0; mode == 1 && k < 4; ++k) {
            if (bars[k] <= extent[k]) continue;                       // a pure reversal of the source's edge: no strip is read
            if (!strips || !strips[4L * i + k]) return invalid(fn, "a bar wider than the source needs its stretched strip");
            p.strip[i][k] = (const uint8_t*)strips[4L * i + k];
            as_add(reads, strips[4L * i + k], strip_bytes[k]);
        }
    }
    if (as_overlap(writes, reads)) return invalid(fn, "a dst overlaps a source, a background, a strip or another dst of the call");
    if ((any & 15) == 0) {
        const dim3 grid(as_grid((long)(dst_bytes >> 4), n), (unsigned)n);
        if (channels == 3) hipLaunchKernelGGL(as_pad16_kernel<3>, grid, dim3(AS_NT), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(as_pad16_kernel<1>, grid, dim3(AS_NT), 0, (hipStream_t)stream, p);
    } else {
        const dim3 grid(as_grid((long)dst_bytes, n), (unsigned)n);
        if (channels == 3) hipLaunchKernelGGL(as_pad_kernel<3>, grid, dim3(AS_NT), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(as_pad_kernel<1>, grid, dim3(AS_NT), 0, (hipStream_t)stream, p);
    }
    return hip_status(fn, hipGetLastError());
}

int fw_aspect_gauss99_u8(const uint8_t* src, int height, int width, int channels, const uint16_t* weights, uint16_t* scratch, uint8_t* dst,
                         void* stream) {
    const char* fn = "fw_aspect_gauss99_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (!src || !weights || !scratch || !dst) return invalid(fn, "null pointer");
    AsGauss g{};
    unsigned sum = 0;
    for (int t = 0; t < AS_TAPS; ++t) g.k[t] = weights[t], sum += weights[t];
    if (sum != 256) return invalid(fn, "99 weights of 8 fractional bits that sum to 256 expected");   // what keeps the sums in 16 and 32 bits
    const size_t bytes = (size_t)height * width * channels;
    std::vector<AsRange> writes, reads;
    as_add(reads, src, bytes), as_add(writes, scratch, 2 * bytes), as_add(writes, dst, bytes);
    if (as_overlap(writes, reads)) return invalid(fn, "src, scratch and dst must not overlap");
    const dim3 grid(as_grid((long)bytes, 1));
    hipLaunchKernelGGL(as_gauss_rows_kernel, grid, dim3(AS_NT), 0, (hipStream_t)stream, src, height, width, channels, g, scratch);
    if (const int s = hip_status(fn, hipGetLastError())) return s;
    hipLaunchKernelGGL(as_gauss_columns_kernel, grid, dim3(AS_NT), 0, (hipStream_t)stream, scratch, height, width, channels, g, dst);
    return hip_status(fn, hipGetLastError());
}

}  // extern "C"
