// The frame path of the reference's deinterlacer (src/framewright/processors/format/interlace.py: `_deinterlace_yadif`,
// `_deinterlace_bwdif`, `_deinterlace_bob`, `_detect_combing`, `_detect_field_order_single`, `_frame_difference`) on uint8 frames that
// are already in HBM, in front of every other stage.  Every output byte is an integer function of the input bytes
// (tests/deinterlace_ref.py, held byte for byte against the reference's own functions on the CPU), so the contract is equality.
//
//   fw_deinterlace_u8 / fw_deinterlace_batch_u8   line interpolation: a frame is `rows` rows of `row_bytes` bytes (W * C, no padding)
//     YADIF   1 <= y <= H-2, y % 2 == parity : out[y] = (cur[y-1] + cur[y+1]) >> 1
//     BWDIF   2 <= y <= H-3, y % 2 == parity : num = 3 * (9 * (cur[y-1] + cur[y+1]) - (cur[y-2] + cur[y+2])) + 4 * (prev[y] + next[y]),
//             out[y] = clamp(num, 0, 255 * 64) >> 6   (the reference's float32 expression: multiples of 1/64 below 2^10, exact)
//     BOB     out = cv2.resize(cur[parity::2], (W, H)): the width does not change, so OpenCV's fixed-point bilinear is vertical
//             only: hor = 2048 * s, out[d] = (((b0 * (hor[s0] >> 4)) >> 16) + ((b1 * (hor[s1] >> 4)) >> 16) + 2) >> 2 with the row
//             table of oracle/face_ref.resize_linear_u8 (float fx from a double product, 11-bit coefficients, rounded half to even).
//             The field is read in place with a row step of two; nothing is copied first.
//     every other row is copied.  parity 1 = TFF (odd rows rebuilt), 0 = BFF.
//   fw_interlace_stats_u8     per frame {n_comb, s_field, s_odd, s_even} of the 14-bit gray image as int64
//   fw_frame_absdiff_sum_u8   per pair sum |gray(a) - gray(b)| as int64
//
// Kernel shape.  The interpolation is one read and one write of the frame (BWDIF: seven row reads per rebuilt byte, five of them
// rows the neighbouring lanes' rows read too - L2).  A lane takes V consecutive bytes of one row: V = 16 when every pointer and
// row_bytes are multiples of 16 (1080p BGR rows are 5760 bytes, 576i 2160), V = 4 when row_bytes is a multiple of 4 and every pointer
// has the same address modulo 4 (a view that starts on an odd byte: the first and last word of a row are then taken byte by byte,
// only bytes inside the row are touched), else V = 1.  Up to 32 frames share a launch: their pointers travel by value in the kernel
// arguments (1 KiB), so a batch needs no table in device memory and the host entry can check every pointer.  No LDS, no scratch.
// The statistics are integer sums, so their order is free: a wave takes a row pair, reduces its three sums with cross-lane shuffles
// and adds them to the frame's four int64 with 64-bit atomic adds from vector memory instructions (global_atomic_add_x2) on a
// buffer the entry zeroes on the same stream; the result is the same in every run.
#include "stage_common.h"

#pragma clang fp contract(off)

namespace fw {
namespace {

constexpr int DI_NT = 256;
constexpr int DI_BATCH = 32;                                          // frames of one launch (4 x 32 pointers by value)
constexpr int DI_MAX_ROWS = MAX_FRAME_SIDE;
constexpr long DI_MAX_ROW_BYTES = 4L * 16384;
constexpr int DI_BLOCKS = 4096;                                       // workgroups of one launch, all frames together, about

struct DiTasks {
    const uint8_t* cur[DI_BATCH];
    const uint8_t* prev[DI_BATCH];
    const uint8_t* next[DI_BATCH];
    uint8_t* dst[DI_BATCH];
};

enum { K_COPY = 0, K_AVG = 1, K_BWDIF = 2, K_BOB = 3 };

template <int V>
struct Chunk {
    uint32_t w[V == 16 ? 4 : 1];
};

// V bytes at p, of which only those with index in [j0, j1) are read (the others are 0): one load when all are inside
template <int V>
__device__ __forceinline__ Chunk<V> di_load(const uint8_t* p, int j0, int j1) {
    Chunk<V> c;
    if constexpr (V == 1) {
        c.w[0] = *p;
    } else if (j0 == 0 && j1 == V) {
        if constexpr (V == 16) {
            const uint4 t = *reinterpret_cast<const uint4*>(p);
            c.w[0] = t.x, c.w[1] = t.y, c.w[2] = t.z, c.w[3] = t.w;
        } else {
            c.w[0] = *reinterpret_cast<const uint32_t*>(p);
        }
    } else {
#pragma unroll
        for (int k = 0; k < (V == 16 ? 4 : 1); ++k) c.w[k] = 0;
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j >= j0 && j < j1) c.w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
    return c;
}

template <int V>
__device__ __forceinline__ void di_store(uint8_t* p, int j0, int j1, const Chunk<V>& c) {
    if constexpr (V == 1) {
        *p = (uint8_t)c.w[0];
    } else if (j0 == 0 && j1 == V) {
        if constexpr (V == 16) *reinterpret_cast<uint4*>(p) = make_uint4(c.w[0], c.w[1], c.w[2], c.w[3]);
        else *reinterpret_cast<uint32_t*>(p) = c.w[0];
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j >= j0 && j < j1) p[j] = (uint8_t)(c.w[j >> 2] >> (8 * (j & 3)));
    }
}

__device__ __forceinline__ int byte_of(uint32_t w, int j) { return (int)((w >> (8 * j)) & 255u); }

// The row table of cv2.resize's 8-bit INTER_LINEAR for destination row d of `dsize` from a field of `ssize` rows (scale = ssize /
// dsize formed on the host as 1.0 / (dsize / ssize), both divisions in double): source row and the two 11-bit coefficients.
__device__ __forceinline__ void bob_row(int d, int ssize, double scale, int& s0, int& b0, int& b1) {
    float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    s0 = (int)floorf(f);
    f = __fsub_rn(f, (float)s0);
    if (s0 < 0) f = 0.f, s0 = 0;
    if (s0 >= ssize - 1) f = 0.f, s0 = ssize - 1;
    b0 = (int)rintf(__fsub_rn(1.f, f) * 2048.f);                      // saturate_cast<short>: to nearest even; |c| <= 2048
    b1 = (int)rintf(f * 2048.f);
}

template <int V>
__global__ __launch_bounds__(DI_NT) void deinterlace_kernel(const DiTasks tasks, int rows, int row_bytes, int mode, int parity, double bob_scale) {
    constexpr int NW = V == 16 ? 4 : 1;
    const int f = blockIdx.y;
    const uint8_t* cur = tasks.cur[f];
    const uint8_t* prev = tasks.prev[f];
    const uint8_t* next = tasks.next[f];
    uint8_t* dst = tasks.dst[f];
    const int off = (int)((uintptr_t)dst & (V - 1));                  // the same for every pointer of the launch (host-checked)
    const int nchunk = row_bytes / V + (off ? 1 : 0);                 // V divides row_bytes
    const int total = rows * nchunk;                                  // < 2^31 (host-checked)
    const int field_rows = (rows + 1 - parity) >> 1;                  // BOB: rows of cur[parity::2]
    for (int i = blockIdx.x * DI_NT + threadIdx.x; i < total; i += gridDim.x * DI_NT) {
        const int y = i / nchunk, k = i - y * nchunk;
        const int x = k * V - off;                                    // byte column of the chunk's first byte; may be < 0
        const int j0 = x < 0 ? -x : 0;
        const int j1 = row_bytes - x < V ? row_bytes - x : V;
        const long at = (long)y * row_bytes + x;
        int kind = K_COPY, b0 = 0, b1 = 0;
        long ra = at, rb = at;
        if (mode == FW_DEINTERLACE_YADIF) {
            if (y >= 1 && y <= rows - 2 && (y & 1) == parity) kind = K_AVG;
        } else if (mode == FW_DEINTERLACE_BWDIF) {
            if (y >= 2 && y <= rows - 3 && (y & 1) == parity) kind = K_BWDIF;
        } else {
            int s0;
            bob_row(y, field_rows, bob_scale, s0, b0, b1);
            const int s1 = s0 + 1 < field_rows ? s0 + 1 : field_rows - 1;
            ra = (long)(2 * s0 + parity) * row_bytes + x;
            rb = (long)(2 * s1 + parity) * row_bytes + x;
            kind = K_BOB;
        }
        Chunk<V> o;
        if (kind == K_COPY) {
            o = di_load<V>(cur + at, j0, j1);
        } else if (kind == K_AVG) {
            const Chunk<V> a = di_load<V>(cur + at - row_bytes, j0, j1), b = di_load<V>(cur + at + row_bytes, j0, j1);
#pragma unroll
            for (int w = 0; w < NW; ++w) o.w[w] = (a.w[w] & b.w[w]) + (((a.w[w] ^ b.w[w]) & 0xfefefefeu) >> 1);   // per byte (a + b) >> 1
        } else if (kind == K_BWDIF) {
            const Chunk<V> a = di_load<V>(cur + at - row_bytes, j0, j1), b = di_load<V>(cur + at + row_bytes, j0, j1);
            const Chunk<V> c = di_load<V>(cur + at - 2L * row_bytes, j0, j1), d = di_load<V>(cur + at + 2L * row_bytes, j0, j1);
            const Chunk<V> p = di_load<V>(prev + at, j0, j1), n = di_load<V>(next + at, j0, j1);
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                uint32_t r = 0;
#pragma unroll
                for (int j = 0; j < (V == 1 ? 1 : 4); ++j) {
                    int num = 3 * (9 * (byte_of(a.w[w], j) + byte_of(b.w[w], j)) - (byte_of(c.w[w], j) + byte_of(d.w[w], j))) +
                              4 * (byte_of(p.w[w], j) + byte_of(n.w[w], j));
                    num = num < 0 ? 0 : (num > 255 * 64 ? 255 * 64 : num);
                    r |= (uint32_t)(num >> 6) << (8 * j);
                }
                o.w[w] = r;
            }
        } else {
            const Chunk<V> a = di_load<V>(cur + ra, j0, j1), b = di_load<V>(cur + rb, j0, j1);
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                uint32_t r = 0;
#pragma unroll
                for (int j = 0; j < (V == 1 ? 1 : 4); ++j) {
                    int v = (((b0 * (byte_of(a.w[w], j) << 7)) >> 16) + ((b1 * (byte_of(b.w[w], j) << 7)) >> 16) + 2) >> 2;
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                    r |= (uint32_t)v << (8 * j);
                }
                o.w[w] = r;
            }
        }
        di_store<V>(dst + at, j0, j1, o);
    }
}

// ---- statistics -------------------------------------------------------------------------------------------------------------------
// one wave per row pair r: rows 2r, 2r+1 and, for r < R-1, 2r+2, 2r+3; out[f] = {n_comb, s_field, s_odd, s_even}
template <int C>
__global__ __launch_bounds__(DI_NT) void interlace_stats_kernel(const DiTasks tasks, int H, int W, unsigned long long* out) {
    const int f = blockIdx.y;
    const uint8_t* img = tasks.cur[f];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = H >> 1;
    const long rb = (long)W * C;
    unsigned long long n_comb = 0, s_field = 0, s_odd = 0, s_even = 0;     // lane 0's are the wave's
    for (int r = blockIdx.x * (DI_NT / 64) + wave; r < R; r += gridDim.x * (DI_NT / 64)) {
        const uint8_t* r0 = img + (long)(2 * r) * rb;
        const bool more = r < R - 1;
        uint32_t sf = 0, so = 0, se = 0;                              // a row's sum is at most 255 * 16384
        for (int x = lane; x < W; x += 64) {
            const int g0 = gray_bgr<C>(r0 + (long)x * C), g1 = gray_bgr<C>(r0 + rb + (long)x * C);
            sf += (uint32_t)abs(g1 - g0);
            if (more) {
                const int g2 = gray_bgr<C>(r0 + 2 * rb + (long)x * C), g3 = gray_bgr<C>(r0 + 3 * rb + (long)x * C);
                se += (uint32_t)abs(g2 - g0);
                so += (uint32_t)abs(g3 - g1);
            }
        }
        sf = wave_sum(sf), so = wave_sum(so), se = wave_sum(se);
        n_comb += sf > 30u * (uint32_t)W ? 1 : 0;
        s_field += sf, s_odd += so, s_even += se;
    }
    if (lane == 0 && R > 0) {
        unsigned long long* o = out + 4L * f;
        if (n_comb) atomicAdd(o, n_comb);
        if (s_field) atomicAdd(o + 1, s_field);
        if (s_odd) atomicAdd(o + 2, s_odd);
        if (s_even) atomicAdd(o + 3, s_even);
    }
}

// out[f] = sum |gray(a) - gray(b)| over the frame; a = tasks.cur[f], b = tasks.prev[f]
template <int C>
__global__ __launch_bounds__(DI_NT) void absdiff_sum_kernel(const DiTasks tasks, long npix, unsigned long long* out) {
    const int f = blockIdx.y;
    const uint8_t* a = tasks.cur[f];
    const uint8_t* b = tasks.prev[f];
    unsigned long long s = 0;
    for (long i = (long)blockIdx.x * DI_NT + threadIdx.x; i < npix; i += (long)gridDim.x * DI_NT)
        s += (unsigned long long)abs(gray_bgr<C>(a + i * C) - gray_bgr<C>(b + i * C));
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out + f, s);
}

// tasks: n x {cur, prev, next, dst}; everything is checked before the first launch (prev and next may be null unless the mode reads
// them, so the table is checked here and not by check_pointer_table)
int deinterlace_run(const char* fn, const void* const* table, int n, int rows, int64_t row_bytes, int mode, int parity, hipStream_t st) {
    if (!table) return invalid(fn, "null pointer");
    if (n < 1) return invalid(fn, "at least one frame expected");
    if (rows < 1 || rows > DI_MAX_ROWS || row_bytes < 1 || row_bytes > DI_MAX_ROW_BYTES)
        return invalid(fn, "1 .. 16384 rows of 1 .. 65536 bytes expected");
    if (mode != FW_DEINTERLACE_YADIF && mode != FW_DEINTERLACE_BWDIF && mode != FW_DEINTERLACE_BOB) return invalid(fn, "unknown mode");
    if (parity != 0 && parity != 1) return invalid(fn, "parity is 0 (even rows) or 1 (odd rows)");
    if (mode == FW_DEINTERLACE_BOB && rows < 2) return invalid(fn, "BOB needs two rows: the odd field of one row is empty");
    const bool temporal = mode == FW_DEINTERLACE_BWDIF;
    const size_t bytes = (size_t)rows * (size_t)row_bytes;
    FrameMarks marks;
    marks.reserve(4 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const void* cur = table[4 * i];
        const void* prev = table[4 * i + 1];
        const void* next = table[4 * i + 2];
        const void* dst = table[4 * i + 3];
        if (!cur || !dst || (temporal && (!prev || !next))) return invalid(fn, "null pointer");
        marks.emplace_back((uintptr_t)dst, 0);
        marks.emplace_back((uintptr_t)cur, 1);
        if (temporal) marks.emplace_back((uintptr_t)prev, 1), marks.emplace_back((uintptr_t)next, 1);
    }
    if (frames_overlap(marks, bytes)) return invalid(fn, "a dst overlaps a source frame of the call (rebuilt rows are read as neighbours)");
    const int field_rows = (rows + 1 - parity) >> 1;
    const double bob_scale = 1.0 / ((double)rows / (double)field_rows);
    for (int base = 0; base < n; base += DI_BATCH) {
        const int m = std::min(DI_BATCH, n - base);
        DiTasks t{};
        uintptr_t any = 0;
        bool alike4 = true;
        for (int i = 0; i < m; ++i) {
            const void* const* e = table + 4 * (size_t)(base + i);
            t.cur[i] = (const uint8_t*)e[0];
            t.prev[i] = temporal ? (const uint8_t*)e[1] : t.cur[i];
            t.next[i] = temporal ? (const uint8_t*)e[2] : t.cur[i];
            t.dst[i] = (uint8_t*)e[3];
            for (const void* p : {(const void*)t.cur[i], (const void*)t.prev[i], (const void*)t.next[i], (const void*)t.dst[i]}) {
                any |= (uintptr_t)p;
                alike4 = alike4 && (((uintptr_t)p ^ (uintptr_t)t.dst[0]) & 3) == 0;
            }
        }
        const int V = (row_bytes % 16 == 0 && (any & 15) == 0) ? 16 : (row_bytes % 4 == 0 && alike4) ? 4 : 1;
        const long nchunk = row_bytes / V + (V == 4 && ((uintptr_t)t.dst[0] & 3) ? 1 : 0);
        const long total = (long)rows * nchunk;                       // <= 16384 * 65536 = 2^30
        const long per_frame = std::max(1L, (long)DI_BLOCKS / m);
        const dim3 grid((unsigned)std::max(1L, std::min(per_frame, (total + DI_NT - 1) / DI_NT)), (unsigned)m);
        if (V == 16) hipLaunchKernelGGL(deinterlace_kernel<16>, grid, dim3(DI_NT), 0, st, t, rows, (int)row_bytes, mode, parity, bob_scale);
        else if (V == 4) hipLaunchKernelGGL(deinterlace_kernel<4>, grid, dim3(DI_NT), 0, st, t, rows, (int)row_bytes, mode, parity, bob_scale);
        else hipLaunchKernelGGL(deinterlace_kernel<1>, grid, dim3(DI_NT), 0, st, t, rows, (int)row_bytes, mode, parity, bob_scale);
        if (const int s = hip_status(fn, hipGetLastError())) return s;
    }
    return FW_OK;
}

int stats_check(const char* fn, const void* const* a, const void* const* b, bool pairs, int n, int H, int W, int C, const void* out) {
    if (!out) return invalid(fn, "null pointer");
    if (const int s = check_pointer_table(fn, a, n, 0)) return s;
    if (pairs)
        if (const int s = check_pointer_table(fn, b, n, 0)) return s;
    return check_side_and_channels(fn, H, W, C);
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_deinterlace_u8(const uint8_t* cur, const uint8_t* prev, const uint8_t* next, uint8_t* dst, int rows, int64_t row_bytes, int mode,
                      int parity, void* stream) {
    const void* table[4] = {cur, prev, next, dst};
    return deinterlace_run("fw_deinterlace_u8", table, 1, rows, row_bytes, mode, parity, (hipStream_t)stream);
}

int fw_deinterlace_batch_u8(const void* const* frames, int n, int rows, int64_t row_bytes, int mode, int parity, void* stream) {
    return deinterlace_run("fw_deinterlace_batch_u8", frames, n, rows, row_bytes, mode, parity, (hipStream_t)stream);
}

int fw_interlace_stats_u8(const void* const* frames, int n, int height, int width, int channels, int64_t* stats, void* stream) {
    const char* fn = "fw_interlace_stats_u8";
    if (const int s = stats_check(fn, frames, nullptr, false, n, height, width, channels, stats)) return s;
    hipStream_t st = (hipStream_t)stream;
    if (const int s = hip_status(fn, hipMemsetAsync(stats, 0, (size_t)n * 4 * sizeof(int64_t), st))) return s;
    const int R = height / 2;
    for (int base = 0; base < n; base += DI_BATCH) {
        const int m = std::min(DI_BATCH, n - base);
        DiTasks t{};
        for (int i = 0; i < m; ++i) t.cur[i] = (const uint8_t*)frames[base + i];
        const int waves = DI_NT / 64;
        const dim3 grid((unsigned)std::max(1, std::min(std::max(1, DI_BLOCKS / m), (R + waves - 1) / waves)), (unsigned)m);
        unsigned long long* out = reinterpret_cast<unsigned long long*>(stats) + 4L * base;
        if (channels == 3) hipLaunchKernelGGL(interlace_stats_kernel<3>, grid, dim3(DI_NT), 0, st, t, height, width, out);
        else hipLaunchKernelGGL(interlace_stats_kernel<1>, grid, dim3(DI_NT), 0, st, t, height, width, out);
        if (const int s = hip_status(fn, hipGetLastError())) return s;
    }
    return FW_OK;
}

int fw_frame_absdiff_sum_u8(const void* const* a, const void* const* b, int n, int height, int width, int channels, int64_t* sums,
                            void* stream) {
    const char* fn = "fw_frame_absdiff_sum_u8";
    if (const int s = stats_check(fn, a, b, true, n, height, width, channels, sums)) return s;
    hipStream_t st = (hipStream_t)stream;
    if (const int s = hip_status(fn, hipMemsetAsync(sums, 0, (size_t)n * sizeof(int64_t), st))) return s;
    const long npix = (long)height * width;
    for (int base = 0; base < n; base += DI_BATCH) {
        const int m = std::min(DI_BATCH, n - base);
        DiTasks t{};
        for (int i = 0; i < m; ++i) {
            t.cur[i] = (const uint8_t*)a[base + i];
            t.prev[i] = (const uint8_t*)b[base + i];
        }
        const long per_frame = std::max(1L, (long)DI_BLOCKS / m);
        const dim3 grid((unsigned)std::max(1L, std::min(per_frame, (npix + DI_NT - 1) / DI_NT)), (unsigned)m);
        unsigned long long* out = reinterpret_cast<unsigned long long*>(sums) + base;
        if (channels == 3) hipLaunchKernelGGL(absdiff_sum_kernel<3>, grid, dim3(DI_NT), 0, st, t, npix, out);
        else hipLaunchKernelGGL(absdiff_sum_kernel<1>, grid, dim3(DI_NT), 0, st, t, npix, out);
        if (const int s = hip_status(fn, hipGetLastError())) return s;
    }
    return FW_OK;
}

}  // extern "C"
