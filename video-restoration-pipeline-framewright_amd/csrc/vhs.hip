// The frame path of the reference's VHS processor (src/framewright/processors/format/vhs.py: `process` with its five list methods,
// `detect_vhs_artifacts` with its `_detect_*` helpers) on uint8 frames that are already in HBM, behind the deinterlacer and in front
// of every other stage.  tests/vhs_ref.py is the contract, held byte for byte against the reference's own functions on the CPU.
//
// What runs here and what on the host.  The reference detects on every frame and then rewrites a few rows, boxes or the whole
// frame.  The device forms the statistics a decision needs as exact integers (or fetches the 30 gray rows a float32 variance is
// taken over), the host takes the decision with the reference's own NumPy steps on those few values, and the device rewrites:
//   fw_vhs_gray_stats_u8        per row sum |g[x+1] - g[x]| (tracking), the bottom 30 gray rows (head switching), runs of g > 250 or
//                               g < 5 (dropouts) appended to a list through an atomic counter
//   fw_vhs_blend_rows_u8        dst[y] = trunc(fa * ((src[y1] + src[y2]) / 2) + fb * src[y]) in float32 for a table of rows: the
//                               tracking repair (y1 = y - 1, y2 = y + 1) and the head-switching blend (y1 = y2 = the source row)
//   fw_vhs_box_gray_sums_u8     sum of g over a box of a neighbour frame: is it clean (10 n < sum < 245 n)
//   fw_vhs_dropout_repair_u8    boxes rewritten in place: temporal (float32 blend with the clean neighbour) or spatial (float64
//                               interpolation between the flank columns); the boxes of one call are disjoint, flanks included
//   fw_vhs_edge_counts_u8       luma edges per row; fw_vhs_chroma_samples_u8: the k-th edge of a row and the R / B step offsets
//   fw_vhs_chroma_shift_u8      R moves right and B left by a per-frame shift
//   fw_vhs_rainbow_u8           the 5-tap diagonal stencil as an integer sum of eighths, then the float32 blend, borders included
//   fw_vhs_column_sums_u8, fw_vhs_jitter_shifts_u8, fw_vhs_saturation_f64   dot crawl, jitter and rainbow analysis
//
// Arithmetic.  float32(fa) * a + float32(fb) * b is two rounded products and a rounded sum (__fmul_rn / __fadd_rn: never an FMA), the
// cast truncates.  The spatial fallback is float64 throughout except float32(1 - s) * float32(result), which is rounded to float32
// first.  Luma is 0.299 R + 0.587 G + 0.114 B in float64 from left to right, then float32.
//
// Kernel shape.  Everything is bound by one read and one write of the frame, or one read for the statistics.  The rainbow stencil, the
// one step that rewrites every byte of every frame, takes 16 bytes a lane when the frames and their rows are 16-byte aligned; it and
// every other kernel otherwise take one byte (or one pixel) a lane, so frames may start at any byte.  Up to 32 frames share a launch, their
// pointers travel by value in the kernel arguments, so a batch needs no pointer table in device memory and the entry checks every
// pointer.  Tables of rows, boxes and samples are in device memory (the host builds them from the statistics); the entry cannot read
// them, so every kernel checks each table entry against the frame itself and skips what does not lie inside: nothing outside a frame
// is read or written whatever a table holds.  No scratch; LDS only in the jitter kernel (two gray rows).  Row and box sums are
// integers reduced across a wave with shuffles and written by one lane: the same in every run.
#include "stage_common.h"

#pragma clang fp contract(off)

namespace fw {
namespace {

constexpr int VH_NT = 256;
constexpr int VH_WAVES = VH_NT / 64;
constexpr int VH_BATCH = 32;                                          // frames of one launch that writes frames
constexpr int VH_TABLE = 64;                                          // frames a box table may refer to (a batch and its neighbours)
constexpr int VH_MAX_SIDE = MAX_FRAME_SIDE;
constexpr int VH_MAX_ENTRIES = 1 << 24;
constexpr int VH_BLOCKS = 4096;
constexpr int VH_BOTTOM = 30;

struct VhFrames {
    const uint8_t* p[VH_TABLE];
};

struct VhPairs {
    const uint8_t* src[VH_BATCH];
    uint8_t* dst[VH_BATCH];
    int shift[VH_BATCH];
};

struct VhOuts {
    uint8_t* p[VH_BATCH];
};

__device__ __forceinline__ uint8_t vh_blend(float fa, float a, float fb, float b) {
    return (uint8_t)(int)__fadd_rn(__fmul_rn(fa, a), __fmul_rn(fb, b));   // in [0, 255.0001]: fa + fb is 1 to an ulp
}

__device__ __forceinline__ float vh_luma(const uint8_t* p) {
    return (float)__dadd_rn(__dadd_rn(__dmul_rn(0.299, (double)p[2]), __dmul_rn(0.587, (double)p[1])), __dmul_rn(0.114, (double)p[0]));
}

__device__ __forceinline__ bool vh_edge(const uint8_t* row, int x) {  // x < W - 1
    return fabsf(__fsub_rn(vh_luma(row + 3L * (x + 1)), vh_luma(row + 3L * x))) > 30.f;
}

// ---- statistics of the gray image: one wave per row ------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(VH_NT) void vh_gray_stats_kernel(const VhFrames frames, int frame0, int H, int W, int min_len, long long* row_sums,
                                                              uint8_t* bottom, int* runs, int cap, int* count) {
    const int f = blockIdx.y;
    const uint8_t* img = frames.p[f];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int y = blockIdx.x * VH_WAVES + wave; y < H; y += gridDim.x * VH_WAVES) {
        const uint8_t* row = img + (long)y * W * C;
        uint32_t s = 0;                                               // at most 255 * 16383
        for (int x0 = 0; x0 < W; x0 += 64) {
            const int x = x0 + lane;
            if (x < W) {
                const int g = gray_bgr<C>(row + (long)x * C);
                if (x + 1 < W) s += (uint32_t)abs(gray_bgr<C>(row + (long)(x + 1) * C) - g);
                if (bottom && y >= H - VH_BOTTOM) bottom[((long)(frame0 + f) * VH_BOTTOM + (y - (H - VH_BOTTOM))) * W + x] = (uint8_t)g;
                if (runs) {
                    const int gp = x > 0 ? gray_bgr<C>(row + (long)(x - 1) * C) : 128;     // 128: neither bright nor dark
                    const bool bright = g > 250 && !(gp > 250), dark = g < 5 && !(gp < 5);
                    if (bright || dark) {                             // this pixel starts a run: its lane walks to the end
                        int len = 1;
                        while (x + len < W) {
                            const int gn = gray_bgr<C>(row + (long)(x + len) * C);
                            if (!(bright ? gn > 250 : gn < 5)) break;
                            ++len;
                        }
                        if (len >= min_len) {
                            const int at = atomicAdd(count, 1);       // the true count, also beyond the capacity
                            if (at < cap) {
                                int* r = runs + 4L * at;
                                r[0] = frame0 + f, r[1] = x, r[2] = y, r[3] = len;
                            }
                        }
                    }
                }
            }
        }
        if (row_sums) {
            s = wave_sum(s);
            if (lane == 0) row_sums[(long)(frame0 + f) * H + y] = (long long)s;
        }
    }
}

// ---- rows: dst[y] = trunc(fa * ((src[y1] + src[y2]) / 2) + fb * src[y]) ---------------------------------------------------------------
__global__ __launch_bounds__(VH_NT) void vh_blend_rows_kernel(const VhPairs t, int n, int rows, int row_bytes, const int* spec_i, const float* spec_f,
                                                              int m) {
    for (int e = blockIdx.x; e < m; e += gridDim.x) {
        const int f = spec_i[4L * e], y = spec_i[4L * e + 1], y1 = spec_i[4L * e + 2], y2 = spec_i[4L * e + 3];
        if ((unsigned)f >= (unsigned)n || (unsigned)y >= (unsigned)rows || (unsigned)y1 >= (unsigned)rows || (unsigned)y2 >= (unsigned)rows) continue;
        const float fa = spec_f[2L * e], fb = spec_f[2L * e + 1];
        const uint8_t* src = t.src[f];
        uint8_t* dst = t.dst[f];
        for (int b = threadIdx.x; b < row_bytes; b += VH_NT) {
            const float mid = __fadd_rn((float)src[(long)y1 * row_bytes + b], (float)src[(long)y2 * row_bytes + b]) * 0.5f;   // exact
            dst[(long)y * row_bytes + b] = vh_blend(fa, mid, fb, (float)src[(long)y * row_bytes + b]);
        }
    }
}

// ---- rainbow: 0.5 c + 0.125 (four diagonal neighbours) as eighths, blended with the frame; borders are blended with themselves ----------
__global__ __launch_bounds__(VH_NT) void vh_rainbow_kernel(const VhPairs t, int H, int W, float fa, float fb) {
    const uint8_t* src = t.src[blockIdx.y];
    uint8_t* dst = t.dst[blockIdx.y];
    const int rb = W * 3;
    const int total = H * rb;                                         // < 2^31 (host-checked)
    for (int i = blockIdx.x * VH_NT + threadIdx.x; i < total; i += gridDim.x * VH_NT) {
        const int y = i / rb, xb = i - y * rb, x = xb / 3;
        const int c = src[i];
        int s8 = 8 * c;
        if (y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2)
            s8 = 4 * c + src[i - rb - 3] + src[i - rb + 3] + src[i + rb - 3] + src[i + rb + 3];
        float v = __fadd_rn(__fmul_rn(fa, (float)s8 * 0.125f), __fmul_rn(fb, (float)c));
        v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
        dst[i] = (uint8_t)(int)v;
    }
}

// the same, 16 bytes a lane, when both frames and the rows are 16-byte aligned (1080p BGR rows are 5760 bytes, 576i 2160): the centre
// chunk and, for an inner row, the chunks above and below with the word before and the word behind them - the diagonal neighbours of
// byte j are bytes j - 3 and j + 3 of those rows.  Seven 16-byte and four 4-byte loads for one 16-byte store, all but one L2 hits.
__device__ __forceinline__ int vh_byte(const uint32_t* w, int idx) { return (int)((w[idx >> 2] >> (8 * (idx & 3))) & 255u); }

__global__ __launch_bounds__(VH_NT) void vh_rainbow16_kernel(const VhPairs t, int H, int W, float fa, float fb) {
    const uint8_t* src = t.src[blockIdx.y];
    uint8_t* dst = t.dst[blockIdx.y];
    const int rb = W * 3;                                             // a multiple of 16
    const int nchunk = rb >> 4;
    const int total = H * nchunk;
    for (int i = blockIdx.x * VH_NT + threadIdx.x; i < total; i += gridDim.x * VH_NT) {
        const int y = i / nchunk, xb0 = (i - y * nchunk) << 4;
        const long at = (long)y * rb + xb0;
        const uint4 c4 = *reinterpret_cast<const uint4*>(src + at);
        const uint32_t cw[4] = {c4.x, c4.y, c4.z, c4.w};
        uint32_t up[6] = {0, 0, 0, 0, 0, 0}, dn[6] = {0, 0, 0, 0, 0, 0};   // [0] the word before the chunk, [1..4] the chunk, [5] the word behind
        const bool inner = y >= 1 && y <= H - 2;
        if (inner) {
            const uint8_t* u = src + at - rb;
            const uint8_t* d = src + at + rb;
            const uint4 a = *reinterpret_cast<const uint4*>(u), b = *reinterpret_cast<const uint4*>(d);
            up[1] = a.x, up[2] = a.y, up[3] = a.z, up[4] = a.w;
            dn[1] = b.x, dn[2] = b.y, dn[3] = b.z, dn[4] = b.w;
            if (xb0 > 0) up[0] = *reinterpret_cast<const uint32_t*>(u - 4), dn[0] = *reinterpret_cast<const uint32_t*>(d - 4);
            if (xb0 + 16 < rb) up[5] = *reinterpret_cast<const uint32_t*>(u + 16), dn[5] = *reinterpret_cast<const uint32_t*>(d + 16);
        }
        uint32_t ow[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int xb = xb0 + j;
            const int c = vh_byte(cw, j);
            int s8 = 8 * c;
            if (inner && xb >= 3 && xb <= rb - 4)                     // pixel 1 .. W - 2: bytes j - 3 and j + 3 lie in the row
                s8 = 4 * c + vh_byte(up, 4 + j - 3) + vh_byte(up, 4 + j + 3) + vh_byte(dn, 4 + j - 3) + vh_byte(dn, 4 + j + 3);
            float v = __fadd_rn(__fmul_rn(fa, (float)s8 * 0.125f), __fmul_rn(fb, (float)c));
            v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
            ow[j >> 2] |= (uint32_t)(int)v << (8 * (j & 3));
        }
        *reinterpret_cast<uint4*>(dst + at) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
}

// ---- dropouts ---------------------------------------------------------------------------------------------------------------------------
// tasks[e] = {frame, x, y, w, h}; sums[e] = sum of gray over the box, -1 for an entry that does not lie inside a frame
template <int C>
__global__ __launch_bounds__(VH_NT) void vh_box_sums_kernel(const VhFrames frames, int n, int H, int W, const int* tasks, int m, long long* sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = blockIdx.x * VH_WAVES + wave; e < m; e += gridDim.x * VH_WAVES) {
        const int f = tasks[5L * e], x = tasks[5L * e + 1], y = tasks[5L * e + 2], w = tasks[5L * e + 3], h = tasks[5L * e + 4];
        const bool ok = (unsigned)f < (unsigned)n && x >= 0 && y >= 0 && w > 0 && h > 0 && (long)x + w <= W && (long)y + h <= H;
        unsigned long long s = 0;
        if (ok) {
            const uint8_t* img = frames.p[f];
            const long np = (long)w * h;
            for (long i = lane; i < np; i += 64) {
                const long yy = y + i / w, xx = x + i % w;
                s += (unsigned long long)gray_bgr<C>(img + (yy * W + xx) * C);
            }
        }
        s = wave_sum(s);
        if (lane == 0) sums[e] = ok ? (long long)s : -1LL;
    }
}

// boxes[e] = {mode, result frame, source frame, x, y, w, h, 0}; mode 0 temporal, 1 spatial; one workgroup per box
template <int C>
__global__ __launch_bounds__(VH_NT) void vh_repair_kernel(const VhFrames srcs, int ns, const VhOuts results, int nr, int H, int W, const int* boxes,
                                                          int m, float fa, float fb, double strength) {
    for (int e = blockIdx.x; e < m; e += gridDim.x) {
        const int* b = boxes + 8L * e;
        const int mode = b[0], ri = b[1], si = b[2], x = b[3], y = b[4], w = b[5], h = b[6];
        bool ok = (unsigned)ri < (unsigned)nr && x >= 0 && y >= 0 && w > 0 && h > 0 && (long)x + w <= W && (long)y + h <= H;
        ok = ok && (mode == 0 ? (unsigned)si < (unsigned)ns : (mode == 1 && x > 0 && (long)x + w < W));
        if (!ok) continue;
        uint8_t* res = results.p[ri];
        const uint8_t* src = mode == 0 ? srcs.p[si] : nullptr;
        const long nb = (long)w * h * C;
        for (long i = threadIdx.x; i < nb; i += VH_NT) {
            const int c = (int)(i % C);
            const long px = i / C;
            const int xx = x + (int)(px % w), yy = y + (int)(px / w);
            const long at = ((long)yy * W + xx) * C + c;
            const float r = (float)res[at];
            if (mode == 0) {
                res[at] = vh_blend(fa, (float)src[at], fb, r);
            } else {
                const double tt = (double)(xx - x + 1) / (double)(w + 1);
                const double left = (double)res[((long)yy * W + (x - 1)) * C + c], right = (double)res[((long)yy * W + (x + w)) * C + c];
                const double mid = __dadd_rn(__dmul_rn(1.0 - tt, left), __dmul_rn(tt, right));
                res[at] = (uint8_t)(int)__dadd_rn(__dmul_rn(strength, mid), (double)__fmul_rn(fb, r));
            }
        }
    }
}

// ---- chroma bleed -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VH_NT) void vh_edge_counts_kernel(const VhFrames frames, int frame0, int H, int W, int* counts) {
    const int f = blockIdx.y;
    const uint8_t* img = frames.p[f];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int y = blockIdx.x * VH_WAVES + wave; y < H; y += gridDim.x * VH_WAVES) {
        const uint8_t* row = img + (long)y * W * 3;
        uint32_t c = 0;
        for (int x = lane; x < W - 1; x += 64) c += vh_edge(row, x) ? 1u : 0u;
        c = wave_sum(c);
        if (lane == 0) counts[(long)(frame0 + f) * H + y] = (int)c;
    }
}

// samples[e] = {frame, row, k}: the k-th luma edge of the row; out[e] = {offset of R, offset of B}, -1 where the channel's largest
// step in [max(0, x - 5), min(W - 2, x + 5)) is not above 20, -2 for an entry that names no edge
__global__ __launch_bounds__(VH_NT) void vh_chroma_samples_kernel(const VhFrames frames, int n, int H, int W, const int* samples, int m, int* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = blockIdx.x * VH_WAVES + wave; e < m; e += gridDim.x * VH_WAVES) {
        const int f = samples[3L * e], y = samples[3L * e + 1], k = samples[3L * e + 2];
        int found = -1;
        if ((unsigned)f < (unsigned)n && (unsigned)y < (unsigned)H && k >= 0) {       // the same in every lane of the wave
            const uint8_t* row = frames.p[f] + (long)y * W * 3;
            int seen = 0;
            for (int x0 = 0; x0 < W - 1 && found < 0; x0 += 64) {
                const int x = x0 + lane;
                const bool is_edge = x < W - 1 && vh_edge(row, x);
                const unsigned long long mask = __ballot(is_edge);
                const int c = __popcll(mask);
                if (k < seen + c) {
                    const bool hit = is_edge && __popcll(mask & ((1ULL << lane) - 1ULL)) == k - seen;
                    found = x0 + __ffsll((long long)__ballot(hit)) - 1;
                }
                seen += c;
            }
            if (found >= 0) {
                const int xs = max(0, found - 5), xe = min(W - 2, found + 5);
                const int xi = xs + lane;
                int kr = -1, kb = -1;                                 // (step << 8) | (255 - lane): the largest step, first position
                if (lane < 10 && xi < xe) {
                    const uint8_t* p = row + 3L * xi;
                    kr = (abs((int)p[5] - (int)p[2]) << 8) | (255 - lane);
                    kb = (abs((int)p[3] - (int)p[0]) << 8) | (255 - lane);
                }
                kr = wave_max(kr), kb = wave_max(kb);
                if (lane == 0) {
                    out[2L * e] = kr >= 0 && (kr >> 8) > 20 ? abs(xs + (255 - (kr & 255)) - found) : -1;
                    out[2L * e + 1] = kb >= 0 && (kb >> 8) > 20 ? abs(xs + (255 - (kb & 255)) - found) : -1;
                }
            }
        }
        if (found < 0 && lane == 0) out[2L * e] = -2, out[2L * e + 1] = -2;
    }
}

__global__ __launch_bounds__(VH_NT) void vh_chroma_shift_kernel(const VhPairs t, int H, int W) {
    const uint8_t* src = t.src[blockIdx.y];
    uint8_t* dst = t.dst[blockIdx.y];
    const int shift = t.shift[blockIdx.y];
    const int npix = H * W;
    for (int i = blockIdx.x * VH_NT + threadIdx.x; i < npix; i += gridDim.x * VH_NT) {
        const int x = i % W;
        dst[3L * i] = src[3L * (x + shift < W ? i + shift : i)];
        dst[3L * i + 1] = src[3L * i + 1];
        dst[3L * i + 2] = src[3L * (x >= shift ? i - shift : i) + 2];
    }
}

// ---- analysis ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VH_NT) void vh_column_sums_kernel(const uint8_t* img, int H, int W, long long* sums) {
    const int x = blockIdx.x * VH_NT + threadIdx.x;
    if (x >= W - 1) return;
    uint32_t s = 0;
    for (int y = 0; y < H; ++y) {
        const uint8_t* p = img + ((long)y * W + x) * 3;
        s += (uint32_t)abs(abs((int)p[5] - (int)p[3]) - abs((int)p[2] - (int)p[0]));
    }
    sums[x] = (long long)s;
}

// one workgroup per sampled row y = 1 + 5 e: c[j] = sum_n cur[n + j - W / 2] * prev[n] in int32, the first maximum
template <int C>
__global__ __launch_bounds__(VH_NT) void vh_jitter_kernel(const uint8_t* img, int H, int W, int* shifts) {
    extern __shared__ uint8_t vh_lds[];
    __shared__ unsigned long long best[VH_NT];
    uint8_t* cur = vh_lds;
    uint8_t* prev = vh_lds + W;
    const int y = 1 + 5 * blockIdx.x;
    for (int x = threadIdx.x; x < W; x += VH_NT) {
        cur[x] = (uint8_t)gray_bgr<C>(img + ((long)y * W + x) * C);
        prev[x] = (uint8_t)gray_bgr<C>(img + ((long)(y - 1) * W + x) * C);
    }
    __syncthreads();
    unsigned long long mine = 0;                                      // (sum << 32) | (2^32 - 1 - j): the largest sum, first position
    for (int j = threadIdx.x; j < W; j += VH_NT) {
        const int k = j - W / 2;
        const int n0 = k < 0 ? -k : 0, n1 = k > 0 ? W - k : W;
        uint32_t acc = 0;                                             // <= 16384 * 255^2 < 2^31
        for (int n = n0; n < n1; ++n) acc += (uint32_t)cur[n + k] * (uint32_t)prev[n];
        const unsigned long long key = ((unsigned long long)acc << 32) | (unsigned long long)(0xffffffffu - (uint32_t)j);
        mine = key > mine ? key : mine;
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int s = VH_NT / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s && best[threadIdx.x + s] > best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) shifts[blockIdx.x] = (int)(0xffffffffu - (uint32_t)(best[0] & 0xffffffffULL)) - W / 2;
}

__global__ __launch_bounds__(VH_NT) void vh_saturation_kernel(const uint8_t* img, long npix, double* out) {
    for (long i = (long)blockIdx.x * VH_NT + threadIdx.x; i < npix; i += (long)gridDim.x * VH_NT) {
        const uint8_t* p = img + 3 * i;
        const int mx = max(max((int)p[0], (int)p[1]), (int)p[2]), mn = min(min((int)p[0], (int)p[1]), (int)p[2]);
        out[i] = mx > 0 ? (double)(mx - mn) / __dadd_rn((double)mx, 1e-6) : 0.0;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// true when a destination (kind 0) of the call overlaps a source (kind 1): all frames are `bytes` long
bool vh_overlap(const void* const* dst, int nd, const void* const* src, int ns, size_t bytes) {
    FrameMarks marks;
    for (int i = 0; i < nd; ++i) marks.emplace_back((uintptr_t)dst[i], 0);
    for (int i = 0; i < ns; ++i) marks.emplace_back((uintptr_t)src[i], 1);
    return frames_overlap(marks, bytes);
}

// destinations must not overlap each other either (two frames of a batch written at once)
bool vh_self_overlap(const void* const* dst, int n, size_t bytes) {
    std::vector<uintptr_t> a;
    for (int i = 0; i < n; ++i) a.push_back((uintptr_t)dst[i]);
    std::sort(a.begin(), a.end());
    for (size_t i = 1; i < a.size(); ++i)
        if (a[i] - a[i - 1] < bytes) return true;
    return false;
}

int vh_fill_pairs(const char* fn, const void* const* src, void* const* dst, int n, size_t bytes, VhPairs& t) {
    if (const int s = check_pointer_table(fn, src, n, VH_BATCH)) return s;
    if (const int s = check_pointer_table(fn, (const void* const*)dst, n, VH_BATCH)) return s;
    if (vh_overlap((const void* const*)dst, n, src, n, bytes)) return invalid(fn, "a dst overlaps a source frame of the call");
    if (vh_self_overlap((const void* const*)dst, n, bytes)) return invalid(fn, "two dst frames of the call overlap");
    for (int i = 0; i < n; ++i) t.src[i] = (const uint8_t*)src[i], t.dst[i] = (uint8_t*)dst[i], t.shift[i] = 0;
    return FW_OK;
}

unsigned vh_grid(long work_items, int frames) {
    const long per_frame = std::max(1L, (long)VH_BLOCKS / std::max(1, frames));
    return (unsigned)std::max(1L, std::min(per_frame, work_items));
}

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

int fw_vhs_gray_stats_u8(const void* const* frames, int n, int height, int width, int channels, int min_length, int64_t* row_sums,
                         uint8_t* bottom, int32_t* runs, int run_capacity, int32_t* run_count, void* stream) {
    const char* fn = "fw_vhs_gray_stats_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (const int s = check_pointer_table(fn, frames, n <= VH_MAX_ENTRIES ? n : 0, 0)) return s;   // more than 2^24: refused as none
    if (!row_sums && !bottom && !runs) return invalid(fn, "nothing asked for");
    if (bottom && height < VH_BOTTOM) return invalid(fn, "the bottom rows need a frame of at least 30 rows");
    if (runs && (!run_count || run_capacity < 1 || run_capacity > VH_MAX_ENTRIES || min_length < 1))
        return invalid(fn, "a run list needs a counter, a capacity of 1 .. 2^24 and a minimum length of at least 1");
    hipStream_t st = (hipStream_t)stream;
    if (runs)
        if (const int s = hip_status(fn, hipMemsetAsync(run_count, 0, sizeof(int32_t), st))) return s;
    for (int base = 0; base < n; base += VH_BATCH) {
        const int m = std::min(VH_BATCH, n - base);
        VhFrames t{};
        for (int i = 0; i < m; ++i) t.p[i] = (const uint8_t*)frames[base + i];
        const dim3 grid(vh_grid((height + VH_WAVES - 1) / VH_WAVES, m), (unsigned)m);
        if (channels == 3)
            hipLaunchKernelGGL(vh_gray_stats_kernel<3>, grid, dim3(VH_NT), 0, st, t, base, height, width, min_length, (long long*)row_sums, bottom,
                               runs, run_capacity, run_count);
        else
            hipLaunchKernelGGL(vh_gray_stats_kernel<1>, grid, dim3(VH_NT), 0, st, t, base, height, width, min_length, (long long*)row_sums, bottom,
                               runs, run_capacity, run_count);
        if (const int s = hip_status(fn, hipGetLastError())) return s;
    }
    return FW_OK;
}

int fw_vhs_blend_rows_u8(const void* const* src, void* const* dst, int n, int rows, int64_t row_bytes, const int32_t* spec_rows,
                         const float* spec_factors, int m, void* stream) {
    const char* fn = "fw_vhs_blend_rows_u8";
    if (rows < 1 || rows > VH_MAX_SIDE || row_bytes < 1 || row_bytes > 4L * VH_MAX_SIDE) return invalid(fn, "1 .. 16384 rows of 1 .. 65536 bytes expected");
    if (!spec_rows || !spec_factors) return invalid(fn, "null pointer");
    if (m < 1 || m > VH_MAX_ENTRIES) return invalid(fn, "1 .. 2^24 rows expected");
    VhPairs t{};
    // dst[y] is written while src[y1], src[y2] of other table rows are read: dst may equal nothing of the sources
    if (const int s = vh_fill_pairs(fn, src, dst, n, (size_t)rows * (size_t)row_bytes, t)) return s;
    hipLaunchKernelGGL(vh_blend_rows_kernel, dim3((unsigned)std::min(m, VH_BLOCKS)), dim3(VH_NT), 0, (hipStream_t)stream, t, n, rows, (int)row_bytes,
                       spec_rows, spec_factors, m);
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_rainbow_u8(const void* const* src, void* const* dst, int n, int height, int width, float fa, float fb, void* stream) {
    const char* fn = "fw_vhs_rainbow_u8";
    if (const int s = check_side_and_channels(fn, height, width, 3)) return s;
    VhPairs t{};
    if (const int s = vh_fill_pairs(fn, src, dst, n, (size_t)height * width * 3, t)) return s;
    const long total = (long)height * width * 3;                      // <= 3 * 2^28
    uintptr_t any = (uintptr_t)(width * 3);
    for (int i = 0; i < n; ++i) any |= (uintptr_t)t.src[i] | (uintptr_t)t.dst[i];
    if ((any & 15) == 0) {
        const dim3 grid(vh_grid((total / 16 + VH_NT - 1) / VH_NT, n), (unsigned)n);
        hipLaunchKernelGGL(vh_rainbow16_kernel, grid, dim3(VH_NT), 0, (hipStream_t)stream, t, height, width, fa, fb);
    } else {
        const dim3 grid(vh_grid((total + VH_NT - 1) / VH_NT, n), (unsigned)n);
        hipLaunchKernelGGL(vh_rainbow_kernel, grid, dim3(VH_NT), 0, (hipStream_t)stream, t, height, width, fa, fb);
    }
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_box_gray_sums_u8(const void* const* frames, int n, int height, int width, int channels, const int32_t* tasks, int m, int64_t* sums,
                            void* stream) {
    const char* fn = "fw_vhs_box_gray_sums_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (const int s = check_pointer_table(fn, frames, n, VH_TABLE)) return s;
    if (!tasks || !sums) return invalid(fn, "null pointer");
    if (m < 1 || m > VH_MAX_ENTRIES) return invalid(fn, "1 .. 2^24 boxes expected");
    VhFrames t{};
    for (int i = 0; i < n; ++i) t.p[i] = (const uint8_t*)frames[i];
    const dim3 grid((unsigned)std::min((m + VH_WAVES - 1) / VH_WAVES, VH_BLOCKS));
    if (channels == 3) hipLaunchKernelGGL(vh_box_sums_kernel<3>, grid, dim3(VH_NT), 0, (hipStream_t)stream, t, n, height, width, tasks, m, (long long*)sums);
    else hipLaunchKernelGGL(vh_box_sums_kernel<1>, grid, dim3(VH_NT), 0, (hipStream_t)stream, t, n, height, width, tasks, m, (long long*)sums);
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_dropout_repair_u8(const void* const* sources, int n_sources, void* const* results, int n_results, int height, int width, int channels,
                             const int32_t* boxes, int m, double strength, void* stream) {
    const char* fn = "fw_vhs_dropout_repair_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (const int s = check_pointer_table(fn, sources, n_sources, VH_TABLE)) return s;
    if (const int s = check_pointer_table(fn, (const void* const*)results, n_results, VH_BATCH)) return s;
    if (!boxes) return invalid(fn, "null pointer");
    if (m < 1 || m > VH_MAX_ENTRIES) return invalid(fn, "1 .. 2^24 boxes expected");
    if (!(strength > 0.0 && strength <= 1.0)) return invalid(fn, "a strength in (0, 1] expected");
    const size_t bytes = (size_t)height * width * channels;
    if (vh_overlap((const void* const*)results, n_results, sources, n_sources, bytes)) return invalid(fn, "a result frame overlaps a source frame of the call");
    if (vh_self_overlap((const void* const*)results, n_results, bytes)) return invalid(fn, "two result frames of the call overlap");
    VhFrames s{};
    VhOuts r{};
    for (int i = 0; i < n_sources; ++i) s.p[i] = (const uint8_t*)sources[i];
    for (int i = 0; i < n_results; ++i) r.p[i] = (uint8_t*)results[i];
    const float fa = (float)strength, fb = (float)(1.0 - strength);
    const dim3 grid((unsigned)std::min(m, VH_BLOCKS));
    if (channels == 3)
        hipLaunchKernelGGL(vh_repair_kernel<3>, grid, dim3(VH_NT), 0, (hipStream_t)stream, s, n_sources, r, n_results, height, width, boxes, m, fa, fb, strength);
    else
        hipLaunchKernelGGL(vh_repair_kernel<1>, grid, dim3(VH_NT), 0, (hipStream_t)stream, s, n_sources, r, n_results, height, width, boxes, m, fa, fb, strength);
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_edge_counts_u8(const void* const* frames, int n, int height, int width, int32_t* counts, void* stream) {
    const char* fn = "fw_vhs_edge_counts_u8";
    if (const int s = check_side_and_channels(fn, height, width, 3)) return s;
    if (!counts) return invalid(fn, "null pointer");
    if (const int s = check_pointer_table(fn, frames, n <= VH_MAX_ENTRIES ? n : 0, 0)) return s;
    for (int base = 0; base < n; base += VH_BATCH) {
        const int m = std::min(VH_BATCH, n - base);
        VhFrames t{};
        for (int i = 0; i < m; ++i) t.p[i] = (const uint8_t*)frames[base + i];
        const dim3 grid(vh_grid((height + VH_WAVES - 1) / VH_WAVES, m), (unsigned)m);
        hipLaunchKernelGGL(vh_edge_counts_kernel, grid, dim3(VH_NT), 0, (hipStream_t)stream, t, base, height, width, counts);
        if (const int s = hip_status(fn, hipGetLastError())) return s;
    }
    return FW_OK;
}

int fw_vhs_chroma_samples_u8(const void* const* frames, int n, int height, int width, const int32_t* samples, int m, int32_t* offsets, void* stream) {
    const char* fn = "fw_vhs_chroma_samples_u8";
    if (const int s = check_side_and_channels(fn, height, width, 3)) return s;
    if (const int s = check_pointer_table(fn, frames, n, VH_TABLE)) return s;
    if (!samples || !offsets) return invalid(fn, "null pointer");
    if (m < 1 || m > 100 * VH_TABLE) return invalid(fn, "1 .. 6400 samples expected (at most 100 a frame)");
    VhFrames t{};
    for (int i = 0; i < n; ++i) t.p[i] = (const uint8_t*)frames[i];
    const dim3 grid((unsigned)std::min((m + VH_WAVES - 1) / VH_WAVES, VH_BLOCKS));
    hipLaunchKernelGGL(vh_chroma_samples_kernel, grid, dim3(VH_NT), 0, (hipStream_t)stream, t, n, height, width, samples, m, offsets);
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_chroma_shift_u8(const void* const* src, void* const* dst, const int32_t* shifts, int n, int height, int width, void* stream) {
    const char* fn = "fw_vhs_chroma_shift_u8";
    if (const int s = check_side_and_channels(fn, height, width, 3)) return s;
    if (!shifts) return invalid(fn, "null pointer");
    VhPairs t{};
    if (const int s = vh_fill_pairs(fn, src, dst, n, (size_t)height * width * 3, t)) return s;
    for (int i = 0; i < n; ++i) {
        if (shifts[i] < 0 || shifts[i] > 2) return invalid(fn, "a shift of 0 .. 2 columns expected");
        t.shift[i] = shifts[i];
    }
    const long npix = (long)height * width;
    const dim3 grid(vh_grid((npix + VH_NT - 1) / VH_NT, n), (unsigned)n);
    hipLaunchKernelGGL(vh_chroma_shift_kernel, grid, dim3(VH_NT), 0, (hipStream_t)stream, t, height, width);
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_column_sums_u8(const uint8_t* frame, int height, int width, int64_t* sums, void* stream) {
    const char* fn = "fw_vhs_column_sums_u8";
    if (const int s = check_side_and_channels(fn, height, width, 3)) return s;
    if (!frame || !sums) return invalid(fn, "null pointer");
    if (width < 2) return invalid(fn, "at least two columns expected");
    hipLaunchKernelGGL(vh_column_sums_kernel, dim3((unsigned)((width - 1 + VH_NT - 1) / VH_NT)), dim3(VH_NT), 0, (hipStream_t)stream, frame, height, width,
                       (long long*)sums);
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_jitter_shifts_u8(const uint8_t* frame, int height, int width, int channels, int32_t* shifts, void* stream) {
    const char* fn = "fw_vhs_jitter_shifts_u8";
    if (const int s = check_side_and_channels(fn, height, width, channels)) return s;
    if (!frame || !shifts) return invalid(fn, "null pointer");
    if (height < 3) return invalid(fn, "at least three rows expected");
    const int rows = (height - 2 + 4) / 5;                            // y = 1, 6, 11 ... <= height - 2
    const size_t lds = 2 * (size_t)width;                             // <= 32 KiB
    if (channels == 3) hipLaunchKernelGGL(vh_jitter_kernel<3>, dim3((unsigned)rows), dim3(VH_NT), lds, (hipStream_t)stream, frame, height, width, shifts);
    else hipLaunchKernelGGL(vh_jitter_kernel<1>, dim3((unsigned)rows), dim3(VH_NT), lds, (hipStream_t)stream, frame, height, width, shifts);
    return hip_status(fn, hipGetLastError());
}

int fw_vhs_saturation_f64(const uint8_t* frame, int height, int width, double* saturation, void* stream) {
    const char* fn = "fw_vhs_saturation_f64";
    if (const int s = check_side_and_channels(fn, height, width, 3)) return s;
    if (!frame || !saturation) return invalid(fn, "null pointer");
    const long npix = (long)height * width;
    hipLaunchKernelGGL(vh_saturation_kernel, dim3(vh_grid((npix + VH_NT - 1) / VH_NT, 1)), dim3(VH_NT), 0, (hipStream_t)stream, frame, npix, saturation);
    return hip_status(fn, hipGetLastError());
}

}  // extern "C"
