// Dense Farneback optical flow, its statistics and the confidence map on the device: the flow the classical temporal denoise
// consumes (reference src/framewright/processors/temporal_denoise.py:294-305, cv2.calcOpticalFlowFarneback(gray1, gray2, None, 0.5,
// 3, 15, 3, 5, 1.1, 0); :320 magnitude; :406-438 `_compute_flow_confidence`).  OpenCV's algorithm (modules/video/src/optflowgf.cpp)
// restated; tests/farneback_ref.py is the same sequence of operations in numpy and the contract these kernels are tested against
// (cv2 itself is absent where this is built: bit-parity with cv2 is unpinned).
//
// All fp32.  Planes are [H][W]; the polynomial-expansion and the matrix images are five such planes ([5][H][W]), so that every load
// and store of a wave is one contiguous row segment and the bilinear gather of the second image reads five nearly contiguous ones.
// The algorithm moves a few flops per byte, so the kernels are laid out by passes over HBM: each separable filter runs both
// directions in one kernel on a 64 x 16 tile staged with its halo in LDS (Gaussian blur, polynomial expansion, the 15 x 15 box mean),
// the gray conversion is part of the blur's tile load, the flow of the coarser level is upsampled inside the kernel that first needs
// it, and the box mean, the 2 x 2 solve and the next iteration's matrix update are one kernel (the new flow of a pixel is all its
// matrix update needs; the matrices are double-buffered because neighbouring tiles still read the old ones).  Intermediate flows are
// never written: only the last iteration of a level stores one.
// The box mean is 15 direct taps per direction inside the tile, never a frame-long running sum, so its rounding error does not grow
// with the frame.
// This file is compiled with -ffp-contract=off (build.py): magnitude = sqrt(fx * fx + fy * fy) has to round like numpy's, and without
// contraction the whole flow follows the float32 restatement operation for operation.
#include <math.h>

#include <vector>

#include "stage_common.h"

namespace fw {
namespace {

constexpr int TW = 64, TH = 16, NT = 256;
constexpr int MAX_BLUR_R = 9;    // 19 taps: scale 1/8 of the pyramid (sigma 3.5)
constexpr int POLY_N = 5;
constexpr int MAX_BOX_M = 15;    // winsize <= 31

__device__ __forceinline__ int of_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cv2.cvtColor(BGR2GRAY) on uint8 as float32
__device__ __forceinline__ float of_gray(const uint8_t* __restrict__ img, int channels, int W, int y, int x) {
    if (channels == 1) return (float)img[(size_t)y * W + x];
    return (float)gray_bgr<3>(img + ((size_t)y * W + x) * 3);
}

struct BlurTaps {
    float k[MAX_BLUR_R + 1];   // k[i]: tap at offset +/- i
    int r;
};

// gray -> float -> GaussianBlur(ksize, sigma), BORDER_REFLECT_101: rows then columns, k0 c + sum k_i (right_i + left_i)
__global__ __launch_bounds__(NT) void of_blur_u8_kernel(const uint8_t* __restrict__ img, int channels, int H, int W, BlurTaps bt,
                                                        float* __restrict__ out) {
    __shared__ float s_in[(TH + 2 * MAX_BLUR_R) * (TW + 2 * MAX_BLUR_R)];
    __shared__ float s_h[(TH + 2 * MAX_BLUR_R) * TW];
    const int r = bt.r, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, iw = TW + 2 * r, ih = TH + 2 * r;
    for (int i = threadIdx.x; i < ih * iw; i += NT) {
        const int ly = i / iw, lx = i - ly * iw;
        s_in[i] = of_gray(img, channels, W, reflect101(y0 - r + ly, H), reflect101(x0 - r + lx, W));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ih * TW; i += NT) {
        const int ly = i / TW, lx = i - ly * TW;
        const float* c = &s_in[ly * iw + lx + r];
        float acc = bt.k[0] * c[0];
        for (int j = 1; j <= r; ++j) acc = acc + bt.k[j] * (c[j] + c[-j]);
        s_h[i] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * TW; i += NT) {
        const int ly = i / TW, lx = i - ly * TW, gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        const float* c = &s_h[(ly + r) * TW + lx];
        float acc = bt.k[0] * c[0];
        for (int j = 1; j <= r; ++j) acc = acc + bt.k[j] * (c[j * TW] + c[-j * TW]);
        out[(size_t)gy * W + gx] = acc;
    }
}

// cv2.resize(INTER_LINEAR) source coordinate: (float)((d + 0.5) * scale - 0.5), floor, clamp with the fraction zeroed
__device__ __forceinline__ void of_resize_coord(int d, double scale, int sn, int& i0, int& i1, float& f) {
    f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    int s = (int)fl;
    f = f - fl;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= sn - 1) { f = 0.0f; s = sn - 1; }
    i0 = s;
    i1 = s + 1 < sn ? s + 1 : sn - 1;
}
__device__ __forceinline__ float of_bilerp(const float* __restrict__ src, int Ws, int y0, int y1, float fy, int x0, int x1, float fx) {
    const float top = src[(size_t)y0 * Ws + x0] * (1.0f - fx) + src[(size_t)y0 * Ws + x1] * fx;
    const float bot = src[(size_t)y1 * Ws + x0] * (1.0f - fx) + src[(size_t)y1 * Ws + x1] * fx;
    return top * (1.0f - fy) + bot * fy;
}

__global__ __launch_bounds__(NT) void of_resize_linear_kernel(const float* __restrict__ src, int Hs, int Ws, float* __restrict__ dst, int Hd,
                                                              int Wd, double sy, double sx) {
    const long n = (long)Hd * Wd;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const int y = (int)(i / Wd), x = (int)(i - (long)y * Wd);
        int x0, x1, y0, y1;
        float fx, fy;
        of_resize_coord(x, sx, Ws, x0, x1, fx);
        of_resize_coord(y, sy, Hs, y0, y1, fy);
        dst[i] = of_bilerp(src, Ws, y0, y1, fy, x0, x1, fx);
    }
}

struct PolyTaps {
    float g[POLY_N + 1], xg[POLY_N + 1], xxg[POLY_N + 1];
    float ig11, ig03, ig33, ig55;
};

// FarnebackPolyExp: [H][W] -> planes (b_y, b_x, A_yy, A_xx, A_xy); replicate border; columns first, then rows
__global__ __launch_bounds__(NT) void of_polyexp_kernel(const float* __restrict__ src, int H, int W, PolyTaps pt, float* __restrict__ dst) {
    constexpr int N = POLY_N, IW = TW + 2 * N, IH = TH + 2 * N;
    __shared__ float s_in[IH * IW];
    __shared__ float s_r[3][TH * IW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int i = threadIdx.x; i < IH * IW; i += NT) {
        const int ly = i / IW, lx = i - ly * IW;
        s_in[i] = src[(size_t)of_clamp(y0 - N + ly, 0, H - 1) * W + of_clamp(x0 - N + lx, 0, W - 1)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * IW; i += NT) {
        const int ly = i / IW, lx = i - ly * IW;
        const float* c = &s_in[(ly + N) * IW + lx];
        float r0 = c[0] * pt.g[0], r1 = 0.0f, r2 = 0.0f;
#pragma unroll
        for (int k = 1; k <= N; ++k) {
            const float a = c[-k * IW], b = c[k * IW], p = a + b;
            r0 = r0 + pt.g[k] * p;
            r1 = r1 + pt.xg[k] * (b - a);
            r2 = r2 + pt.xxg[k] * p;
        }
        s_r[0][i] = r0;
        s_r[1][i] = r1;
        s_r[2][i] = r2;
    }
    __syncthreads();
    const size_t hw = (size_t)H * W;
    for (int i = threadIdx.x; i < TH * TW; i += NT) {
        const int ly = i / TW, lx = i - ly * TW, gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        const float* c0 = &s_r[0][ly * IW + lx + N];
        const float* c1 = &s_r[1][ly * IW + lx + N];
        const float* c2 = &s_r[2][ly * IW + lx + N];
        float b1 = c0[0] * pt.g[0], b3 = c1[0] * pt.g[0], b5 = c2[0] * pt.g[0], b2 = 0.0f, b4 = 0.0f, b6 = 0.0f;
#pragma unroll
        for (int k = 1; k <= N; ++k) {
            const float tg = c0[k] + c0[-k];
            b1 = b1 + tg * pt.g[k];
            b4 = b4 + tg * pt.xxg[k];
            b2 = b2 + (c0[k] - c0[-k]) * pt.xg[k];
            b3 = b3 + (c1[k] + c1[-k]) * pt.g[k];
            b6 = b6 + (c1[k] - c1[-k]) * pt.xg[k];
            b5 = b5 + (c2[k] + c2[-k]) * pt.g[k];
        }
        const size_t o = (size_t)gy * W + gx;
        dst[o] = b3 * pt.ig11;
        dst[hw + o] = b2 * pt.ig11;
        dst[2 * hw + o] = b1 * pt.ig03 + b5 * pt.ig33;
        dst[3 * hw + o] = b1 * pt.ig03 + b4 * pt.ig33;
        dst[4 * hw + o] = b6 * pt.ig55;
    }
}

// the border ramp {0.14, 0.14, 0.4472, 0.4472, 0.4472} of FarnebackUpdateMatrices along one axis: (near edge) * (far edge)
__device__ __forceinline__ float of_border_ramp(int p, int len) {
    const float lo = p < 5 ? (p < 2 ? 0.14f : 0.4472f) : 1.0f;
    const float hi = p >= len - 5 ? (len - p - 1 < 2 ? 0.14f : 0.4472f) : 1.0f;
    return lo * hi;
}

// FarnebackUpdateMatrices for one pixel: (G11, G12, G22, h1, h2) from the two expansions and the displacement (dx, dy)
__device__ __forceinline__ void of_matrices(const float* __restrict__ R0, const float* __restrict__ R1, size_t hw, int H, int W, int y, int x,
                                            float dx, float dy, float* __restrict__ M) {
    const size_t o = (size_t)y * W + x;
    float fx = (float)x + dx, fy = (float)y + dy;
    const float flx = floorf(fx), fly = floorf(fy);
    float r2, r3, r4, r5, r6;
    // the comparison in float keeps NaN and out-of-int-range displacements on the "outside" branch
    if (flx >= 0.0f && flx < (float)(W - 1) && fly >= 0.0f && fly < (float)(H - 1)) {
        const int x1 = (int)flx, y1 = (int)fly;
        fx = fx - flx;
        fy = fy - fly;
        const float a00 = (1.0f - fx) * (1.0f - fy), a01 = fx * (1.0f - fy), a10 = (1.0f - fx) * fy, a11 = fx * fy;
        const float* p = R1 + (size_t)y1 * W + x1;
        r2 = a00 * p[0] + a01 * p[1] + a10 * p[W] + a11 * p[W + 1];
        p += hw;
        r3 = a00 * p[0] + a01 * p[1] + a10 * p[W] + a11 * p[W + 1];
        p += hw;
        r4 = a00 * p[0] + a01 * p[1] + a10 * p[W] + a11 * p[W + 1];
        p += hw;
        r5 = a00 * p[0] + a01 * p[1] + a10 * p[W] + a11 * p[W + 1];
        p += hw;
        r6 = a00 * p[0] + a01 * p[1] + a10 * p[W] + a11 * p[W + 1];
        r4 = (R0[2 * hw + o] + r4) * 0.5f;
        r5 = (R0[3 * hw + o] + r5) * 0.5f;
        r6 = (R0[4 * hw + o] + r6) * 0.25f;
    } else {
        r2 = r3 = 0.0f;
        r4 = R0[2 * hw + o];
        r5 = R0[3 * hw + o];
        r6 = R0[4 * hw + o] * 0.5f;
    }
    r2 = (R0[o] - r2) * 0.5f;
    r3 = (R0[hw + o] - r3) * 0.5f;
    r2 = r2 + (r4 * dy + r6 * dx);
    r3 = r3 + (r6 * dy + r5 * dx);
    const float yl = y < 5 ? (y < 2 ? 0.14f : 0.4472f) : 1.0f, yh = y >= H - 5 ? (H - y - 1 < 2 ? 0.14f : 0.4472f) : 1.0f;
    const float scale = of_border_ramp(x, W) * yl * yh;
    r2 *= scale; r3 *= scale; r4 *= scale; r5 *= scale; r6 *= scale;
    M[o] = r4 * r4 + r6 * r6;
    M[hw + o] = (r4 + r5) * r6;
    M[2 * hw + o] = r5 * r5 + r6 * r6;
    M[3 * hw + o] = r4 * r2 + r6 * r3;
    M[4 * hw + o] = r6 * r2 + r5 * r3;
}

// the first matrices of a level: displacement = the coarser level's flow, resized INTER_LINEAR and multiplied by 1 / pyr_scale (zero at
// the coarsest level: pfx == nullptr)
__global__ __launch_bounds__(NT) void of_init_matrices_kernel(const float* __restrict__ R0, const float* __restrict__ R1, const float* __restrict__ pfx,
                                                              const float* __restrict__ pfy, int Hp, int Wp, double sy, double sx, float mul,
                                                              int H, int W, float* __restrict__ M) {
    const long n = (long)H * W;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        float dx = 0.0f, dy = 0.0f;
        if (pfx) {
            int x0, x1, y0, y1;
            float fx, fy;
            of_resize_coord(x, sx, Wp, x0, x1, fx);
            of_resize_coord(y, sy, Hp, y0, y1, fy);
            dx = of_bilerp(pfx, Wp, y0, y1, fy, x0, x1, fx) * mul;
            dy = of_bilerp(pfy, Wp, y0, y1, fy, x0, x1, fx) * mul;
        }
        of_matrices(R0, R1, (size_t)n, H, W, y, x, dx, dy, M);
    }
}

// One iteration of FarnebackUpdateFlow_Blur (flags = 0): (2m + 1)^2 box mean of the five matrix planes (replicate border; 2m + 1 direct
// taps down the columns, then along the rows), the 2 x 2 solve, and - Mout != nullptr - the matrices of the next iteration from the new
// flow; fx_out / fy_out != nullptr stores the flow (the last iteration of a level).
__global__ __launch_bounds__(NT) void of_flow_iter_kernel(const float* __restrict__ M, const float* __restrict__ R0, const float* __restrict__ R1, int H,
                                                          int W, int m, float scale, float* __restrict__ Mout, float* __restrict__ fx_out,
                                                          float* __restrict__ fy_out) {
    __shared__ float s_in[(TH + 2 * MAX_BOX_M) * (TW + 2 * MAX_BOX_M)];
    __shared__ float s_v[TH * (TW + 2 * MAX_BOX_M)];
    constexpr int PER = TH * TW / NT;   // 4 pixels per thread: column threadIdx & 63, rows (threadIdx >> 6) + 4 q
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, iw = TW + 2 * m, ih = TH + 2 * m, taps = 2 * m + 1;
    const size_t hw = (size_t)H * W;
    float g[PER][5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const float* Mc = M + c * hw;
        for (int i = threadIdx.x; i < ih * iw; i += NT) {
            const int ly = i / iw, lx = i - ly * iw;
            s_in[i] = Mc[(size_t)of_clamp(y0 - m + ly, 0, H - 1) * W + of_clamp(x0 - m + lx, 0, W - 1)];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TH * iw; i += NT) {
            const int ly = i / iw, lx = i - ly * iw;
            const float* c0 = &s_in[ly * iw + lx];
            float acc = c0[0];
            for (int j = 1; j < taps; ++j) acc = acc + c0[j * iw];
            s_v[i] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = threadIdx.x + q * NT, ly = i / TW, lx = i - ly * TW;
            const float* c0 = &s_v[ly * iw + lx];
            float acc = c0[0];
            for (int j = 1; j < taps; ++j) acc = acc + c0[j];
            g[q][c] = acc * scale;
        }
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = threadIdx.x + q * NT, ly = i / TW, lx = i - ly * TW, gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        const float g11 = g[q][0], g12 = g[q][1], g22 = g[q][2], h1 = g[q][3], h2 = g[q][4];
        const float idet = 1.0f / (g11 * g22 - g12 * g12 + 1e-3f);
        const float dx = (g11 * h2 - g12 * h1) * idet, dy = (g22 * h1 - g12 * h2) * idet;
        if (fx_out) {
            fx_out[(size_t)gy * W + gx] = dx;
            fy_out[(size_t)gy * W + gx] = dy;
        }
        if (Mout) of_matrices(R0, R1, hw, H, W, gy, gx, dx, dy, Mout);
    }
}

// magnitude = sqrt(fx^2 + fy^2) (each operation rounded on its own, as numpy does) and the local-variance map of
// `_compute_flow_confidence`: 5 x 5 box means (cv2.filter2D with the float kernel 1 / 25, BORDER_REFLECT_101, taps row by row) of both
// components, box means of the squared deviations, var_x + var_y.  A 9 x 9 footprint per pixel, staged in LDS.  The squared deviation
// "at" a position outside the image is the one at its reflection, computed from that pixel's own (reflected) neighbourhood.
__global__ __launch_bounds__(NT) void of_flow_stats_kernel(const float* __restrict__ fx, const float* __restrict__ fy, int H, int W,
                                                           float* __restrict__ mag, float* __restrict__ var) {
    constexpr int IW = TW + 8, IH = TH + 8, DW = TW + 4, DH = TH + 4;
    __shared__ float s_f[2][IH * IW];
    __shared__ float s_d[2][DH * DW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    // rows / columns of the image that this tile holds: [oy, oy + IH) x [ox, ox + IW), shifted inwards at the far border so that every
    // reflected neighbour of a reflected position is inside it
    const int ox = of_clamp(x0 - 4, 0, W - IW > 0 ? W - IW : 0), oy = of_clamp(y0 - 4, 0, H - IH > 0 ? H - IH : 0);
    for (int i = threadIdx.x; i < IH * IW; i += NT) {
        const int ly = i / IW, lx = i - ly * IW, gy = oy + ly, gx = ox + lx;
        const bool in = gy < H && gx < W;
        s_f[0][i] = in ? fx[(size_t)gy * W + gx] : 0.0f;
        s_f[1][i] = in ? fy[(size_t)gy * W + gx] : 0.0f;
    }
    __syncthreads();
    const float kf = (float)(1.0 / 25.0);
    for (int i = threadIdx.x; i < DH * DW; i += NT) {
        const int ly = i / DW, lx = i - ly * DW;
        const int py = reflect101(y0 - 2 + ly, H), px = reflect101(x0 - 2 + lx, W);
        float ax = 0.0f, ay = 0.0f;
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = reflect101(py + dy, H) - oy;
            for (int dx = -2; dx <= 2; ++dx) {
                const int q = qy * IW + reflect101(px + dx, W) - ox;
                ax = ax + kf * s_f[0][q];
                ay = ay + kf * s_f[1][q];
            }
        }
        const int c = (py - oy) * IW + px - ox;
        const float ex = s_f[0][c] - ax, ey = s_f[1][c] - ay;
        s_d[0][i] = ex * ex;
        s_d[1][i] = ey * ey;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * TW; i += NT) {
        const int ly = i / TW, lx = i - ly * TW, gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float vx = 0.0f, vy = 0.0f;
        for (int dy = 0; dy < 5; ++dy)
            for (int dx = 0; dx < 5; ++dx) {
                const int q = (ly + dy) * DW + lx + dx;
                vx = vx + kf * s_d[0][q];
                vy = vy + kf * s_d[1][q];
            }
        const size_t o = (size_t)gy * W + gx;
        var[o] = vx + vy;
        if (mag) {
            const float a = s_f[0][(gy - oy) * IW + gx - ox], b = s_f[1][(gy - oy) * IW + gx - ox];
            mag[o] = sqrtf(a * a + b * b);
        }
    }
}

// confidence = 1 - clip(variance / (p95 + 1e-6), 0, 1); weight_map = confidence * (magnitude > threshold ? 0.5 : 1).  Both scalars are
// read from device memory: the caller takes the order statistics on the device and never waits for them.
__global__ __launch_bounds__(NT) void of_confidence_kernel(const float* __restrict__ var, const float* __restrict__ p95, const float* __restrict__ mag,
                                                           const float* __restrict__ thr, long n, float* __restrict__ conf, float* __restrict__ wmap) {
    const float max_var = p95[0] + 1e-6f;
    const float t = thr ? thr[0] : 0.0f;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        float r = var[i] / max_var;
        r = r < 0.0f ? 0.0f : (r > 1.0f ? 1.0f : r);     // NaN stays NaN, as np.clip leaves it
        const float c = 1.0f - r;
        if (conf) conf[i] = c;
        if (wmap) wmap[i] = (mag[i] > t) ? c * 0.5f : c;
    }
}

int of_cv_round(double v) { return (int)nearbyint(v); }   // round half to even (the default rounding mode)

int of_blocks(long n) {
    const long b = (n + NT - 1) / NT;
    return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

struct Level {
    int k, h, w, ksize;
    double sigma;
};

std::vector<Level> of_plan(int H, int W, int levels, double pyr_scale) {
    double scale = 1.0;
    int usable = 0;
    for (; usable < levels; ++usable) {
        scale *= pyr_scale;
        if (W * scale < 32 || H * scale < 32) break;
    }
    std::vector<Level> plan;
    for (int k = usable; k >= 0; --k) {
        scale = 1.0;
        for (int i = 0; i < k; ++i) scale *= pyr_scale;
        Level l;
        l.k = k;
        l.sigma = (1.0 / scale - 1.0) * 0.5;
        l.ksize = of_cv_round(l.sigma * 5) | 1;
        if (l.ksize < 3) l.ksize = 3;
        l.w = of_cv_round(W * scale);
        l.h = of_cv_round(H * scale);
        plan.push_back(l);
    }
    return plan;
}

// cv::getGaussianKernel(ksize, sigma, CV_32F): sigma <= 0 takes the fixed table (ksize 3 here)
BlurTaps of_blur_taps(int ksize, double sigma) {
    BlurTaps t{};
    t.r = ksize / 2;
    if (sigma <= 0 && ksize == 3) {
        t.k[0] = 0.5f;
        t.k[1] = 0.25f;
        return t;
    }
    if (sigma <= 0) sigma = ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8;
    std::vector<double> v(ksize);
    double sum = 0;
    for (int i = 0; i < ksize; ++i) {
        const double x = i - (ksize - 1) * 0.5;
        v[i] = exp(-0.5 / (sigma * sigma) * x * x);
        sum += v[i];
    }
    for (int i = 0; i <= t.r; ++i) t.k[i] = (float)(v[t.r + i] / sum);
    return t;
}

// FarnebackPrepareGaussian (n = 5): the taps in float, the Gram matrix of {1, x, y, x^2, y^2, xy} from float products summed in double, its
// inverse by Gauss-Jordan elimination in double
PolyTaps of_poly_taps(double sigma) {
    constexpr int n = POLY_N;
    PolyTaps t{};
    if (sigma < 1.1920929e-7) sigma = n * 0.3;
    float g[2 * n + 1];
    double s = 0;
    for (int x = -n; x <= n; ++x) {
        g[x + n] = (float)exp(-x * x / (2 * sigma * sigma));
        s += g[x + n];
    }
    s = 1.0 / s;
    for (int x = -n; x <= n; ++x) g[x + n] = (float)(g[x + n] * s);
    for (int k = 0; k <= n; ++k) {
        t.g[k] = g[k + n];
        t.xg[k] = (float)(k * g[k + n]);
        t.xxg[k] = (float)(k * k * g[k + n]);
    }
    double G[6][12] = {};
    for (int y = -n; y <= n; ++y)
        for (int x = -n; x <= n; ++x) {
            const float gg = g[y + n] * g[x + n];
            G[0][0] += gg;
            G[1][1] += gg * x * x;
            G[3][3] += gg * x * x * x * x;
            G[5][5] += gg * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    for (int i = 0; i < 6; ++i) G[i][6 + i] = 1.0;
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(G[r][c]) > fabs(G[piv][c])) piv = r;
        if (piv != c)
            for (int j = 0; j < 12; ++j) std::swap(G[c][j], G[piv][j]);
        const double d = 1.0 / G[c][c];
        for (int j = 0; j < 12; ++j) G[c][j] *= d;
        for (int r = 0; r < 6; ++r) {
            if (r == c) continue;
            const double f = G[r][c];
            if (f != 0.0)
                for (int j = 0; j < 12; ++j) G[r][j] -= f * G[c][j];
        }
    }
    t.ig11 = (float)G[1][7];
    t.ig03 = (float)G[0][9];
    t.ig33 = (float)G[3][9];
    t.ig55 = (float)G[5][11];
    return t;
}

constexpr int SCRATCH_PLANES = 27;   // blurred image 1, level images 2, expansions 2 x 5, matrices 2 x 5, coarser flows 2 x 2
size_t of_plane_bytes(int H, int W) { return (((size_t)H * W * sizeof(float)) + 255) / 256 * 256; }

}  // namespace
}  // namespace fw

using namespace fw;

extern "C" {

size_t fw_farneback_scratch_bytes(int height, int width, int levels) {
    if (height < 1 || width < 1 || levels < 0) return 0;
    return (size_t)SCRATCH_PLANES * of_plane_bytes(height, width) + 256;
}

int fw_farneback_flow_u8(const uint8_t* prev, const uint8_t* next, int channels, int height, int width, double pyr_scale, int levels,
                         int winsize, int iterations, int poly_n, double poly_sigma, int flags, void* scratch, float* flow_x,
                         float* flow_y, void* stream) {
    if (!prev || !next || !scratch || !flow_x || !flow_y) return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: null pointer");
    if (channels != 1 && channels != 3) return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: channels must be 1 (gray) or 3 (BGR)");
    if (height < 1 || width < 1 || (long)height * width > (1L << 30)) return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: bad frame size");
    if (poly_n != 5) return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: poly_n must be 5 (the only expansion the kernels implement)");
    if (flags != 0)
        return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: flags must be 0 (OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN are not implemented)");
    if (winsize < 3 || winsize > 2 * MAX_BOX_M + 1 || (winsize & 1) == 0)
        return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: winsize must be odd, 3 .. 31");
    if (iterations < 1 || levels < 0 || levels > 16) return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: iterations >= 1 and 0 <= levels <= 16 expected");
    if (!(pyr_scale > 0.0) || !(pyr_scale < 1.0)) return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: 0 < pyr_scale < 1 expected");
    if (!(poly_sigma >= 0.0) || poly_sigma > 100.0) return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: bad poly_sigma");
    const std::vector<Level> plan = of_plan(height, width, levels, pyr_scale);
    for (const Level& l : plan)
        if (l.ksize / 2 > MAX_BLUR_R || l.h < 1 || l.w < 1)
            return fail(FW_ERR_INVALID, "fw_farneback_flow_u8: pyramid level needs a smoothing kernel of more than 19 taps (scale below 1/8): not implemented");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const size_t pb = of_plane_bytes(height, width);
        char* base = (char*)(((uintptr_t)scratch + 255) / 256 * 256);
        auto plane = [&](int i) { return (float*)(base + (size_t)i * pb); };
        float* blurred = plane(0);
        float* I[2] = {plane(1), plane(2)};
        float* R[2] = {plane(3), plane(8)};
        float* M[2] = {plane(13), plane(18)};
        float* F[2][2] = {{plane(23), plane(24)}, {plane(25), plane(26)}};
        const uint8_t* img[2] = {prev, next};
        const PolyTaps pt = of_poly_taps(poly_sigma);
        const int m = winsize / 2;
        const float box_scale = (float)(1.0 / ((double)winsize * winsize));
        const float* pfx = nullptr;
        const float* pfy = nullptr;
        int ph = 0, pw = 0;
        const dim3 full_grid((width + TW - 1) / TW, (height + TH - 1) / TH);
        for (size_t li = 0; li < plan.size(); ++li) {
            const Level& l = plan[li];
            const bool last_level = l.k == 0;
            const dim3 grid((l.w + TW - 1) / TW, (l.h + TH - 1) / TH);
            const BlurTaps bt = of_blur_taps(l.ksize, l.sigma);
            for (int i = 0; i < 2; ++i) {
                const bool same = l.h == height && l.w == width;     // resize to the same size is a copy
                hipLaunchKernelGGL(of_blur_u8_kernel, full_grid, dim3(NT), 0, st, img[i], channels, height, width, bt, same ? I[i] : blurred);
                if (!same)
                    hipLaunchKernelGGL(of_resize_linear_kernel, dim3(of_blocks((long)l.h * l.w)), dim3(NT), 0, st, blurred, height, width, I[i], l.h,
                                       l.w, 1.0 / ((double)l.h / height), 1.0 / ((double)l.w / width));
                hipLaunchKernelGGL(of_polyexp_kernel, grid, dim3(NT), 0, st, I[i], l.h, l.w, pt, R[i]);
            }
            hipLaunchKernelGGL(of_init_matrices_kernel, dim3(of_blocks((long)l.h * l.w)), dim3(NT), 0, st, R[0], R[1], pfx, pfy, ph, pw,
                               pfx ? 1.0 / ((double)l.h / ph) : 1.0, pfx ? 1.0 / ((double)l.w / pw) : 1.0, (float)(1.0 / pyr_scale), l.h, l.w, M[0]);
            float* ofx = last_level ? flow_x : F[li & 1][0];
            float* ofy = last_level ? flow_y : F[li & 1][1];
            for (int it = 0; it < iterations; ++it) {
                const bool last = it == iterations - 1;
                hipLaunchKernelGGL(of_flow_iter_kernel, grid, dim3(NT), 0, st, M[it & 1], R[0], R[1], l.h, l.w, m, box_scale,
                                   last ? (float*)nullptr : M[(it + 1) & 1], last ? ofx : (float*)nullptr, last ? ofy : (float*)nullptr);
            }
            pfx = ofx;
            pfy = ofy;
            ph = l.h;
            pw = l.w;
        }
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_flow_stats_f32(const float* flow_x, const float* flow_y, int height, int width, float* magnitude, float* variance, void* stream) {
    if (!flow_x || !flow_y || !variance || height < 1 || width < 1) return fail(FW_ERR_INVALID, "fw_flow_stats_f32: bad argument");
    hipLaunchKernelGGL(of_flow_stats_kernel, dim3((width + TW - 1) / TW, (height + TH - 1) / TH), dim3(NT), 0, (hipStream_t)stream, flow_x,
                       flow_y, height, width, magnitude, variance);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FW_ERR_HIP, std::string("fw_flow_stats_f32: ") + hipGetErrorString(e));
    return FW_OK;
}

int fw_flow_confidence_f32(const float* variance, const float* variance_p95, const float* magnitude, const float* motion_threshold,
                           int height, int width, float* confidence, float* weight_map, void* stream) {
    if (!variance || !variance_p95 || height < 1 || width < 1 || (!confidence && !weight_map))
        return fail(FW_ERR_INVALID, "fw_flow_confidence_f32: bad argument");
    if (weight_map && (!magnitude || !motion_threshold))
        return fail(FW_ERR_INVALID, "fw_flow_confidence_f32: weight_map needs magnitude and motion_threshold");
    const long n = (long)height * width;
    hipLaunchKernelGGL(of_confidence_kernel, dim3(of_blocks(n)), dim3(NT), 0, (hipStream_t)stream, variance, variance_p95, magnitude,
                       motion_threshold, n, confidence, weight_map);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FW_ERR_HIP, std::string("fw_flow_confidence_f32: ") + hipGetErrorString(e));
    return FW_OK;
}

}  // extern "C"
