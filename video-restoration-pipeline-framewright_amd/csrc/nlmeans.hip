// Non-local-means spatial denoise (the reference's `_apply_spatial_denoise`, temporal_denoise.py:1611-1634:
// cv2.fastNlMeansDenoisingColored(frame, None, h, h, 7, 21)) on 8-bit planes, gfx950.
//
// The contract is tests/nlmeans_ref.py (OpenCV's 8-bit algorithm as recalled; cv2 parity unpinned) and the bar is bit-exactness:
// everything behind the construction of the tables is integer arithmetic.
//
// Core kernel.  A wave owns 64 - 2 th image columns (one lane per column, th halo lanes on either side) and NLM_ROWS output rows;
// a workgroup of NLM_WAVES waves shares one LDS image of its tile plus the th + sh border, one dword per pixel (C <= 3 bytes), and
// the weight table (short: the 0.001 cut-off zeroes everything past ~6.9 h^2 C / m).  For each of the search^2 offsets a lane walks
// down its column: squared difference of its pixel and the shifted one (one LDS read), the horizontal template sum through lane
// permutes (s3 = left + own + right, s7 = s3 two to the left + own + s3 two to the right), the vertical one as a running sum over
// the last `template` rows held in registers, one table look-up, C multiply-adds into uint32 accumulators.  No barrier inside the
// offset loop; HBM traffic is one read and one write per plane.
#include "stage_common.h"
#include "lab_tables.h"

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace fw {
namespace {

constexpr int NLM_ROWS = 16;                       // output rows per wave
constexpr int NLM_WAVES = 2;
constexpr int NLM_NT = 64 * NLM_WAVES;
constexpr int NLM_MAX_SH = 20;                     // search window <= 41
constexpr int NLM_COLS = 64 + 2 * NLM_MAX_SH;      // LDS row stride in dwords: a constant, so row steps are immediate offsets
constexpr int NLM_MAX_TH = 3;                      // template window 3, 5 or 7
constexpr size_t NLM_MAX_LDS = 64 * 1024;

template <int C, int TH>
__global__ __launch_bounds__(NLM_NT) void nlmeans_kernel(const uint8_t* __restrict__ src, int H, int W, int sh, int shift,
                                                         const int* __restrict__ table, int n, uint8_t* __restrict__ dst) {
    extern __shared__ uint32_t nlm_lds[];
    constexpr int NIT = NLM_ROWS + 2 * TH;         // rows a lane walks per offset
    constexpr int XSTEP = 64 - 2 * TH;
    const int rows = NLM_WAVES * NLM_ROWS + 2 * TH + 2 * sh;
    const int cols_used = 64 + 2 * sh;
    uint32_t* pix = nlm_lds;
    int* tab = (int*)(nlm_lds + rows * NLM_COLS);  // n entries and a zero behind them: an index past the end is weight 0
    const int X0 = (int)blockIdx.x * XSTEP - TH - sh;
    const int Y0 = (int)blockIdx.y * (NLM_WAVES * NLM_ROWS) - TH - sh;
    for (int i = threadIdx.x; i < rows * cols_used; i += NLM_NT) {
        const int r = i / cols_used, c = i - r * cols_used;
        const uint8_t* p = src + ((size_t)reflect101(Y0 + r, H) * W + reflect101(X0 + c, W)) * C;
        uint32_t v = p[0];
        if (C > 1) v |= (uint32_t)p[1] << 8;
        if (C > 2) v |= (uint32_t)p[2] << 16;
        pix[r * NLM_COLS + c] = v;
    }
    for (int i = threadIdx.x; i <= n; i += NLM_NT) tab[i] = i < n ? table[i] : 0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t* own_base = pix + (wave * NLM_ROWS + sh) * NLM_COLS + lane + sh;
    uint32_t own[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) own[i] = own_base[i * NLM_COLS];
    uint32_t est[C][NLM_ROWS], wsum[NLM_ROWS];
#pragma unroll
    for (int j = 0; j < NLM_ROWS; ++j) {
        wsum[j] = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) est[c][j] = 0;
    }
    int from_left[NLM_MAX_TH], from_right[NLM_MAX_TH];   // ds_bpermute addresses: lane l reads lane l -/+ (k + 1)
#pragma unroll
    for (int k = 0; k < NLM_MAX_TH; ++k) {
        from_left[k] = ((lane - k - 1) & 63) << 2;
        from_right[k] = ((lane + k + 1) & 63) << 2;
    }

    for (int oy = -sh; oy <= sh; ++oy) {
        const uint32_t* row_base = own_base + oy * NLM_COLS;
        for (int ox = -sh; ox <= sh; ++ox) {
            const uint32_t* nbp = row_base + ox;
            uint32_t nb[NIT];
            int hs[NIT];
            int run = 0;
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                nb[i] = nbp[i * NLM_COLS];
                int d2 = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int d = (int)((own[i] >> (8 * c)) & 255u) - (int)((nb[i] >> (8 * c)) & 255u);
                    d2 += __mul24(d, d);
                }
                int h;
                if (TH == 3) {
                    const int s3 = d2 + __builtin_amdgcn_ds_bpermute(from_left[0], d2) + __builtin_amdgcn_ds_bpermute(from_right[0], d2);
                    h = d2 + __builtin_amdgcn_ds_bpermute(from_left[1], s3) + __builtin_amdgcn_ds_bpermute(from_right[1], s3);
                } else {
                    h = d2;
#pragma unroll
                    for (int k = 0; k < TH; ++k)
                        h += __builtin_amdgcn_ds_bpermute(from_left[k], d2) + __builtin_amdgcn_ds_bpermute(from_right[k], d2);
                }
                hs[i] = h;
                run += h;
                if (i >= 2 * TH + 1) run -= hs[i - 2 * TH - 1];
                if (i >= 2 * TH) {                  // rows i - 2 th .. i are in: the patch distance of the pixel in row i - th
                    const int j = i - 2 * TH;
                    const int idx = min(run >> shift, n);
                    const uint32_t w = (uint32_t)tab[idx];
                    const uint32_t q = nb[i - TH];
                    wsum[j] += w;
#pragma unroll
                    for (int c = 0; c < C; ++c) est[c][j] += __umul24(w, (q >> (8 * c)) & 255u);
                }
            }
        }
    }

    const int x = (int)blockIdx.x * XSTEP + lane - TH;
    if (lane >= TH && lane < 64 - TH && x < W) {
        const int y0 = (int)blockIdx.y * (NLM_WAVES * NLM_ROWS) + wave * NLM_ROWS;
#pragma unroll
        for (int j = 0; j < NLM_ROWS; ++j) {
            const int y = y0 + j;
            if (y < H) {
                const uint32_t ws = wsum[j];       // >= the centre offset's weight (distance 0): never 0
                uint8_t* o = dst + ((size_t)y * W + x) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = (uint8_t)((est[c][j] + (ws >> 1)) / ws);
            }
        }
    }
}

// ---- 8-bit linear BGR <-> Lab (COLOR_LBGR2Lab / COLOR_Lab2LBGR), integers over tables built once in float64 ----
// constants, LabFwd, LabInv, LabTables and lab_tables(): lab_tables.h (shared with flicker.hip)
__global__ __launch_bounds__(256) void bgr_to_lab_kernel(const uint8_t* __restrict__ bgr, long n, LabFwd k, const int* __restrict__ cbrt_tab,
                                                         uint8_t* __restrict__ Lp, uint8_t* __restrict__ abp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = bgr[3 * i], g = bgr[3 * i + 1], r = bgr[3 * i + 2];
    int f[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
        f[q] = cbrt_tab[(k.coef[3 * q] * b + k.coef[3 * q + 1] * g + k.coef[3 * q + 2] * r + (1 << (COEF_BITS - 9))) >> (COEF_BITS - 8)];
    constexpr int sh = F_BITS + L_SCALE_BITS;
    const int L = (k.l_scale * f[1] - k.l_offset + (1 << (sh - 1))) >> sh;
    const int a = (500 * (f[0] - f[1]) + (128 << F_BITS) + (1 << (F_BITS - 1))) >> F_BITS;
    const int bb = (200 * (f[1] - f[2]) + (128 << F_BITS) + (1 << (F_BITS - 1))) >> F_BITS;
    Lp[i] = (uint8_t)min(max(L, 0), 255);
    abp[2 * i] = (uint8_t)min(max(a, 0), 255);
    abp[2 * i + 1] = (uint8_t)min(max(bb, 0), 255);
}

__global__ __launch_bounds__(256) void lab_to_bgr_kernel(const uint8_t* __restrict__ Lp, const uint8_t* __restrict__ abp, long n, LabInv k,
                                                         const int* __restrict__ t256 /* fy, yl, ax, bz */, uint8_t* __restrict__ bgr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int L = Lp[i], a = abp[2 * i], b = abp[2 * i + 1];
    const long long fy = t256[L];
    const long long v[3] = {lab_inv_g(fy + t256[512 + a], k), (long long)t256[256 + L], lab_inv_g(fy - t256[768 + b], k)};
    constexpr int sh = F_BITS + INV_COEF_BITS;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const long long s = (k.coef[3 * q] * v[0] + k.coef[3 * q + 1] * v[1] + k.coef[3 * q + 2] * v[2] + (1ll << (sh - 1))) >> sh;
        bgr[3 * i + q] = (uint8_t)(s < 0 ? 0 : s > 255 ? 255 : s);
    }
}

// ---- the weight table (host, float64) ----
struct TableShape {
    int mult, shift, n;
    double m;
};

bool table_shape(int channels, int template_window, int search_window, TableShape* out) {
    if (channels < 1 || channels > 3 || template_window < 1 || search_window < 1 || !(template_window & 1) || !(search_window & 1) ||
        template_window > 255 || search_window > 1023)
        return false;
    const long ss = (long)search_window * search_window * 255;
    out->mult = (int)std::min<long>(2147483647l / ss, 2147483647l);
    out->shift = 0;
    while ((1 << out->shift) < template_window * template_window) ++out->shift;
    out->m = (double)(1 << out->shift) / (double)(template_window * template_window);
    out->n = (int)(65025.0 * channels / out->m + 1);
    return true;
}

// truncated behind its last non-zero entry (the weights fall monotonically: the first zeroed entry ends it)
std::vector<int> weight_table(double h, int channels, const TableShape& s) {
    std::vector<int> t;
    const double den = h * h * channels;
    for (int i = 0; i < s.n; ++i) {
        const double v = std::nearbyint(s.mult * std::exp(-(i * s.m) / den));
        if (v < 0.001 * s.mult) break;
        t.push_back((int)v);
    }
    return t;
}

// ---- device-resident copies: made on first use (an allocation and a blocking copy), then only read ----
struct DeviceTable {
    int* ptr = nullptr;
    int n = 0;
};
std::mutex g_mutex;
std::map<int, DeviceLab> g_lab;
std::map<std::tuple<int, double, int, int, int>, DeviceTable> g_tables;
constexpr size_t MAX_CACHED_TABLES = 64;

int* upload(const std::vector<int>& v) {
    int* d = nullptr;
    FW_HIP_CHECK(hipMalloc((void**)&d, v.size() * sizeof(int)));
    FW_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return d;
}

// a table of more than max_n entries is not uploaded: {nullptr, its length}
DeviceTable device_weight_table(double h, int channels, int template_window, int search_window, const TableShape& s, size_t max_n) {
    int dev = 0;
    FW_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_mutex);
    const auto key = std::make_tuple(dev, h, channels, template_window, search_window);
    auto it = g_tables.find(key);
    if (it != g_tables.end()) return it->second;
    if (g_tables.size() >= MAX_CACHED_TABLES) {               // hipFree waits for the device: nothing in flight reads them afterwards
        for (auto& kv : g_tables) (void)hipFree(kv.second.ptr);
        g_tables.clear();
    }
    const std::vector<int> t = weight_table(h, channels, s);
    DeviceTable d;
    d.n = (int)t.size();
    if (t.empty() || t.size() > max_n) return d;
    d.ptr = upload(t);
    g_tables[key] = d;
    return d;
}

size_t plane_bytes(size_t n) { return (n + 255) / 256 * 256; }

// argument check shared by the two device entries; empty = fine
std::string check_args(const char* fn, int channels, int H, int W, double h, int template_window, int search_window) {
    const std::string p = std::string(fn) + ": ";
    if (channels < 1 || channels > 3) return p + "channels must be 1, 2 or 3";
    if (H < 2 || W < 2) return p + "a side of 1 px (or less) cannot be extended by reflection";
    if ((long)H * W > (1l << 30)) return p + "bad frame size";
    if (!(h > 0.0) || !(h <= 1000.0)) return p + "h must be positive";
    if (template_window < 3 || template_window > 2 * NLM_MAX_TH + 1 || !(template_window & 1))
        return p + "template window must be 3, 5 or 7 (even sizes are rejected, not forced odd)";
    if (search_window < 3 || search_window > 2 * NLM_MAX_SH + 1 || !(search_window & 1))
        return p + "search window must be odd, 3 .. 41 (even sizes are rejected, not forced odd)";
    return "";
}

template <int C>
void launch_core_th(int th, dim3 grid, size_t lds, hipStream_t st, const uint8_t* src, int H, int W, int sh, int shift, const int* table,
                    int n, uint8_t* dst) {
    if (th == 1) hipLaunchKernelGGL((nlmeans_kernel<C, 1>), grid, dim3(NLM_NT), lds, st, src, H, W, sh, shift, table, n, dst);
    else if (th == 2) hipLaunchKernelGGL((nlmeans_kernel<C, 2>), grid, dim3(NLM_NT), lds, st, src, H, W, sh, shift, table, n, dst);
    else hipLaunchKernelGGL((nlmeans_kernel<C, 3>), grid, dim3(NLM_NT), lds, st, src, H, W, sh, shift, table, n, dst);
}

// arguments already checked; everything that can refuse a launch happens in plan_core (throws fw::Error), run_core only launches
struct CorePlan {
    DeviceTable table;
    int th, sh, shift;
    size_t lds;
};

CorePlan plan_core(const char* fn, int channels, double h, int template_window, int search_window) {
    TableShape s;
    if (!table_shape(channels, template_window, search_window, &s)) throw Error(FW_ERR_INVALID, std::string(fn) + ": bad window");
    CorePlan p;
    p.th = template_window / 2;
    p.sh = search_window / 2;
    p.shift = s.shift;
    const size_t tile = (size_t)(NLM_WAVES * NLM_ROWS + 2 * p.th + 2 * p.sh) * NLM_COLS;
    p.table = device_weight_table(h, channels, template_window, search_window, s, NLM_MAX_LDS / sizeof(int) - tile - 1);
    p.lds = (tile + p.table.n + 1) * sizeof(int);
    if (!p.table.ptr)
        throw Error(FW_ERR_INVALID, std::string(fn) + ": h is too large for this search window (the weight table of " +
                                        std::to_string(p.table.n) + " entries and the tile do not fit the kernel's 64 KiB of LDS)");
    return p;
}

void run_core(const CorePlan& p, const uint8_t* src, int channels, int H, int W, uint8_t* dst, hipStream_t st) {
    const dim3 grid((W + 64 - 2 * p.th - 1) / (64 - 2 * p.th), (H + NLM_WAVES * NLM_ROWS - 1) / (NLM_WAVES * NLM_ROWS));
    if (channels == 1) launch_core_th<1>(p.th, grid, p.lds, st, src, H, W, p.sh, p.shift, p.table.ptr, p.table.n, dst);
    else if (channels == 2) launch_core_th<2>(p.th, grid, p.lds, st, src, H, W, p.sh, p.shift, p.table.ptr, p.table.n, dst);
    else launch_core_th<3>(p.th, grid, p.lds, st, src, H, W, p.sh, p.shift, p.table.ptr, p.table.n, dst);
}

}  // namespace

// ---- declared in lab_tables.h ----
const LabTables& lab_tables() {
    static const LabTables t = [] {
        LabTables r;
        const double XN = 0.950456, ZN = 1.088754, T0 = 0.008856;
        const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
        const double MI[3][3] = {{3.240479, -1.53715, -0.498535}, {-0.969256, 1.875991, 0.041556}, {0.055648, -0.204043, 1.057311}};
        const double wp[3] = {XN, 1.0, ZN};
        const double f_thresh = 7.787 * T0 + 16.0 / 116.0, l_thresh = T0 * 903.3;
        r.cbrt_tab.resize(CBRT_N);
        for (int i = 0; i < CBRT_N; ++i) {
            const double x = (double)i / (double)(CBRT_N - 1);
            const double f = x > T0 ? std::cbrt(x) : 7.787 * x + 16.0 / 116.0;
            r.cbrt_tab[i] = (int)std::nearbyint((double)(1 << F_BITS) * f);
        }
        for (int q = 0; q < 3; ++q) {
            double row[3];
            for (int j = 0; j < 3; ++j) row[j] = M[q][j] / wp[q];
            const double s = (row[0] + row[1]) + row[2];
            long c[3], sum = 0;
            int big = 0;
            for (int j = 0; j < 3; ++j) {                     // (B, G, R) order: column 2 - j of the RGB matrix
                c[j] = (long)std::nearbyint(row[2 - j] / s * (double)(1 << COEF_BITS));
                sum += c[j];
                if (c[j] > c[big]) big = j;
            }
            c[big] += (1l << COEF_BITS) - sum;
            for (int j = 0; j < 3; ++j) r.fwd.coef[3 * q + j] = (int)c[j];
        }
        r.fwd.l_scale = (int)std::nearbyint(116.0 * 2.55 * (double)(1 << L_SCALE_BITS));
        r.fwd.l_offset = (int)std::nearbyint(16.0 * 2.55 * (double)(1 << (F_BITS + L_SCALE_BITS)));
        r.t256.resize(1024);
        for (int i = 0; i < 256; ++i) {
            const double L = (double)i * 100.0 / 255.0;
            const double y_low = L / 903.3;
            const double fy = L <= l_thresh ? 7.787 * y_low + 16.0 / 116.0 : (L + 16.0) / 116.0;
            const double yl = L <= l_thresh ? y_low : fy * fy * fy;
            const double ab = (double)i - 128.0;
            r.t256[i] = (int)std::nearbyint(fy * (double)(1 << F_BITS));
            r.t256[256 + i] = (int)std::nearbyint(yl * (double)(1 << F_BITS));
            r.t256[512 + i] = (int)std::nearbyint(ab / 500.0 * (double)(1 << F_BITS));
            r.t256[768 + i] = (int)std::nearbyint(ab / 200.0 * (double)(1 << F_BITS));
        }
        for (int q = 0; q < 3; ++q)                           // rows B, G, R
            for (int j = 0; j < 3; ++j)
                r.inv.coef[3 * q + j] = (int)std::nearbyint(MI[2 - q][j] * wp[j] * 255.0 * (double)(1 << INV_COEF_BITS));
        r.inv.thr = (int)std::nearbyint(f_thresh * (double)(1 << F_BITS));
        r.inv.c16 = (int)std::nearbyint(16.0 / 116.0 * (double)(1 << F_BITS));
        r.inv.kinv = (int)std::nearbyint((double)(1 << F_BITS) / 7.787);
        return r;
    }();
    return t;
}

DeviceLab device_lab() {
    int dev = 0;
    FW_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_mutex);
    DeviceLab& d = g_lab[dev];
    if (!d.cbrt_tab) d.cbrt_tab = upload(lab_tables().cbrt_tab);
    if (!d.t256) d.t256 = upload(lab_tables().t256);
    return d;
}

}  // namespace fw

using namespace fw;

extern "C" {

size_t fw_nlmeans_scratch_bytes(int height, int width, int search_window) {
    if (height < 2 || width < 2 || (long)height * width > (1l << 30) || search_window < 3 || search_window > 2 * NLM_MAX_SH + 1 ||
        !(search_window & 1))
        return 0;
    const size_t n = (size_t)height * width;
    return 2 * (plane_bytes(n) + plane_bytes(2 * n)) + 256;     // L and ab planes, in and out
}

int fw_nlmeans_weight_table(double h, int channels, int template_window, int search_window, int32_t* out, int capacity) {
    TableShape s;
    if (!(h > 0.0) || !table_shape(channels, template_window, search_window, &s)) {
        last_error_ref() = "fw_nlmeans_weight_table: h > 0, channels 1 .. 3 and odd windows expected";
        return 0;
    }
    const std::vector<int> t = weight_table(h, channels, s);
    if (out) {
        if (capacity < (int)t.size()) {
            last_error_ref() = "fw_nlmeans_weight_table: capacity " + std::to_string(capacity) + " < " + std::to_string(t.size()) + " entries";
            return 0;
        }
        memcpy(out, t.data(), t.size() * sizeof(int));
    }
    return (int)t.size();
}

int fw_nlmeans_lab_tables(int which, int32_t* out, int capacity) {
    const LabTables& t = lab_tables();
    std::vector<int> v;
    if (which == 0) v = t.cbrt_tab;
    else if (which == 1) v.assign(t.fwd.coef, t.fwd.coef + 9);
    else if (which == 2) v = t.t256;
    else if (which == 3) {
        v.assign(t.inv.coef, t.inv.coef + 9);
        v.push_back(t.inv.thr);
        v.push_back(t.inv.c16);
        v.push_back(t.inv.kinv);
    } else {
        last_error_ref() = "fw_nlmeans_lab_tables: which must be 0 .. 3";
        return 0;
    }
    if (out) {
        if (capacity < (int)v.size()) {
            last_error_ref() = "fw_nlmeans_lab_tables: capacity too small";
            return 0;
        }
        memcpy(out, v.data(), v.size() * sizeof(int));
    }
    return (int)v.size();
}

int fw_nlmeans_u8(const uint8_t* src, int channels, int height, int width, double h, int template_window, int search_window, void* scratch,
                  uint8_t* dst, void* stream) {
    (void)scratch;                                             // the whole neighbourhood lives in LDS: the core needs none
    if (!src || !dst) return fail(FW_ERR_INVALID, "fw_nlmeans_u8: null pointer");
    if (src == dst) return fail(FW_ERR_INVALID, "fw_nlmeans_u8: src and dst must differ (every output reads a 27 x 27 neighbourhood)");
    const std::string bad = check_args("fw_nlmeans_u8", channels, height, width, h, template_window, search_window);
    if (!bad.empty()) return fail(FW_ERR_INVALID, bad);
    return guarded([&] {
        const CorePlan p = plan_core("fw_nlmeans_u8", channels, h, template_window, search_window);
        run_core(p, src, channels, height, width, dst, (hipStream_t)stream);
        FW_HIP_CHECK(hipGetLastError());
    });
}

int fw_nlmeans_colored_u8(const uint8_t* src_bgr, int height, int width, double h, double h_color, int template_window, int search_window,
                          void* scratch, uint8_t* dst_bgr, void* stream) {
    if (!src_bgr || !dst_bgr || !scratch) return fail(FW_ERR_INVALID, "fw_nlmeans_colored_u8: null pointer");
    std::string bad = check_args("fw_nlmeans_colored_u8", 1, height, width, h, template_window, search_window);
    if (bad.empty()) bad = check_args("fw_nlmeans_colored_u8", 2, height, width, h_color, template_window, search_window);
    if (!bad.empty()) return fail(FW_ERR_INVALID, bad);
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        const CorePlan pl = plan_core("fw_nlmeans_colored_u8", 1, h, template_window, search_window);
        const CorePlan pc = plan_core("fw_nlmeans_colored_u8", 2, h_color, template_window, search_window);
        const DeviceLab lab = device_lab();
        const LabTables& t = lab_tables();
        const size_t n = (size_t)height * width;
        uint8_t* base = (uint8_t*)(((uintptr_t)scratch + 255) / 256 * 256);
        uint8_t* L = base;
        uint8_t* ab = L + plane_bytes(n);
        uint8_t* Ld = ab + plane_bytes(2 * n);
        uint8_t* abd = Ld + plane_bytes(n);
        const dim3 grid((unsigned)((n + 255) / 256));
        hipLaunchKernelGGL(bgr_to_lab_kernel, grid, dim3(256), 0, st, src_bgr, (long)n, t.fwd, lab.cbrt_tab, L, ab);
        run_core(pl, L, 1, height, width, Ld, st);
        run_core(pc, ab, 2, height, width, abd, st);
        hipLaunchKernelGGL(lab_to_bgr_kernel, grid, dim3(256), 0, st, Ld, abd, (long)n, t.inv, lab.t256, dst_bgr);
        FW_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
