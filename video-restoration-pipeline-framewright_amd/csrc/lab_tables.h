// The integer tables of the 8-bit BGR <-> Lab transforms (D65, L * 255 / 100, a + 128, b + 128), built once in float64, shared by
// nlmeans.hip (linear BGR: COLOR_LBGR2Lab / COLOR_Lab2LBGR, contract tests/nlmeans_ref.py) and flicker.hip (sRGB BGR: COLOR_BGR2LAB /
// COLOR_LAB2BGR, contract tests/flicker_ref.py, which puts a decode table in front of the same matrix and an encode behind the same
// inverse).  lab_tables() and device_lab() are defined in nlmeans.hip.
// The per-pixel bodies stay in the two files: they are not the same arithmetic.  nlmeans.hip multiplies the bytes themselves (32-bit
// sums, index = sum >> 12) and clamps the inverse to 0 .. 255; flicker.hip multiplies decoded 16-bit values (64-bit sums, index =
// sum >> 20) and keeps the inverse at 16 bits for the sRGB encode.  What they share is the tables and g^-1 below.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace fw {

constexpr int F_BITS = 16, COEF_BITS = 20, INV_COEF_BITS = 14, CBRT_STEPS = 256, CBRT_N = 255 * CBRT_STEPS + 1;
constexpr int L_SCALE_BITS = 6;

struct LabFwd {
    int coef[9];        // rows X / Xn, Y, Z / Zn over (B, G, R), each summing to 2^20
    int l_scale, l_offset;
};
struct LabInv {
    int coef[9];        // rows B, G, R over (X, Y, Z)
    int thr, c16, kinv;
};

struct LabTables {
    std::vector<int> cbrt_tab, t256;      // f(t) at t = i / 65280 (16 fractional bits); fy, Y, a / 500, b / 200 per byte
    LabFwd fwd;
    LabInv inv;
};

const LabTables& lab_tables();

// device-resident copies of the two tables: made on first use per device (an allocation and a blocking copy), then only read
struct DeviceLab {
    int* cbrt_tab = nullptr;
    int* t256 = nullptr;
};
DeviceLab device_lab();

// g^-1 of the Lab inverse, 16 fractional bits in and out: t^3 above the threshold, the linear branch below
__device__ __forceinline__ long long lab_inv_g(long long t, const LabInv& k) {
    if (t > k.thr) return (t * t * t + (1ll << (2 * F_BITS - 1))) >> (2 * F_BITS);
    return ((t - k.c16) * k.kinv + (1ll << (F_BITS - 1))) >> F_BITS;
}

}  // namespace fw
