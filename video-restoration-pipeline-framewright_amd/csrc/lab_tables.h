// The integer tables of the 8-bit BGR <-> Lab transforms (D65, L * 255 / 100, a + 128, b + 128), built once in float64, shared by
// nlmeans.hip (linear BGR: COLOR_LBGR2Lab / COLOR_Lab2LBGR, contract tests/nlmeans_ref.py) and flicker.hip (sRGB BGR: COLOR_BGR2LAB /
// COLOR_LAB2BGR, contract tests/flicker_ref.py, which puts a decode table in front of the same matrix and an encode behind the same
// inverse).  lab_tables() and device_lab() are defined in nlmeans.hip.
#pragma once
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

}  // namespace fw
