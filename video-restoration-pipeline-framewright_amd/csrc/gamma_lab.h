// The per-pixel bodies of the 8-bit sRGB BGR <-> Lab transforms (cv2.COLOR_BGR2LAB / COLOR_LAB2BGR as tests/flicker_ref.py states them:
// integers over the tables of lab_tables.h plus a 256-entry sRGB decode in front and an sRGB encode, 255 thresholds, behind), shared by
// flicker.hip, where they were written, hdr.hip (the local-contrast step of the HDR conversion) and perceptual.hip (detail recovery).  Integer arithmetic throughout,
// so the floating-point flags of the including file play no part.  device_gamma_small() is defined in flicker.hip.
#pragma once
#include "lab_tables.h"
#include "stage_common.h"

namespace fw {

constexpr int LIN_MAX = 255 * 256;                              // the scale of a decoded channel = the last f(t) index
constexpr int LIN_SHIFT = F_BITS + INV_COEF_BITS - 8;           // the inverse matrix carries x 255: this leaves x 255 x 256

struct SmallTables {
    int t256[1024];             // fy, Y, a / 500, b / 200 (the inverse transform)
    uint16_t dec[256];          // sRGB decode (the forward transform)
    uint16_t thr[256];          // encode thresholds, [255] = 0xffff: above every value
    uint8_t lut[256];           // flicker.hip: the frame's map of L
};

// per device: decode[256], thresholds[256] ([255] = 0xffff) as int; made on first use (an allocation and a blocking copy)
int* device_gamma_small();

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// index into f(t) of row q: (coef . decoded + 2^19) >> 20, 0 .. 65280 (the rows sum to 2^20)
__device__ __forceinline__ int f_index(const LabFwd& k, int q, uint32_t db, uint32_t dg, uint32_t dr) {
    const unsigned long long s = (unsigned long long)(uint32_t)k.coef[3 * q] * db + (unsigned long long)(uint32_t)k.coef[3 * q + 1] * dg +
                                 (unsigned long long)(uint32_t)k.coef[3 * q + 2] * dr + (1ull << (COEF_BITS - 1));
    return (int)(s >> COEF_BITS);
}

__device__ __forceinline__ int l_of_fy(const LabFwd& k, int fy) {
    constexpr int sh = F_BITS + L_SCALE_BITS;
    return clamp255((k.l_scale * fy - k.l_offset + (1 << (sh - 1))) >> sh);
}

// packed pixel: byte 0 | byte 1 << 8 | byte 2 << 16
__device__ __forceinline__ uint32_t bgr_to_lab_px(uint32_t p, const SmallTables& s, const LabFwd& k, const int* __restrict__ cbrt_tab) {
    const uint32_t db = s.dec[p & 255u], dg = s.dec[(p >> 8) & 255u], dr = s.dec[(p >> 16) & 255u];
    const int fx = cbrt_tab[f_index(k, 0, db, dg, dr)], fy = cbrt_tab[f_index(k, 1, db, dg, dr)], fz = cbrt_tab[f_index(k, 2, db, dg, dr)];
    int a = clamp255((500 * (fx - fy) + (128 << F_BITS) + (1 << (F_BITS - 1))) >> F_BITS);
    const int b = clamp255((200 * (fy - fz) + (128 << F_BITS) + (1 << (F_BITS - 1))) >> F_BITS);
    // Keeps a and b from being fused into one v_ashr_pk_u8_i32 (shift, saturate and pack two bytes).  The compiler ORs that
    // instruction's result into a dword as if its upper 16 bits were zero; on the MI355X they were observed to hold the old
    // destination bits (pixel 2 of a group of four came back with L | a of pixel 1).
    asm volatile("" : "+v"(a));
    return (uint32_t)l_of_fy(k, fy) | (uint32_t)a << 8 | (uint32_t)b << 16;
}

// the number of thresholds <= v: the contract's encode[v]
__device__ __forceinline__ uint32_t srgb_encode(const uint16_t* thr, int v) {
    int n = 0;
#pragma unroll
    for (int step = 128; step > 0; step >>= 1)
        if ((int)thr[n + step - 1] <= v) n += step;
    return (uint32_t)n;
}

__device__ __forceinline__ uint32_t lab_to_bgr_px(uint32_t p, const SmallTables& s, const LabInv& k) {
    const int L = p & 255u, a = (p >> 8) & 255u, b = (p >> 16) & 255u;
    const long long fy = s.t256[L];
    const long long v[3] = {lab_inv_g(fy + s.t256[512 + a], k), (long long)s.t256[256 + L], lab_inv_g(fy - s.t256[768 + b], k)};
    uint32_t out = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        long long lin = (k.coef[3 * q] * v[0] + k.coef[3 * q + 1] * v[1] + k.coef[3 * q + 2] * v[2] + (1ll << (LIN_SHIFT - 1))) >> LIN_SHIFT;
        lin = lin < 0 ? 0 : lin > LIN_MAX ? LIN_MAX : lin;
        out |= srgb_encode(s.thr, (int)lin) << (8 * q);
    }
    return out;
}

__device__ __forceinline__ uint32_t l_of_px(uint32_t p, const uint16_t* dec, const LabFwd& k, const int* __restrict__ cbrt_tab) {
    return (uint32_t)l_of_fy(k, cbrt_tab[f_index(k, 1, dec[p & 255u], dec[(p >> 8) & 255u], dec[(p >> 16) & 255u])]);
}

}  // namespace fw
