// The saturation step on one 8-bit BGR pixel, as tests/hdr_ref.adjust_saturation_u8 states it: cv2's integer BGR -> HSV (hue 0 .. 179),
// s = trunc(clip(s * boost, 0, 255)) in float32, cv2's float32 HSV -> BGR.  Written in hdr.hip, shared with perceptual.hip (the colour
// step of the perceptual tuner).  Every float operation rounds once: the including file is compiled with contraction off.
#pragma once
#include <stdint.h>

#pragma clang fp contract(off)

namespace fw {

// numpy's clip: the bound where the value is not beyond it, so -0.0 becomes the bound's +0.0
__device__ __forceinline__ float clipf(float x, float lo, float hi) {
    const float t = x > lo ? x : lo;
    return t < hi ? t : hi;
}

// cv2's sector table {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}: two bits per (sector, channel)
constexpr uint64_t sector_bits() {
    const int t[18] = {1, 3, 0, 1, 0, 2, 3, 0, 1, 0, 2, 1, 0, 1, 3, 2, 1, 0};
    uint64_t v = 0;
    for (int i = 0; i < 18; ++i) v |= (uint64_t)t[i] << (2 * i);
    return v;
}

// packed pixel b | g << 8 | r << 16.  div: sdiv[256] = round((255 << 12) / i), then hdiv[256] = round((180 << 12) / (6 i))
__device__ __forceinline__ uint32_t saturate_px(uint32_t q, const int* div, float boost, float hue_scale) {
    const int b = q & 255u, g = (q >> 8) & 255u, r = (q >> 16) & 255u;
    const int v = max(max(b, g), r), diff = v - min(min(b, g), r);
    const int s = (diff * div[v] + 2048) >> 12;
    int h = v == r ? g - b : v == g ? b - r + 2 * diff : r - g + 4 * diff;
    h = (h * div[256 + diff] + 2048) >> 12;
    if (h < 0) h += 180;
    const int s2 = (int)clipf((float)s * boost, 0.0f, 255.0f);
    const float hh = (float)(h & 255) * hue_scale, ss = __fdiv_rn((float)s2, 255.0f), vv = __fdiv_rn((float)v, 255.0f);
    const float sec = floorf(hh), fr = hh - sec;
    const int sector = ((int)sec) % 6;
    const float t0 = vv, t1 = vv * (1.0f - ss), t2 = vv * (1.0f - ss * fr), t3 = vv * (1.0f - ss * (1.0f - fr));
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int pick = (int)((sector_bits() >> (2 * (3 * sector + c))) & 3u);
        const float x = pick == 0 ? t0 : pick == 1 ? t1 : pick == 2 ? t2 : t3;
        out |= (uint32_t)min(max(__float2int_rn(x * 255.0f), 0), 255) << (8 * c);
    }
    return out;
}

}  // namespace fw
