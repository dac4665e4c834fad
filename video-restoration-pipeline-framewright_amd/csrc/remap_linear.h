// cv2.remap(frame, map_x, map_y, INTER_LINEAR) on uint8 BGR, one pixel: OpenCV's 8-bit arithmetic restated once for every border
// mode (coordinates rounded to 1/32 pixel with round-half-even, 15-bit coefficients, (sum + 2^14) >> 15); cv2 parity is unpinned,
// oracle/temporal_ref.py is the contract.  Used by flow_accumulate.h (BORDER_REFLECT_101) and frame_generation.hip (BORDER_REFLECT).
// The only floating-point operation is one product, so the including file's contraction flag cannot change a result.
#pragma once
#include "stage_common.h"

namespace fw {

struct BorderReflect101 {                      // ...dcb|abcd|cba...
    __device__ __forceinline__ int operator()(int p, int len) const { return reflect101(p, len); }
};

struct BorderReflect {                         // ...cba|abc|cba..., in closed form: a map may leave the frame by any distance
    __device__ __forceinline__ int operator()(int p, int len) const {
        const int period = 2 * len;
        int m = p % period;
        if (m < 0) m += period;
        return m < len ? m : period - 1 - m;
    }
};

// out[c] = the sample of `frame` (H x W x 3) at (mx, my)
template <typename Border>
__device__ __forceinline__ void remap_linear_u8c3(const uint8_t* __restrict__ frame, int H, int W, float mx, float my, Border border, int* out) {
    const int sx = (int)rintf(mx * 32.0f), sy = (int)rintf(my * 32.0f);
    const int ix = sx >> 5, iy = sy >> 5, ax = sx & 31, ay = sy & 31;
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    const int x0 = border(ix, W), x1 = border(ix + 1, W), y0 = border(iy, H), y1 = border(iy + 1, H);
    const uint8_t* p00 = frame + ((size_t)y0 * W + x0) * 3;
    const uint8_t* p01 = frame + ((size_t)y0 * W + x1) * 3;
    const uint8_t* p10 = frame + ((size_t)y1 * W + x0) * 3;
    const uint8_t* p11 = frame + ((size_t)y1 * W + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (p00[c] * w00 + p01[c] * w01 + p10[c] * w10 + p11[c] * w11 + (1 << 14)) >> 15;
}

}  // namespace fw
