// The remap-and-accumulate step of the classical temporal denoise, shared by fw_flow_accumulate_u8 (frame_ops.hip: weight =
// scale * map, halved above a magnitude threshold) and fw_flow_accumulate_affine_u8 (temporal_chain.hip: weight = a + b * map):
//   aligned = cv2.remap(frame, x +/- flow_x, y +/- flow_y, INTER_LINEAR, BORDER_REFLECT_101);
//   accumulated += aligned (float64) * weight;  weight_sum += weight.
// The remap restates OpenCV's 8-bit INTER_LINEAR arithmetic (coordinates rounded to 1/32 pixel with round-half-even, 15-bit
// coefficients, (sum + 2^14) >> 15); cv2 parity is unpinned, oracle/temporal_ref.py is the contract.
// Both translation units are compiled with -ffp-contract=off: value * weight rounds before it is added.
#pragma once
#include "stage_common.h"

namespace fw {

// One grid-stride pass over the H x W pixels; weight(i) is the float64 weight of pixel i.  fx == NULL: the frame as it is.
template <typename WeightFn>
__device__ __forceinline__ void flow_accumulate_pixels(const uint8_t* __restrict__ frame, const float* __restrict__ fx,
                                                       const float* __restrict__ fy, int inverse, int H, int W, double* acc,
                                                       double* wsum, WeightFn weight) {
    const long n = (long)H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        double v[3];
        if (fx) {
            // map = (grid +/- flow).astype(float32); cv2.remap fixed-point: round(map * 32), 5 fractional bits
            const float mx = inverse ? (float)((double)x - (double)fx[i]) : (float)((double)x + (double)fx[i]);
            const float my = inverse ? (float)((double)y - (double)fy[i]) : (float)((double)y + (double)fy[i]);
            const int sx = (int)rintf(mx * 32.0f), sy = (int)rintf(my * 32.0f);
            const int ix = sx >> 5, iy = sy >> 5, ax = sx & 31, ay = sy & 31;
            const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
            const int x0 = reflect101(ix, W), x1 = reflect101(ix + 1, W), y0 = reflect101(iy, H), y1 = reflect101(iy + 1, H);
            const uint8_t* p00 = frame + ((size_t)y0 * W + x0) * 3;
            const uint8_t* p01 = frame + ((size_t)y0 * W + x1) * 3;
            const uint8_t* p10 = frame + ((size_t)y1 * W + x0) * 3;
            const uint8_t* p11 = frame + ((size_t)y1 * W + x1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[c] = (double)((p00[c] * w00 + p01[c] * w01 + p10[c] * w10 + p11[c] * w11 + (1 << 14)) >> 15);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (double)frame[(size_t)i * 3 + c];
        }
        const double w = weight(i);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[(size_t)i * 3 + c] += v[c] * w;
        wsum[i] += w;
    }
}

}  // namespace fw
