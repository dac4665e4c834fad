// The remap-and-accumulate step of the classical temporal denoise, shared by fw_flow_accumulate_u8 (frame_ops.hip: weight =
// scale * map, halved above a magnitude threshold) and fw_flow_accumulate_affine_u8 (temporal_chain.hip: weight = a + b * map):
//   aligned = cv2.remap(frame, x +/- flow_x, y +/- flow_y, INTER_LINEAR, BORDER_REFLECT_101);
//   accumulated += aligned (float64) * weight;  weight_sum += weight.
// The remap is remap_linear.h's restatement of OpenCV's 8-bit INTER_LINEAR arithmetic; cv2 parity is unpinned,
// oracle/temporal_ref.py is the contract.
// Both translation units are compiled with -ffp-contract=off: value * weight rounds before it is added.
#pragma once
#include "remap_linear.h"

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
            // map = (grid +/- flow).astype(float32); the sample is remap_linear.h's
            const float mx = inverse ? (float)((double)x - (double)fx[i]) : (float)((double)x + (double)fx[i]);
            const float my = inverse ? (float)((double)y - (double)fy[i]) : (float)((double)y + (double)fy[i]);
            int s[3];
            remap_linear_u8c3(frame, H, W, mx, my, BorderReflect101(), s);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (double)s[c];
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
