// cv2.addWeighted(a, alpha, b, beta, 0) on one uint8 value, as fw_add_weighted_u8 defines it (tests/temporal_chain_ref.add_weighted):
// float32 weights, both products and the sum rounded to float32, the result rounded half to even and saturated.  The including file
// is compiled with -ffp-contract=off (temporal_chain.hip, frame_generation.hip, perceptual.hip): a fused a * alpha + b * beta would round twice, not
// three times.
#pragma once
#include <stdint.h>

namespace fw {

__device__ __forceinline__ uint32_t aw_byte(uint32_t a, float alpha, uint32_t b, float beta) {
    const float t = (float)a * alpha + (float)b * beta;       // three roundings (no contraction in the including file)
    return (uint32_t)fminf(fmaxf(rintf(t), 0.0f), 255.0f);     // round half to even, saturate
}

}  // namespace fw
