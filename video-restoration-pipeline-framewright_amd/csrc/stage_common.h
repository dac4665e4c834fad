// Scaffolding shared by the frame-stage files (scene_cuts, dedup_hash, optical_flow, nlmeans, temporal_chain, flicker, color_lut,
// deinterlace, vhs, hdr, qp_artifacts, frame_generation, temporal_consistency, perceptual .hip, and frame_ops.hip for the device helpers and for the C entries of its own launchers): the status / last-error mapping of the C-ABI (fw_status.h:
// fail, invalid, hip_status, guarded), the 64-lane reductions, the small integer device helpers every stage restated, and the host
// checks of a call's frames.  A new stage includes this header and declares none of these again.
// The translation units that include it differ in their floating-point flags, so nothing here is floating-point arithmetic whose
// contraction could matter: the reductions only add or compare what they are given, the rest is integer.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "fw_status.h"

namespace fw {

// ---- device: reductions over the 64 lanes of a wave -----------------------------------------------------------------------------
// Butterfly: every lane ends with the result.  Lane 0 adds the same partial sums in the same pairing as a __shfl_down tree would
// ((l0 + l32) + (l16 + l48) ...), so a float64 sum that only lane 0 stores (scene_cuts.hip) is bit for bit what that tree gave.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

// ---- device: integer helpers ----------------------------------------------------------------------------------------------------
// The aligned word at `p`, of which only the bytes inside [lo, hi) are read: one load when the word lies inside, else its bytes.
__device__ __forceinline__ uint32_t load_word_inside(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p + k >= lo && p + k < hi) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

// cv2.cvtColor(BGR2GRAY) on uint8: 14-bit weights, rounded; C == 1: the byte is the gray value
template <int C>
__device__ __forceinline__ int gray_bgr(const uint8_t* p) {
    if constexpr (C == 1) return p[0];
    else return (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14;
}

// BORDER_REFLECT_101 for any p, reflected as often as it takes; a side of one pixel is that pixel
__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - p - 2;
    return p;
}

// the splitmix64 finaliser: the counter-based noise of qp_artifacts.hip and frame_generation.hip is
// table[mix64(key + element) >> 48], with tests/qp_artifact_ref.py's host-mixed key
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- host: the frames of a call --------------------------------------------------------------------------------------------------
constexpr int MAX_FRAME_SIDE = 16384;

inline int check_side_and_channels(const char* fn, int H, int W, int C) {
    if (H < 1 || H > MAX_FRAME_SIDE || W < 1 || W > MAX_FRAME_SIDE) return invalid(fn, "1 .. 16384 pixels a side expected");
    if (C != 1 && C != 3) return invalid(fn, "1 (gray) or 3 (BGR) channels expected");
    return FW_OK;
}

// a host table of n frame pointers, none of them null; cap = 0: any n >= 1, else 1 .. cap frames
inline int check_pointer_table(const char* fn, const void* const* table, int n, int cap) {
    if (!table) return invalid(fn, "null pointer");
    if (n < 1 || (cap && n > cap)) return invalid(fn, cap ? "1 .. " + std::to_string(cap) + " frames a call expected" : "at least one frame expected");
    for (int i = 0; i < n; ++i)
        if (!table[i]) return invalid(fn, "null pointer");
    return FW_OK;
}

// true when a destination (kind 0) of the call overlaps a source (kind 1) of the call, of its own frame or of another: all frames
// are `bytes` long, so after sorting the start addresses a destination overlaps a source exactly when one follows the other within
// `bytes`.  marks = {start address, kind}; sorted in place.
using FrameMarks = std::vector<std::pair<uintptr_t, int>>;
inline bool frames_overlap(FrameMarks& marks, size_t bytes) {
    std::sort(marks.begin(), marks.end());
    uintptr_t last[2] = {0, 0};                                      // the latest start seen of a destination (0) / a source (1)
    bool seen[2] = {false, false};
    for (const auto& m : marks) {
        const int other = 1 - m.second;
        if (seen[other] && m.first - last[other] < bytes) return true;
        last[m.second] = m.first, seen[m.second] = true;
    }
    return false;
}

}  // namespace fw
