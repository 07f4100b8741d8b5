// Lane helpers of the channels-last fusion kernels (warp_fuse_nhwc.hip, w2comm.hip): LPP = C / 8 lanes share a pixel, 8 channels per lane.  Both kernels reduce a
// pixel's scores and hand an agent's taps round with the same instructions, so that their results agree bit for bit.
#pragma once
#include "common.h"
#include "warp_taps.h"

namespace {

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// sum over the LPP lanes that share a pixel (aligned groups of 8 / 16 / 32 lanes); every lane of the group gets the same value
template <int LPP>
__device__ __forceinline__ float group_sum(float v) {
    v += dpp<0xB1>(v);                         // quad_perm [1, 0, 3, 2]: xor 1
    v += dpp<0x4E>(v);                         // quad_perm [2, 3, 0, 1]: xor 2
    v += dpp<0x141>(v);                        // row_half_mirror: lane i <- 7 - i of its 8-lane group (both quads now hold their sums)
    if constexpr (LPP >= 16) v += dpp<0x140>(v);   // row_mirror: lane i <- 15 - i
    if constexpr (LPP >= 32) v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (16 << 10) | 0x1f));
    return v;
}

// Round 4: the LPP >= 8 lanes of a pixel used to compute the SAME taps for every agent (float64 grid + clamps: ~60 VALU instructions per agent and lane, a
// third of the kernel's instructions, and the kernel is half issue-bound).  Now lane li of a pixel computes the taps of agent li once (N <= 8 <= LPP), and
// agent n's taps reach the pixel's other lanes through the LDS crossbar: ds_swizzle in bit-mask mode, new lane = (lane & ~(LPP - 1)) | n inside each half.
template <int LPP, int N>
__device__ __forceinline__ int from_lane(int v) {
    return __builtin_amdgcn_ds_swizzle(v, ((~(LPP - 1)) & 0x1f) | (N << 5));
}
template <int LPP>
__device__ __forceinline__ int from_lane_n(int v, int n) {          // n is a constant after unrolling: the switch folds
    switch (n) {
        case 0: return from_lane<LPP, 0>(v);
        case 1: return from_lane<LPP, 1>(v);
        case 2: return from_lane<LPP, 2>(v);
        case 3: return from_lane<LPP, 3>(v);
        case 4: return from_lane<LPP, 4>(v);
        case 5: return from_lane<LPP, 5>(v);
        case 6: return from_lane<LPP, 6>(v);
        default: return from_lane<LPP, 7>(v);
    }
}
template <int LPP>
__device__ __forceinline__ Taps taps_of_agent(const Taps &mine, int n) {
    Taps t;
    t.o00 = from_lane_n<LPP>(mine.o00, n); t.o01 = from_lane_n<LPP>(mine.o01, n); t.o10 = from_lane_n<LPP>(mine.o10, n); t.o11 = from_lane_n<LPP>(mine.o11, n);
    t.w00 = __builtin_bit_cast(float, from_lane_n<LPP>(__builtin_bit_cast(int, mine.w00), n));
    t.w01 = __builtin_bit_cast(float, from_lane_n<LPP>(__builtin_bit_cast(int, mine.w01), n));
    t.w10 = __builtin_bit_cast(float, from_lane_n<LPP>(__builtin_bit_cast(int, mine.w10), n));
    t.w11 = __builtin_bit_cast(float, from_lane_n<LPP>(__builtin_bit_cast(int, mine.w11), n));
    return t;
}

}  // namespace
