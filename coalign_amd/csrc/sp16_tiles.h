// What the units that run small dense layers on a 32-pixel tile share (csrc/disco_fuse.hip, csrc/v2x_attn.hip, csrc/v2x_window.hip, csrc/v2x_ffn.hip): the LDS tile
// of sp16 pairs and the row tile of a folded projection on v_mfma_f32_32x32x16_f16 (three products per fp32 product), the weight image streamed in operand order.
#pragma once
#include "common.h"

namespace {

using coalign::floatx16;
using coalign::halfx8;

constexpr int TP = 32;                         // pixels per workgroup = columns of one matrix instruction

__host__ __device__ constexpr size_t image_bytes(int rows, int C) { return (size_t)(C / 16) * (rows / 32) * 64 * 32; }      // [C / 16 steps][rows / 32 tiles][64 lanes][8 h | 8 l] fp16
__host__ __device__ constexpr int x_row_bytes(int C) { return C * 4 + 16; }                                                // a pixel's row in the LDS tile: C / 8 groups x (8 h + 8 l) + the bank pad

// 8 values -> the tile's [8 h | 8 l] image of one channel group
__device__ __forceinline__ void store_split8(char *dst, const float (&v)[8]) {
    uint4 h, l;
    coalign::sp16_split8(v, h, l);
    *reinterpret_cast<uint4 *>(dst) = h;
    *reinterpret_cast<uint4 *>(dst + 16) = l;
}

struct Pair { halfx8 h, l; };

__device__ __forceinline__ Pair load_pair(const void *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    Pair r;
    r.h = __builtin_bit_cast(halfx8, q[0]);
    r.l = __builtin_bit_cast(halfx8, q[1]);
    return r;
}

// acc += w_h x_h, accl += w_h x_l' + w_l' x_h (the two terms that carry 2^10)
__device__ __forceinline__ void mfma3(const Pair &w, const Pair &x, floatx16 &acc, floatx16 &accl) {
    accl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w.h, x.l, accl, 0, 0, 0);
    accl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w.l, x.h, accl, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w.h, x.h, acc, 0, 0, 0);
}

// row tile `tile` of an image of `tiles` row tiles times the LDS tile's `steps` 16-channel steps (even), for the 32 pixels; bias seeds the accumulator.  Returns the
// lane's 16 values: rows 32 tile + 8 (q >> 2) + 4 half + (q & 3) of pixel lane & 31.
__device__ __forceinline__ floatx16 row_tile(const unsigned char *img, int tiles, int tile, const float *bias, int lane, const char *xrow, int steps) {
    const size_t STEP = (size_t)tiles * 64 * 32;
    const unsigned char *wp = img + ((size_t)tile * 64 + lane) * 32;
    const int h = lane >> 5;
    floatx16 acc, accl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 b = *reinterpret_cast<const float4 *>(bias + 32 * tile + 8 * i + 4 * h);
        acc[4 * i] = b.x; acc[4 * i + 1] = b.y; acc[4 * i + 2] = b.z; acc[4 * i + 3] = b.w;
        accl[4 * i] = accl[4 * i + 1] = accl[4 * i + 2] = accl[4 * i + 3] = 0.f;
    }
    Pair w0 = load_pair(wp), w1 = load_pair(wp + STEP);
    for (int s = 0; s < steps; s += 2) {
        Pair n0 = w0, n1 = w1;
        if (s + 2 < steps) {
            n0 = load_pair(wp + (size_t)(s + 2) * STEP);
            n1 = load_pair(wp + (size_t)(s + 3) * STEP);
        }
        const Pair x0 = load_pair(xrow + (2 * s + h) * 32), x1 = load_pair(xrow + (2 * s + 2 + h) * 32);
        mfma3(w0, x0, acc, accl);
        mfma3(w1, x1, acc, accl);
        w0 = n0; w1 = n1;
    }
    floatx16 r;
#pragma unroll
    for (int q = 0; q < 16; ++q) r[q] = fmaf(accl[q], coalign::kSp16LowInv, acc[q]);
    return r;
}

// sum over the G lanes that hold one pixel (G a power of two <= 32, the lanes consecutive and aligned)
__device__ __forceinline__ float pixel_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace
