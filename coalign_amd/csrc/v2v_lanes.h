// The lane mapping and the 8-channel load / store / split helpers the glue kernels of csrc/v2v_fuse.hip and csrc/v2v_robust.hip share: a wavefront owns 16 consecutive
// pixels of one map; lane = (pixel = lane & 15, channel group = lane >> 4) and walks the 8-channel groups g, g + 4, ...  The 4 lanes of a pixel read 4 x 32 B = one
// 128-byte line of a channels-last row, the 16 lanes of a group write 16 x 16 B = 256 contiguous bytes of a SplitMap plane.
#pragma once
#include "common.h"

namespace {

constexpr int PW = 16;      // pixels per wavefront
constexpr int GL = 4;       // channel groups in flight per pixel (lanes per pixel)

// this wavefront's (map, pixel tile) and this lane's pixel of it; false: the wavefront lies beyond the last tile
struct Place { int map, pix, g0; bool live; };
__device__ __forceinline__ bool place(int maps, int HW, Place &p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = (HW + PW - 1) / PW;
    const long long t = (long long)blockIdx.x * 4 + wave;
    if (t >= (long long)maps * tiles) return false;
    p.map = (int)(t / tiles);
    const int raw = (int)(t - (long long)p.map * tiles) * PW + (lane & (PW - 1));
    p.live = raw < HW;
    p.pix = p.live ? raw : HW - 1;      // (a lane past the end reads the last pixel and stores nothing)
    p.g0 = lane / PW;
    return true;
}

__device__ __forceinline__ void load8(const float *p, float (&v)[8]) {
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ void store8(float *p, const float (&v)[8]) {
    reinterpret_cast<float4 *>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4 *>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// 8 consecutive channels (group g of a map of C16 16-channel steps) of one pixel -> the two planes of their channel half (the arithmetic of sp_pack_kernel)
template <bool STREAM = false>      // STREAM: non-temporal stores (common.h), for planes the next launch reads from another XCD anyway
__device__ __forceinline__ bool store_split8(uint4 *y, int map, int C16, int g, int HW, int pix, const float (&v)[8], bool live) {
    uint4 h, l;
    coalign::sp16_split8(v, h, l);
    bool big = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) big = big || fabsf(v[k]) > 65504.f;
    if (live) {
        const size_t base = ((size_t)((size_t)map * C16 + (g >> 1)) * 4 + (g & 1) * 2) * HW + pix;
        if (STREAM) {
            coalign::store_stream(y + base, h);
            coalign::store_stream(y + base + HW, l);
        } else {
            y[base] = h;
            y[base + HW] = l;
        }
    }
    return big && live;
}

inline unsigned blocks_of(int maps, int H, int W) {
    const long long tiles = ((long long)H * W + PW - 1) / PW;
    return (unsigned)((maps * tiles + 3) / 4);
}

}  // namespace
