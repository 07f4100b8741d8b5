// The bilinear taps of the pose-aware warp on CHANNELS-LAST maps, shared by warp_fuse_nhwc.hip and disco_fuse.hip so that both kernels warp with the same
// instructions in the same order (warp_affine_simple, torch_transformation_utils.py:322-331: F.affine_grid on a float64 theta -> .to(float32) -> F.grid_sample,
// bilinear, zero padding, align_corners=False).
#pragma once
#include "common.h"

namespace {

struct Taps {
    int o00, o01, o10, o11;                // element offsets of the four (clamped) taps inside the agent's plane (channel 0 of the pixel)
    float w00, w01, w10, w11;              // masked bilinear weights (zero padding)
};

// grid_sample geometry of output pixel (ox, oy) in agent n's plane, reference arithmetic (identical to warp_fuse.hip):
// F.affine_grid on a float64 theta -> .to(float32) -> (g + 1) * (size / 2) - 0.5 -> floor / floor + 1 taps, masked weights
struct Geom { int C, H, W, Ho, Wo; };      // what make_taps reads: source plane and output grid (the same map in the fusion kernels that build one per tile)

template <class G>      // G: Geom, or a kernel's argument record with the members C, H, W (source plane) and Ho, Wo (output grid)
__device__ __forceinline__ Taps make_taps(const G &a, const double *theta, int n, int ox, int oy) {
    const double xn = (2.0 * ox + 1.0) / a.Wo - 1.0;
    const double yn = (2.0 * oy + 1.0) / a.Ho - 1.0;
    const double *th = theta + n * 6;
    const float gx = (float)(th[0] * xn + th[1] * yn + th[2]);
    const float gy = (float)(th[3] * xn + th[4] * yn + th[5]);
    const float ix = (gx + 1.f) * ((float)a.W / 2) - 0.5f;
    const float iy = (gy + 1.f) * ((float)a.H / 2) - 0.5f;
    Taps t;
    t.w00 = t.w01 = t.w10 = t.w11 = 0.f;
    int x0 = 0, y0 = 0;
    if (ix > -1.f && ix < (float)a.W && iy > -1.f && iy < (float)a.H) {
        const float x0f = floorf(ix), y0f = floorf(iy);
        const float tx = ix - x0f, ty = iy - y0f, ex = 1.f - tx, ey = 1.f - ty;
        x0 = (int)x0f; y0 = (int)y0f;
        const bool vx0 = x0 >= 0, vx1 = x0 + 1 <= a.W - 1, vy0 = y0 >= 0, vy1 = y0 + 1 <= a.H - 1;
        t.w00 = (vx0 && vy0) ? ey * ex : 0.f;
        t.w01 = (vx1 && vy0) ? ey * tx : 0.f;
        t.w10 = (vx0 && vy1) ? ty * ex : 0.f;
        t.w11 = (vx1 && vy1) ? ty * tx : 0.f;
    }
    const int xc0 = min(max(x0, 0), a.W - 1), xc1 = min(max(x0 + 1, 0), a.W - 1);
    const int yc0 = min(max(y0, 0), a.H - 1), yc1 = min(max(y0 + 1, 0), a.H - 1);
    t.o00 = (yc0 * a.W + xc0) * a.C;       // (C * H * W <= INT32_MAX is checked by the entry point)
    t.o01 = (yc0 * a.W + xc1) * a.C;
    t.o10 = (yc1 * a.W + xc0) * a.C;
    t.o11 = (yc1 * a.W + xc1) * a.C;
    return t;
}

// base: channel c_lo of pixel (0, 0) of the agent's plane (wave-uniform pointer + this lane's channel slice); hi4 = C / 8: float4 index of the high channel group
__device__ __forceinline__ void issue(const Taps &t, const float *base, int hi4, float4 (&v)[8]) {
    const float4 *p00 = reinterpret_cast<const float4 *>(base + t.o00), *p01 = reinterpret_cast<const float4 *>(base + t.o01);
    const float4 *p10 = reinterpret_cast<const float4 *>(base + t.o10), *p11 = reinterpret_cast<const float4 *>(base + t.o11);
    v[0] = p00[0]; v[1] = p01[0]; v[2] = p10[0]; v[3] = p11[0];
    v[4] = p00[hi4]; v[5] = p01[hi4]; v[6] = p10[hi4]; v[7] = p11[hi4];
}

__device__ __forceinline__ void blend(const Taps &t, const float4 (&v)[8], float (&X)[8]) {
    // v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11, evaluated left to right, every product and sum rounded (-ffp-contract=off)
#define COALIGN_TAP(j, f) X[j] = v[(j / 4) * 4 + 0].f * t.w00 + v[(j / 4) * 4 + 1].f * t.w01 + v[(j / 4) * 4 + 2].f * t.w10 + v[(j / 4) * 4 + 3].f * t.w11
    COALIGN_TAP(0, x); COALIGN_TAP(1, y); COALIGN_TAP(2, z); COALIGN_TAP(3, w);
    COALIGN_TAP(4, x); COALIGN_TAP(5, y); COALIGN_TAP(6, z); COALIGN_TAP(7, w);
#undef COALIGN_TAP
}

}  // namespace
