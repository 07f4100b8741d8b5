// The tile of Where2comm's masked warp + fusion on channels-last maps, shared by w2comm.hip (every agent a dense plane of one tensor, a row table) and
// w2comm_msg.hip (every agent a source of its own: a dense plane or a packed message) so that both kernels warp, blend and fuse with the same instructions in
// the same order and their results agree bit for bit.  What differs between the two is where an agent's pixels lie and how a tap's weight is masked: the SOURCE
// policy F, a kernel-argument struct with
//   theta, n, mode                                     the frame's affines [n, 2, 3] float64, its agent count, COALIGN_FUSE_ATT / COALIGN_FUSE_MAX
//   static constexpr bool kPacked                      true: a tap's offset may be negative = "this pixel was not sent": it is loaded from offset 0 and replaced by zero
//   mask_taps(a, k, agent, taps)                       per lane: fold agent's mask at the four source pixels into the taps of scale k
//   plane(a, k, n)                                     wave-uniform: channel 0 of pixel / row 0 of agent n at scale k
#pragma once
#include "common.h"
#include "warp_taps.h"
#include "nhwc_lanes.h"
#include "coalign_amd.h"

namespace {

constexpr int kMaxScales = 3;

struct ScaleArgs {
    const float *x;       // [n, H, W, C] of this frame (w2comm.hip; unused by a policy with sources of its own)
    const uint8_t *mask;  // [n, H, W]                  (likewise)
    float *out;           // [Ho, Wo, C]
    int C, H, W, Ho, Wo, tiles_x, ntiles, first_block, n_blocks, log2C;
    float sqrt_dim, inv_sqrt_dim;
};

// Fills the launch geometry of `n_scales` scales, heaviest tiles first (by channel count, descending); s[k] describes scale order[k].  -> blocks of the launch.
// The caller has checked the shapes.
inline int plan_scales(ScaleArgs *s, int *order, int n_scales, const int32_t *C, const int32_t *H, const int32_t *W, const int32_t *Ho, const int32_t *Wo, float *const *out) {
    for (int i = 0; i < kMaxScales; ++i) order[i] = i;
    for (int i = 0; i < n_scales; ++i)
        for (int j = i + 1; j < n_scales; ++j)
            if (C[order[j]] > C[order[i]]) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
    int next_block = 0;
    for (int k = 0; k < n_scales; ++k) {
        const int i = order[k];
        ScaleArgs &a = s[k];
        a.x = nullptr; a.mask = nullptr; a.out = out[i]; a.C = C[i]; a.H = H[i]; a.W = W[i]; a.Ho = Ho[i]; a.Wo = Wo[i];
        a.log2C = C[i] == 64 ? 6 : C[i] == 128 ? 7 : 8;
        a.tiles_x = (Wo[i] + (512 / C[i]) - 1) / (512 / C[i]);       // 64 lanes / (C / 8 lanes per pixel) pixels per wave
        a.ntiles = a.tiles_x * ((Ho[i] + 3) / 4);
        a.n_blocks = (a.ntiles + 7) / 8 * 8;
        a.first_block = next_block;
        a.sqrt_dim = (float)sqrt((double)C[i]);
        a.inv_sqrt_dim = 1.0f / a.sqrt_dim;
        next_block += a.n_blocks;
    }
    return next_block;
}

// kPacked: the taps as they are loaded (a pixel that was not sent reads offset 0, which every source has), and the loaded values of such a pixel replaced by zero:
// what lies there may be anything, NaN included, and anything times a zero weight is not zero.
__device__ __forceinline__ Taps loadable(const Taps &t) {
    Taps c = t;
    c.o00 = max(t.o00, 0); c.o01 = max(t.o01, 0); c.o10 = max(t.o10, 0); c.o11 = max(t.o11, 0);
    return c;
}
__device__ __forceinline__ void zero_unsent(const Taps &t, float4 (&v)[8]) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t.o00 < 0) v[0] = v[4] = z;
    if (t.o01 < 0) v[1] = v[5] = z;
    if (t.o10 < 0) v[2] = v[6] = z;
    if (t.o11 < 0) v[3] = v[7] = z;
}

template <int NA, int LPP, class F>
__device__ __forceinline__ void fuse_tile(const F &f, const ScaleArgs &a, int k, int tile, int wave, int lane) {
    constexpr int PPW = 64 / LPP;
    const int li = lane % LPP, pi = lane / LPP;
    const int c_lo = 4 * li, hi4 = a.C / 8;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int oy = ty * 4 + wave;
    if (oy >= a.Ho) return;                        // wave-uniform
    const int ox_raw = tx * PPW + pi;
    const bool pix_ok = ox_raw < a.Wo;
    const int ox = pix_ok ? ox_raw : a.Wo - 1;
    float X[NA][8];
    const int my_agent = min(li, f.n - 1);
    Taps mine = make_taps(a, f.theta, my_agent, ox, oy);                             // lane li of the pixel: agent li's taps
    // x_j * mask_j (where2comm_attn.py:269, :275, :334) folded into the weights: the mask at each tap's source pixel.  A clamped tap lies inside the plane and its
    // weight is zero already.
    f.mask_taps(a, k, my_agent, mine);
    Taps cur = taps_of_agent<LPP>(mine, 0), nxt;
    float4 vc[8], vn[8];
    issue(F::kPacked ? loadable(cur) : cur, f.plane(a, k, 0) + c_lo, hi4, vc);
#pragma unroll
    for (int n = 0; n < NA; ++n) {
        if (n < f.n) {
            if (n + 1 < NA && n + 1 < f.n) {   // the next agent's taps are in flight while this one is blended
                nxt = taps_of_agent<LPP>(mine, n + 1);
                issue(F::kPacked ? loadable(nxt) : nxt, f.plane(a, k, (n + 1) % 8) + c_lo, hi4, vn);
            }
            if constexpr (F::kPacked) zero_unsent(cur, vc);
            blend(cur, vc, X[n]);
            if (n + 1 < NA && n + 1 < f.n) {
                cur = nxt;
#pragma unroll
                for (int j = 0; j < 8; ++j) vc[j] = vn[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) X[n][j] = 0.f;
        }
    }
    const size_t opix = ((size_t)oy * a.Wo + ox) * a.C + c_lo;
    float o[8];
    if (f.mode == COALIGN_FUSE_ATT) {              // AttenFusion (where2comm_attn.py:44-54): the arithmetic of warp_fuse_nhwc.hip, instruction for instruction
        float s[NA];
        float smax = -INFINITY;
#pragma unroll
        for (int n = 0; n < NA; ++n) {
            float p = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) p = fmaf(X[0][j], X[n][j], p);
            s[n] = (LPP == 16) ? group_sum<LPP>(p) / a.sqrt_dim : group_sum<LPP>(p) * a.inv_sqrt_dim;
            if (n < f.n) smax = fmaxf(smax, s[n]);
        }
        float den = 0.f;
#pragma unroll
        for (int n = 0; n < NA; ++n) {
            s[n] = (n < f.n) ? __builtin_amdgcn_exp2f((s[n] - smax) * 1.44269504088896341f) : 0.f;
            den += s[n];
        }
        const float inv_den = 1.0f / den;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
        for (int n = 0; n < NA; ++n) {
            const float sn = s[n] * inv_den;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = fmaf(sn, X[n][j], o[j]);
        }
    } else {                                        // MaxFusion (where2comm_attn.py:56-61)
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = -INFINITY;
#pragma unroll
        for (int n = 0; n < NA; ++n)
            if (n < f.n) {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = fmaxf(o[j], X[n][j]);
            }
    }
    if (pix_ok) {
        coalign::store_stream(reinterpret_cast<float4 *>(a.out + opix), make_float4(o[0], o[1], o[2], o[3]));
        coalign::store_stream(reinterpret_cast<float4 *>(a.out + opix + a.C / 2), make_float4(o[4], o[5], o[6], o[7]));
    }
}

// The body of a kernel `template <int NA> __global__ __launch_bounds__(256) void kernel(const F f)`: one launch over the tiles of up to three scales, block -> its
// scale (first_block and n_blocks are multiples of 8) -> its tile, remapped over the XCDs.  A macro, not a function: the scales are told apart inside the kernel
// itself, where the argument struct stays in the kernel-argument segment (behind a call, even an inlined one, the compiler copied the struct to scratch memory
// first: 280 bytes per lane).
#define COALIGN_W2COMM_FUSE_BLOCK(NA, f)                                                                              \
    do {                                                                                                              \
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;                   \
        const int bid = blockIdx.x;                                                                                   \
        _Pragma("unroll") for (int k = 0; k < kMaxScales; ++k) {                                                      \
            if (k < f.n_scales && bid >= f.s[k].first_block && bid < f.s[k].first_block + f.s[k].n_blocks) {          \
                const ScaleArgs &a = f.s[k];                                                                          \
                const int tile = coalign::xcd_remap(bid - a.first_block, a.n_blocks);                                 \
                if (tile >= a.ntiles) return;                                                                         \
                const int lpp = a.C / 8;                                                                              \
                if (lpp == 8) fuse_tile<NA, 8>(f, a, k, tile, wave, lane);                                            \
                else if (lpp == 16) fuse_tile<NA, 16>(f, a, k, tile, wave, lane);                                     \
                else fuse_tile<NA, 32>(f, a, k, tile, wave, lane);                                                    \
                return;                                                                                               \
            }                                                                                                         \
        }                                                                                                             \
    } while (0)

}  // namespace
