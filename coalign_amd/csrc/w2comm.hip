// Where2comm on gfx950: the communication masks of all agents in one launch, and the masked counterpart of warp_fuse_nhwc.hip.
//
// Reference: Communication.forward (opencood/models/comm_modules/where2comm.py:34-78) thresholds a smoothed confidence map of every agent's own detections into a
// 0 / 1 mask; Where2comm.forward (opencood/models/fuse_modules/where2comm_attn.py:224-341) multiplies every agent's map by its mask (:269, :275, :334), pools the
// mask 2 x 2 for the next backbone level (:274), warps the masked maps into the ego frame (:292, :335) and fuses them per pixel (AttenFusion :44-54, MaxFusion
// :56-61).
//
// (1) w2comm_masks_kernel.  One workgroup of 1024 lanes per agent (grid = 8 x frames, the workgroups past a frame's agent count leave at once): the rate of a
// frame is a count over its ego's whole map, and a workgroup that owns the map counts it in integers without a second launch, a workspace or a float atomic.  The
// workgroup walks its map in 32 x 64 tiles: sigmoid and maximum over the anchors of the tile and its (k - 1) / 2 halo go to LDS once (zero outside the map: the
// convolution's padding), every lane then smooths two pixels from LDS, thresholds them, and the tile's 16 x 32 and 8 x 16 pooled pixels follow from the mask bytes
// in LDS (tiles start at multiples of 32 and 64, so no pooling window crosses a tile).  Agents with an even index inside their frame get all-ones masks
// (communication_mask_nodiag[::2] = 1, where2comm.py:71): agents 2, 4, 6 only fill, agent 0 also computes, for the count.  The smoothing size is a template
// parameter (0, 1, 3, 5, 7, 9): measured on the MI355X at 5 x 2 x 100 x 352, k = 5, 63 us against 97 us with a run-time k.
//
// (2) w2comm_fuse_nhwc_kernel.  The tile scheme, lane layout and arithmetic of warp_fuse_nhwc.hip (same helpers: warp_taps.h, nhwc_lanes.h).  The one difference:
// the lane that computes agent j's taps multiplies each of the four bilinear weights by the mask byte of the tap's SOURCE pixel before the taps go round the pixel's
// lanes.  v * (w * m) equals (v * m) * w bit for bit when m is 0 or 1 (w * 1 = w; a zero product keeps the sign of v either way), so the result is that of
// coalign_warp_fuse_nhwc on maps multiplied by their masks beforehand, and no masked copy of a map is written or read.
#include "common.h"
#include "warp_taps.h"
#include "nhwc_lanes.h"
#include "w2comm_fuse_tile.h"
#include "coalign_amd_where2comm.h"

namespace {

// ---- (1) masks --------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxGroups = COALIGN_W2COMM_MAX_GROUPS, kMaxK = 9, kMaskLevels = 3;
constexpr int kTH = 32, kTW = 64, kMaskThreads = 1024;

struct MaskArgs {
    const float *psm;            // [n_total, A, H, W]
    const float *wts, *bias;     // [k * k], [1]; unused when k == 0
    uint8_t *m[kMaskLevels];     // [n_total, H >> l, W >> l]
    float *rates;                // [n_groups]
    int A, H, W, k, levels;
    float thre;
    uint16_t first[kMaxGroups];  // first agent of the frame
    uint8_t len[kMaxGroups];     // agents of the frame
};

template <int K>      // the smoothing kernel's size, a compile-time constant: the taps unroll, their weights sit in registers and the tile's row stride is a constant
__global__ __launch_bounds__(kMaskThreads) void w2comm_masks_kernel(const MaskArgs a) {
    constexpr int p = K > 0 ? (K - 1) / 2 : 0, stride = kTW + 2 * p;
    __shared__ float conf[(kTH + 2 * p) * stride];
    __shared__ uint8_t m0[kTH * kTW], m1[(kTH / 2) * (kTW / 2)];
    __shared__ int count;
    const int g = blockIdx.y, ai = blockIdx.x, tid = threadIdx.x;
    if (ai >= a.len[g]) return;                                  // workgroup-uniform
    const int agent = a.first[g] + ai;
    const bool ones = (ai & 1) == 0;                             // where2comm.py:71
    const int H = a.H, W = a.W;
    if (ai > 0 && ones) {                                        // nothing to compute: every level is all ones
#pragma unroll
        for (int l = 0; l < kMaskLevels; ++l) {
            if (l >= a.levels) break;
            const int hw = (H >> l) * (W >> l);
            uint8_t *m = a.m[l] + (size_t)agent * hw;
            for (int i = tid; i < hw; i += kMaskThreads) m[i] = 1;
        }
        return;
    }
    if (tid == 0) count = 0;
    float wts[K > 0 ? K * K : 1];
    float bias = 0.f;
    if constexpr (K > 0) {
#pragma unroll
        for (int i = 0; i < K * K; ++i) wts[i] = a.wts[i];          // workgroup-uniform addresses
        bias = a.bias[0];
    }
    const float *psm = a.psm + (size_t)agent * a.A * H * W;
    const int H1 = H >> 1, W1 = W >> 1, H2 = H >> 2, W2 = W >> 2;
    int mine = 0;
    for (int ty0 = 0; ty0 < H; ty0 += kTH)
        for (int tx0 = 0; tx0 < W; tx0 += kTW) {
            // sigmoid().max(dim=1) (where2comm.py:52) of the tile and its halo; zero outside the map
            for (int i = tid; i < (kTH + 2 * p) * stride; i += kMaskThreads) {
                const int r = i / stride, c = i - r * stride;
                const int gy = ty0 - p + r, gx = tx0 - p + c;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    for (int an = 0; an < a.A; ++an) {
                        const float s = 1.f / (1.f + expf(-psm[((size_t)an * H + gy) * W + gx]));
                        v = an == 0 ? s : fmaxf(v, s);
                    }
                }
                conf[i] = v;
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < kTH * kTW / kMaskThreads; ++h) {
                const int i = tid + h * kMaskThreads;
                const int r = i / kTW, c = i % kTW;
                const int gy = ty0 + r, gx = tx0 + c;
                uint8_t bit = 0;
                if (gy < H && gx < W) {
                    float s = conf[r * stride + c];                          // k == 0: the confidence itself (where2comm.py:57)
                    if constexpr (K > 0) {                                   // gaussian_filter (where2comm.py:55): cross-correlation, taps in row-major order, then the bias
                        s = 0.f;
#pragma unroll
                        for (int dy = 0; dy < K; ++dy)
#pragma unroll
                            for (int dx = 0; dx < K; ++dx) s = fmaf(wts[dy * K + dx], conf[(r + dy) * stride + c + dx], s);
                        s += bias;
                    }
                    const bool on = s > a.thre;                              // where2comm.py:61
                    mine += on ? 1 : 0;                                      // the rate counts the mask BEFORE the even agents are set to one (where2comm.py:63)
                    bit = (on || ones) ? 1 : 0;
                    a.m[0][((size_t)agent * H + gy) * W + gx] = bit;
                }
                m0[i] = bit;
            }
            __syncthreads();
            // F.max_pool2d(kernel_size=2) (where2comm_attn.py:274): floor, so every window lies inside the level below
            if (a.levels > 1 && tid < (kTH / 2) * (kTW / 2)) {
                const int r = tid / (kTW / 2), c = tid % (kTW / 2);
                const uint8_t *q = m0 + 2 * r * kTW + 2 * c;
                const uint8_t bit = q[0] | q[1] | q[kTW] | q[kTW + 1];
                m1[tid] = bit;
                const int gy = ty0 / 2 + r, gx = tx0 / 2 + c;
                if (gy < H1 && gx < W1) a.m[1][((size_t)agent * H1 + gy) * W1 + gx] = bit;
            }
            __syncthreads();
            if (a.levels > 2 && tid < (kTH / 4) * (kTW / 4)) {
                const int r = tid / (kTW / 4), c = tid % (kTW / 4);
                const uint8_t *q = m1 + 2 * r * (kTW / 2) + 2 * c;
                const uint8_t bit = q[0] | q[1] | q[kTW / 2] | q[kTW / 2 + 1];
                const int gy = ty0 / 4 + r, gx = tx0 / 4 + c;
                if (gy < H2 && gx < W2) a.m[2][((size_t)agent * H2 + gy) * W2 + gx] = bit;
            }
        }
    if (ai == 0) {
        // an integer count: exact, and the same in any order
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if ((tid & 63) == 0) atomicAdd(&count, mine);
        __syncthreads();
        if (tid == 0) a.rates[g] = (float)count / (float)(H * W);            // communication_mask[0].sum() / (H * W), where2comm.py:63
    }
}

// ---- (2) masked warp + fusion, channels-last ---------------------------------------------------------------------------------------------------------------------
// The tile itself is w2comm_fuse_tile.h's (shared with w2comm_msg.hip); this is its source policy for dense planes of one tensor behind a row table.
struct FuseArgs {
    ScaleArgs s[kMaxScales];
    const double *theta;  // [n, 2, 3]
    int n_scales, n, mode;
    int rows[8];
    static constexpr bool kPacked = false;

    // The mask byte of each tap's source pixel, in the row of x that holds the agent.
    __device__ __forceinline__ void mask_taps(const ScaleArgs &a, int, int agent, Taps &t) const {
        int row = rows[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) row = agent == i ? rows[i] : row;
        const uint8_t *m = a.mask + (size_t)row * (a.H * a.W);
        t.w00 *= (float)m[t.o00 >> a.log2C];
        t.w01 *= (float)m[t.o01 >> a.log2C];
        t.w10 *= (float)m[t.o10 >> a.log2C];
        t.w11 *= (float)m[t.o11 >> a.log2C];
    }
    __device__ __forceinline__ const float *plane(const ScaleArgs &a, int, int n) const { return a.x + rows[n] * ((size_t)a.H * a.W * a.C); }
};

template <int NA>
__global__ __launch_bounds__(256) void w2comm_fuse_nhwc_kernel(const FuseArgs f) {
    COALIGN_W2COMM_FUSE_BLOCK(NA, f);
}

}  // namespace

extern "C" int coalign_w2comm_masks(const float *psm, int n_total, int A, int H, int W, const int32_t *group_len, int n_groups, const float *weights,
                                    const float *bias, int k, float thre, int levels, uint8_t *const *masks, float *rates, void *stream_) {
    using namespace coalign;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_total < 1 || A < 1 || H < 1 || W < 1 || n_groups < 1 || k < 0 || levels < 1) return COALIGN_ERR_BAD_SHAPE;
    if (A > 8 || n_groups > kMaxGroups || levels > kMaskLevels || k > kMaxK || (k > 0 && k % 2 == 0)) return COALIGN_ERR_UNSUPPORTED;
    if (!psm || !group_len || !masks || !rates || (k > 0 && (!weights || !bias))) return COALIGN_ERR_NULL_POINTER;
    if ((H >> (levels - 1)) < 1 || (W >> (levels - 1)) < 1) return COALIGN_ERR_BAD_SHAPE;
    if ((size_t)n_total * A * H * W > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    MaskArgs a;
    int sum = 0;
    for (int g = 0; g < kMaxGroups; ++g) {
        const int len = g < n_groups ? group_len[g] : 0;
        if (g < n_groups) {
            if (len < 1) return COALIGN_ERR_BAD_SHAPE;
            if (len > 8) return COALIGN_ERR_UNSUPPORTED;
        }
        a.first[g] = (uint16_t)sum;
        a.len[g] = (uint8_t)len;
        sum += len;
    }
    if (sum != n_total) return COALIGN_ERR_BAD_SHAPE;
    for (int l = 0; l < kMaskLevels; ++l) {
        if (l < levels && !masks[l]) return COALIGN_ERR_NULL_POINTER;
        a.m[l] = l < levels ? masks[l] : nullptr;
    }
    a.psm = psm; a.wts = weights; a.bias = bias; a.rates = rates;
    a.A = A; a.H = H; a.W = W; a.k = k; a.levels = levels; a.thre = thre;
    const dim3 grid(8, n_groups), block(kMaskThreads);
    if (k == 0) hipLaunchKernelGGL(w2comm_masks_kernel<0>, grid, block, 0, stream, a);
    else if (k == 1) hipLaunchKernelGGL(w2comm_masks_kernel<1>, grid, block, 0, stream, a);
    else if (k == 3) hipLaunchKernelGGL(w2comm_masks_kernel<3>, grid, block, 0, stream, a);
    else if (k == 5) hipLaunchKernelGGL(w2comm_masks_kernel<5>, grid, block, 0, stream, a);
    else if (k == 7) hipLaunchKernelGGL(w2comm_masks_kernel<7>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(w2comm_masks_kernel<9>, grid, block, 0, stream, a);
    return check_launch();
}

extern "C" int coalign_w2comm_fuse_nhwc(int n_scales, const float *const *x, const int32_t *C, const int32_t *H, const int32_t *W, const uint8_t *const *masks,
                                        float *const *out, const int32_t *Ho, const int32_t *Wo, int n, const double *theta, const int32_t *rows, int mode,
                                        void *stream_) {
    using namespace coalign;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_scales < 1 || n_scales > kMaxScales || n < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > 8) return COALIGN_ERR_UNSUPPORTED;
    if (mode != COALIGN_FUSE_ATT && mode != COALIGN_FUSE_MAX) return COALIGN_ERR_UNSUPPORTED;
    if (!x || !C || !H || !W || !masks || !out || !Ho || !Wo || !theta) return COALIGN_ERR_NULL_POINTER;
    FuseArgs f;
    f.theta = theta; f.n = n; f.mode = mode; f.n_scales = n_scales;
    unsigned seen = 0;
    for (int i = 0; i < 8; ++i) {
        const int r = (rows && i < n) ? rows[i] : (i < n ? i : 0);
        if (i < n) {
            if (r < 0 || r >= n || ((seen >> r) & 1u)) return COALIGN_ERR_BAD_SHAPE;
            seen |= 1u << r;
        }
        f.rows[i] = r;
    }
    for (int i = 0; i < n_scales; ++i) {
        if (!x[i] || !out[i] || !masks[i]) return COALIGN_ERR_NULL_POINTER;
        if (C[i] < 1 || H[i] < 1 || W[i] < 1 || Ho[i] < 1 || Wo[i] < 1) return COALIGN_ERR_BAD_SHAPE;
        if (C[i] != 64 && C[i] != 128 && C[i] != 256) return COALIGN_ERR_UNSUPPORTED;
        if ((size_t)C[i] * H[i] * W[i] > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
        if ((reinterpret_cast<uintptr_t>(x[i]) | reinterpret_cast<uintptr_t>(out[i])) & 15) return COALIGN_ERR_UNSUPPORTED;
    }
    int order[kMaxScales];
    const int n_blocks = plan_scales(f.s, order, n_scales, C, H, W, Ho, Wo, out);      // heaviest tiles first
    for (int k = 0; k < n_scales; ++k) { f.s[k].x = x[order[k]]; f.s[k].mask = masks[order[k]]; }
    for (int k = n_scales; k < kMaxScales; ++k) f.s[k] = f.s[0];
    const dim3 grid(n_blocks), block(256);
    if (n == 1) hipLaunchKernelGGL(w2comm_fuse_nhwc_kernel<1>, grid, block, 0, stream, f);
    else if (n == 2) hipLaunchKernelGGL(w2comm_fuse_nhwc_kernel<2>, grid, block, 0, stream, f);
    else if (n == 3) hipLaunchKernelGGL(w2comm_fuse_nhwc_kernel<3>, grid, block, 0, stream, f);
    else if (n <= 5) hipLaunchKernelGGL(w2comm_fuse_nhwc_kernel<5>, grid, block, 0, stream, f);
    else hipLaunchKernelGGL(w2comm_fuse_nhwc_kernel<8>, grid, block, 0, stream, f);
    return check_launch();
}
