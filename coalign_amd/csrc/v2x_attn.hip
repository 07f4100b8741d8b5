// V2X-ViT's heterogeneous agent attention on CHANNELS-LAST maps, gfx950: x + HGTCavAttention(LayerNorm(x)) over the agents of one frame in two launches.
//
// Reference semantics (eval mode, every agent of type 0): HGTCavAttention.forward, sub_modules/hmsa.py:110-151, under PreNorm (base_transformer.py:7-14) and the
// residual of V2XFusionBlock.forward (v2xvit_basic.py:118-122).  Per pixel and receiver i, over the senders j and the heads m (32 channels each):
//   y_j   = LayerNorm(xw_j)                                      xw_j = warp_affine_simple(x_j, theta_j) (the taps of warp_taps.h) or x_j in place
//   att   = softmax_j( q_i^m . A_m k_j^m / sqrt(32) )            q / k / v = the type-0 linears of y, A = relation_att[0]
//   out_i = xw_i + Wa concat_m( sum_j att_ij  M_m^T v_j^m ) + ba M = relation_msg[0]
// Done op by op this materialises v_msg as [heads, H, W, L, L, 32].  The host folds gamma / beta, A, M^T and the scale into ONE 3C x C projection (float64, once per
// parameter change), which leaves per pixel: statistics, [q | k' | v'] = Wqkv yhat + b, an n x n softmax per head, Wa.
//
// Launch 1 (project): a workgroup (4 wavefronts) owns 32 consecutive pixels of ONE agent.  Gather (the blend of warp_fuse_nhwc.hip, or a plain load), the pixel's mean
//   and variance in fp32 (two passes over the registers, the lanes of a pixel meet by cross-lane exchanges), yhat as sp16 pairs in an LDS tile, then the 3C / 32 row
//   tiles of Wqkv dealt over the wavefronts: v_mfma_f32_32x32x16_f16 on sp16 pairs, three products per fp32 product, the pixel on the lane -- disco_fuse.hip's layer 1.
//   The split Wqkv (768 KB at C = 256) streams from L2 in operand order, two steps ahead of its use.  A row tile is one head's 32 channels of q, k' or v'; it goes to
//   the workspace [agent][pixel][3C] as fp32.  Senders that are no receivers skip the query tiles.
// Launch 2 (attend): a workgroup owns 32 pixels of ONE receiver (R workgroups per tile: the 264 tiles of the OPV2V map alone are one wavefront per SIMD, and the
//   lane-serial loads below have nothing to hide behind).  Lane (pixel, head) reads q_i and every k'_j, v'_j of its head (128-byte pieces, coalesced over
//   the heads of a pixel), scores / softmax / weighted sum in fp32, and writes o as sp16 pairs into the LDS tile; the C / 32 row tiles of Wa run on the matrix cores as
//   above; the residual xw_i is gathered again with the same taps (bit for bit the value launch 1 normalised) and the sum stored, 16 bytes per lane.
// Why two launches: q, k', v' of a 32-pixel tile are n x 96 KB at C = 256 and the tokens themselves n x 33 KB -- neither fits the 160 KB of LDS beside the other for
// n >= 5, and keeping them in registers across the agents (online softmax) needs R x 34 registers per head.  The workspace costs one write and R reads of 3 KB per token.
// The caller's stream, no allocation: capturable.  Accuracy: the projections see operands rounded to 22 bits (sp16), everything else is fp32.
#include "common.h"
#include "warp_taps.h"
#include "sp16_tiles.h"

#include "coalign_amd_v2x.h"

namespace {

constexpr int DH = COALIGN_V2X_DIM_HEAD;

__host__ __device__ constexpr size_t param_bytes(int C) { return image_bytes(3 * C, C) + image_bytes(C, C) + (size_t)4 * C * 4; }
__host__ __device__ constexpr size_t lds_bytes(int C) { return (size_t)TP * x_row_bytes(C) + TP * sizeof(Taps); }

struct V2xArgs {
    const float *x;          // [n, H, W, C]
    const double *theta;     // [n, 2, 3] or NULL
    const unsigned char *params;
    float *qkv;              // workspace [n, H W, 3C]
    float *out;              // [R, H, W, C]
    int n, R, C, H, W;
};


// the 8 channels [8 g, 8 g + 8) of pixel `pix` of one agent's plane: the warp's blend, or the stored values
__device__ __forceinline__ void gather8(const float *plane, const Taps *t, int pix, int C, int g, float (&X)[8]) {
    if (t) {
        float4 v[8];
        issue(*t, plane + g * 8, 1, v);
        blend(*t, v, X);
    } else {
        const float4 *src = reinterpret_cast<const float4 *>(plane + (size_t)pix * C + g * 8);
        const float4 v0 = src[0], v1 = src[1];
        X[0] = v0.x; X[1] = v0.y; X[2] = v0.z; X[3] = v0.w; X[4] = v1.x; X[5] = v1.y; X[6] = v1.z; X[7] = v1.w;
    }
}

// ---- launch 1: [q | k' | v'] of one agent's 32 pixels -> workspace ------------------------------------------------------------------------------------------------
template <int MAXI>      // items (pixel, 8-channel group) per lane: 32 * (C / 8) / 256
__global__ __launch_bounds__(256) void v2x_project_kernel(const V2xArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = a.C, G = C / 8, steps = C / 16, xrow_b = x_row_bytes(C);
    char *xt = lds;
    Taps *taps = reinterpret_cast<Taps *>(xt + TP * xrow_b);
    const int HW = a.H * a.W;
    const int tiles_px = (HW + TP - 1) / TP;
    const int agent = blockIdx.x / tiles_px;
    const int pix0 = (blockIdx.x - agent * tiles_px) * TP;
    const float *plane = a.x + (size_t)agent * HW * C;

    if (a.theta != nullptr) {
        if (tid < TP) {
            const Geom geo{C, a.H, a.W, a.H, a.W};
            const int pix = min(pix0 + tid, HW - 1);
            const int oy = pix / a.W;
            taps[tid] = make_taps(geo, a.theta, agent, pix - oy * a.W, oy);
        }
        __syncthreads();
    }
    // (32 * G is a multiple of 256 for both channel counts: every lane holds MAXI live items, a pixel's G items sit in G consecutive lanes of one `it`)
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
        const int idx = it * 256 + tid;
        const int ip = idx / G, ig = idx - ip * G;
        const int pix = min(pix0 + ip, HW - 1);
        float X[8];
        gather8(plane, a.theta != nullptr ? taps + ip : nullptr, pix, C, ig, X);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += X[j];
        const float mean = pixel_sum(s, G) / (float)C;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            X[j] -= mean;
            d = fmaf(X[j], X[j], d);
        }
        const float rstd = 1.0f / sqrtf(pixel_sum(d, G) / (float)C + COALIGN_V2X_LN_EPS);
#pragma unroll
        for (int j = 0; j < 8; ++j) X[j] *= rstd;
        store_split8(xt + ip * xrow_b + ig * 32, X);
    }
    __syncthreads();

    const int col = lane & 31, half = lane >> 5;
    const char *xrow = xt + col * xrow_b;
    const int tiles = 3 * C / 32, first = agent < a.R ? 0 : C / 32;      // a sender that is no receiver needs no queries
    const float *bias = reinterpret_cast<const float *>(a.params + image_bytes(3 * C, C) + image_bytes(C, C));
    const bool live = pix0 + col < HW;
    float *dst = a.qkv + ((size_t)agent * HW + min(pix0 + col, HW - 1)) * (3 * C);
    for (int t = first + wave; t < tiles; t += 4) {
        const floatx16 r = row_tile(a.params, tiles, t, bias, lane, xrow, steps);
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *reinterpret_cast<float4 *>(dst + 32 * t + 8 * i + 4 * half) = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
        }
    }
}

// ---- launch 2: softmax over the senders per (pixel, head), Wa, residual -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void v2x_attend_kernel(const V2xArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = a.C, heads = C / DH, steps = C / 16, xrow_b = x_row_bytes(C);
    char *xt = lds;
    Taps *taps = reinterpret_cast<Taps *>(xt + TP * xrow_b);
    const int HW = a.H * a.W;
    // one workgroup per (pixel tile, receiver): the R receivers of a tile are neighbours in the remapped order, so they run on one XCD and share its L2 copy of k', v'
    const int block = coalign::xcd_remap(blockIdx.x, gridDim.x);
    const int pix0 = (block / a.R) * TP, i = block - (block / a.R) * a.R;
    const unsigned char *wa = a.params + image_bytes(3 * C, C);
    const float *ba = reinterpret_cast<const float *>(wa + image_bytes(C, C)) + 3 * C;
    const int col = lane & 31, half = lane >> 5;
    const char *xrow = xt + col * xrow_b;
    const int ap = tid / heads, ah = tid - ap * heads;      // the attention's (pixel, head) of this lane; lanes with ap >= 32 idle there (C = 64)
    const size_t tok = (size_t)3 * C;

    {
        if (a.theta != nullptr && tid < TP) {
            const Geom geo{C, a.H, a.W, a.H, a.W};
            const int pix = min(pix0 + tid, HW - 1);
            const int oy = pix / a.W;
            taps[tid] = make_taps(geo, a.theta, i, pix - oy * a.W, oy);
        }
        if (ap < TP) {
            const int pix = min(pix0 + ap, HW - 1);
            const float *base = a.qkv + (size_t)pix * tok + ah * DH;
            float q[DH];
            {
                const float4 *src = reinterpret_cast<const float4 *>(base + (size_t)i * HW * tok);
#pragma unroll
                for (int c = 0; c < DH / 4; ++c) {
                    const float4 v = src[c];
                    q[4 * c] = v.x; q[4 * c + 1] = v.y; q[4 * c + 2] = v.z; q[4 * c + 3] = v.w;
                }
            }
            float s[8], m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[j] = -INFINITY;
                if (j < a.n) {
                    const float4 *src = reinterpret_cast<const float4 *>(base + (size_t)j * HW * tok + C);
                    float d = 0.f;
#pragma unroll
                    for (int c = 0; c < DH / 4; ++c) {
                        const float4 v = src[c];
                        d = fmaf(q[4 * c], v.x, d); d = fmaf(q[4 * c + 1], v.y, d); d = fmaf(q[4 * c + 2], v.z, d); d = fmaf(q[4 * c + 3], v.w, d);
                    }
                    s[j] = d;
                    m = fmaxf(m, d);
                }
            }
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[j] = j < a.n ? __expf(s[j] - m) : 0.f;
                den += s[j];
            }
            const float inv = 1.0f / den;
            float o[DH];
#pragma unroll
            for (int c = 0; c < DH; ++c) o[c] = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < a.n) {
                    const float4 *src = reinterpret_cast<const float4 *>(base + (size_t)j * HW * tok + 2 * C);
                    const float p = s[j] * inv;
#pragma unroll
                    for (int c = 0; c < DH / 4; ++c) {
                        const float4 v = src[c];
                        o[4 * c] = fmaf(p, v.x, o[4 * c]); o[4 * c + 1] = fmaf(p, v.y, o[4 * c + 1]);
                        o[4 * c + 2] = fmaf(p, v.z, o[4 * c + 2]); o[4 * c + 3] = fmaf(p, v.w, o[4 * c + 3]);
                    }
                }
#pragma unroll
            for (int g = 0; g < DH / 8; ++g) {
                const float v[8] = {o[8 * g], o[8 * g + 1], o[8 * g + 2], o[8 * g + 3], o[8 * g + 4], o[8 * g + 5], o[8 * g + 6], o[8 * g + 7]};
                store_split8(xt + ap * xrow_b + (ah * (DH / 8) + g) * 32, v);
            }
        }
        __syncthreads();
        const bool live = pix0 + col < HW;
        const int pix = min(pix0 + col, HW - 1);
        const float *plane = a.x + (size_t)i * HW * C;
        for (int t = wave; t < C / 32; t += 4) {
            const floatx16 r = row_tile(wa, C / 32, t, ba, lane, xrow, steps);
            if (live) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c0 = 32 * t + 8 * k + 4 * half;
                    float4 xw;
                    if (a.theta != nullptr) {
                        // the four channels' blend, the expression of warp_taps.h's blend(): products and sums left to right, each rounded
                        const Taps tp = taps[col];
                        const float4 v00 = *reinterpret_cast<const float4 *>(plane + tp.o00 + c0), v01 = *reinterpret_cast<const float4 *>(plane + tp.o01 + c0);
                        const float4 v10 = *reinterpret_cast<const float4 *>(plane + tp.o10 + c0), v11 = *reinterpret_cast<const float4 *>(plane + tp.o11 + c0);
                        xw.x = v00.x * tp.w00 + v01.x * tp.w01 + v10.x * tp.w10 + v11.x * tp.w11;
                        xw.y = v00.y * tp.w00 + v01.y * tp.w01 + v10.y * tp.w10 + v11.y * tp.w11;
                        xw.z = v00.z * tp.w00 + v01.z * tp.w01 + v10.z * tp.w10 + v11.z * tp.w11;
                        xw.w = v00.w * tp.w00 + v01.w * tp.w01 + v10.w * tp.w10 + v11.w * tp.w11;
                    } else {
                        xw = *reinterpret_cast<const float4 *>(plane + (size_t)pix * C + c0);
                    }
                    float4 *dst = reinterpret_cast<float4 *>(a.out + ((size_t)i * HW + pix) * C + c0);
                    coalign::store_stream(dst, make_float4(xw.x + r[4 * k], xw.y + r[4 * k + 1], xw.z + r[4 * k + 2], xw.w + r[4 * k + 3]));
                }
            }
        }
    }
}

template <int MAXI>
int launch(const V2xArgs &a, hipStream_t stream) {
    // the C = 256 tile (33 KB + taps) stays below the 64 KB of dynamic LDS a kernel gets without asking
    const int tiles = (a.H * a.W + TP - 1) / TP;
    hipLaunchKernelGGL(v2x_project_kernel<MAXI>, dim3((unsigned)(a.n * tiles)), dim3(256), lds_bytes(a.C), stream, a);
    int rc = coalign::check_launch();
    if (rc != COALIGN_OK) return rc;
    hipLaunchKernelGGL(v2x_attend_kernel, dim3((unsigned)(tiles * a.R)), dim3(256), lds_bytes(a.C), stream, a);
    return coalign::check_launch();
}

bool shape_ok(int C) { return C == 64 || C == 256; }

}  // namespace

extern "C" size_t coalign_v2x_param_bytes(int C) {
    if (!shape_ok(C)) return 0;
    return param_bytes(C);
}

extern "C" size_t coalign_v2x_workspace_bytes(int n, int C, int H, int W) {
    if (!shape_ok(C) || n < 1 || n > 8 || H < 1 || W < 1 || (size_t)C * H * W > (size_t)INT32_MAX) return 0;
    return (size_t)n * H * W * 3 * C * sizeof(float);
}

extern "C" int coalign_v2x_agent_attention(const float *x, int n, int R, int C, int H, int W, const double *theta, const void *params, size_t params_bytes, float *out,
                                           void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || R < 0 || R > n || C < 1 || H < 1 || W < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > 8 || !shape_ok(C) || (R != n && R > 1)) return COALIGN_ERR_UNSUPPORTED;
    if (n == 0 || R == 0) return COALIGN_OK;
    if (!x || !params || !out || !workspace) return COALIGN_ERR_NULL_POINTER;
    if ((size_t)C * H * W > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (params_bytes != param_bytes(C) || workspace_bytes < coalign_v2x_workspace_bytes(n, C, H, W)) return COALIGN_ERR_BAD_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(workspace)) & 15)
        return COALIGN_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(theta) & 7) return COALIGN_ERR_UNSUPPORTED;
    V2xArgs a;
    a.x = x; a.theta = theta; a.params = static_cast<const unsigned char *>(params); a.qkv = static_cast<float *>(workspace); a.out = out;
    a.n = n; a.R = R; a.C = C; a.H = H; a.W = W;
    return C == 256 ? launch<4>(a, stream) : launch<1>(a, stream);
}
