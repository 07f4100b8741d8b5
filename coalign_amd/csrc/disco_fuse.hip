// DiscoNet's pixel-weight fusion on CHANNELS-LAST feature maps in ONE launch per frame, gfx950.
//
// Reference semantics (eval mode): DiscoFusion.forward, fuse_modules/fusion_in_one.py:144-171, with PixelWeightLayer, fuse_modules/disco_fuse.py:76-99:
//   xw_j = warp_affine_simple(x_j, theta_j)                      every agent, the ego included (the taps of warp_taps.h: the warp of warp_fuse_nhwc.hip)
//   s_j  = relu(w4 . relu(W3 relu(W2 relu(W1 [xw_j | x_0] + b1) + b2) + b3) + b4)      BatchNorms folded into W1..W3 by the host, x_0 = the UNWARPED ego map
//   out  = sum_j softmax_j(s_j) xw_j                             an agent warped wholly outside contributes xw_j = 0 and still takes its softmax share
// Done op by op this writes and re-reads an [n, 2C, H, W] concatenation and an [n, 128, H, W] activation; here nothing but x is read and nothing but out written.
//
// A workgroup (4 wavefronts) owns 32 consecutive pixels of the flattened H x W grid and walks the agents:
//   gather   the 256 lanes split the tile's 32 x C/8 (pixel, 8-channel group) items; an item is 8 x 16 B loads (4 taps x 2), the blend of warp_fuse_nhwc.hip, and
//            the sp16 split (common.h) of the 8 warped values, written to the LDS tile [pixel][group][8 h | 8 l] (rows padded by 16 B: the 32 lanes of a
//            ds_read_b128 operand read are 4 banks apart).  The lane KEEPS its fp32 values in registers for the weighted sum
//   layer 1  W1 = [W1a | W1b].  The ego half W1b x_0 + b1 is computed once per tile (the same gather path without taps) and seeds every agent's accumulator, so
//            an agent costs C x 128 products per pixel, not 2C x 128.  Wavefront w owns hidden rows [32 w, 32 w + 32): v_mfma_f32_32x32x16_f16 on sp16 pairs,
//            three products per fp32 product (w_h x_h | w_h x_l + w_l x_h in a second accumulator that enters with 2^-10), the pixel on the lane.  The split W1
//            (128 KB at C = 256) does not sit in LDS: every wavefront reads ITS 32 rows of the packed image (one contiguous 2 KB piece per 16-channel step, made
//            by the host in operand order) from L2, two steps ahead of their use
//   layer 2  the 128 hidden values of a pixel cross the wavefronts through a second LDS tile (sp16 again); wavefront 0 runs 128 -> 32 on the matrix cores and
//            32 -> 8 -> 1 on the VALU (fp32 fmaf; the two lane halves of a pixel meet with one cross-half exchange), while wavefront 1 computes the NEXT agent's taps
//   softmax  ONLINE: wavefront 0 keeps the running maximum and denominator of its 32 pixels and publishes (rescale, weight) of the agent; every lane then
//            updates acc = acc * rescale + weight * xw for the items it gathered.  Chosen over a second gather after the weights are known because the warped
//            values are already in the gathering lane's registers (C / 8 <= 48 floats + as many for acc): the second pass would re-read n x 1 KB per pixel from L2
//            and recompute every blend, the accumulator costs two fmaf per value.  After the last agent acc / denominator is stored (16 B pieces, channels-last).
// No workspace, no allocation, the caller's stream: capturable.  Accuracy: the matrix layers see operands rounded to 22 bits (sp16), everything else is fp32.
#include "common.h"
#include "warp_taps.h"
#include "sp16_tiles.h"

#include "coalign_amd_disco.h"

namespace {

using namespace coalign;
constexpr int H1 = 128, H2 = 32, H3 = 8;       // PixelWeightLayer's widths (disco_fuse.py:80-89)
constexpr int H1_ROW = H1 * 4 + 16;            // bytes of a pixel's row in the hidden tile: 16 groups x (8 h + 8 l) + the bank pad
// float section of the parameter image: b1[128] b2[32] w3[2 halves][8 outputs][16 registers] b3[8] w4[8] b4[1] + 3 of padding
constexpr int F_B1 = 0, F_B2 = 128, F_W3 = 160, F_B3 = 416, F_W4 = 424, F_B4 = 432, F_COUNT = 436;

__host__ __device__ constexpr size_t w1_bytes(int C) { return (size_t)(C / 16) * 4 * 64 * 32; }      // [C / 16 steps][4 row tiles][64 lanes][8 h | 8 l] fp16
constexpr size_t kW2Bytes = 8 * 64 * 32;                                                              // [8 steps][64 lanes][8 h | 8 l] fp16
__host__ __device__ constexpr size_t param_bytes(int C) { return 2 * w1_bytes(C) + kW2Bytes + F_COUNT * 4; }
__host__ __device__ constexpr size_t lds_bytes(int C) { return (size_t)TP * x_row_bytes(C) + TP * H1_ROW + TP * sizeof(Taps) + F_COUNT * 4 + 3 * TP * 4; }

struct DiscoArgs {
    const float *x;          // [n, H, W, C]
    const double *theta;     // [n, 2, 3]
    const unsigned char *params;
    float *out;              // [H, W, C]
    int n, C, H, W;
};

// rows [32 w, 32 w + 32) of W (image `img`, this wavefront's row tile) times the LDS tile's `steps` 16-channel steps, for the 32 pixels; the weight pieces of two
// steps are fetched while the two before them are multiplied.  steps is even (C % 32 == 0).
__device__ __forceinline__ void layer1(const unsigned char *img, int wave, int lane, const char *xrow, int steps, floatx16 &acc, floatx16 &accl) {
    const unsigned char *wp = img + ((size_t)wave * 64 + lane) * 32;      // + step * 4 * 64 * 32
    constexpr size_t STEP = 4 * 64 * 32;
    const int h = lane >> 5;
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
}

template <int MAXI>      // items (pixel, 8-channel group) per lane: 32 * (C / 8) / 256 rounded up
__global__ __launch_bounds__(256) void disco_fuse_kernel(const DiscoArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = a.C, G = C / 8, steps = C / 16, xrow_b = x_row_bytes(C);
    char *xt = lds;                                                        // [TP][xrow_b]
    char *ht = xt + TP * xrow_b;                                           // [TP][H1_ROW]
    Taps *taps = reinterpret_cast<Taps *>(ht + TP * H1_ROW);               // [TP]
    float *fp = reinterpret_cast<float *>(taps + TP);                      // [F_COUNT]
    float *s_scale = fp + F_COUNT, *s_weight = s_scale + TP, *s_inv = s_weight + TP;
    const unsigned char *w1a = a.params, *w1b = w1a + w1_bytes(C), *w2 = w1b + w1_bytes(C);
    const float *fparams = reinterpret_cast<const float *>(w2 + kW2Bytes);

    const int HW = a.H * a.W;
    const int tile = coalign::xcd_remap(blockIdx.x, gridDim.x);
    const int pix0 = tile * TP;
    const Geom geo{C, a.H, a.W, a.H, a.W};
    const size_t plane = (size_t)HW * C;

    // this lane's items: item it is (pixel ip[it] of the tile, channel group ig[it]); the lanes of a pixel read its C floats as consecutive 32-byte pieces
    int ip[MAXI], ig[MAXI];
    bool live[MAXI];
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
        const int idx = it * 256 + tid;
        live[it] = idx < TP * G;
        ip[it] = live[it] ? idx / G : 0;
        ig[it] = live[it] ? idx - ip[it] * G : 0;
    }

    for (int i = tid; i < F_COUNT; i += 256) fp[i] = fparams[i];
    auto write_taps = [&](int agent) {                                     // lanes 0 .. 31 of one wavefront: the taps of the tile's pixels in `agent`'s plane
        if (lane < TP) {
            const int pix = min(pix0 + lane, HW - 1);
            const int oy = pix / a.W;
            taps[lane] = make_taps(geo, a.theta, agent, pix - oy * a.W, oy);
        }
    };
    if (wave == 1) write_taps(0);

    // ---- the ego half: x_0 as it stands -> tile -> E = W1b x_0 + b1 (kept in registers, seeds every agent) ----
#pragma unroll
    for (int it = 0; it < MAXI; ++it)
        if (live[it]) {
            const int pix = min(pix0 + ip[it], HW - 1);
            const float4 *src = reinterpret_cast<const float4 *>(a.x + (size_t)pix * C + ig[it] * 8);
            const float4 v0 = src[0], v1 = src[1];
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            store_split8(xt + ip[it] * xrow_b + ig[it] * 32, v);
        }
    __syncthreads();
    const int col = lane & 31, half = lane >> 5;
    const char *xrow = xt + col * xrow_b;
    floatx16 ego;
    {
        floatx16 acc, accl;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            acc[q] = fp[F_B1 + 32 * wave + 8 * (q >> 2) + 4 * half + (q & 3)];
            accl[q] = 0.f;
        }
        layer1(w1b, wave, lane, xrow, steps, acc, accl);
#pragma unroll
        for (int q = 0; q < 16; ++q) ego[q] = fmaf(accl[q], coalign::kSp16LowInv, acc[q]);
    }
    __syncthreads();

    float X[MAXI][8], O[MAXI][8];
#pragma unroll
    for (int it = 0; it < MAXI; ++it)
#pragma unroll
        for (int j = 0; j < 8; ++j) O[it][j] = 0.f;
    float run_max = -INFINITY, run_den = 0.f;                              // wavefront 0: of pixel `col`

    for (int agent = 0; agent < a.n; ++agent) {
        // ---- gather: warp this agent's map into the tile; the fp32 values stay in X ----
        const float *xa = a.x + agent * plane;
#pragma unroll
        for (int it = 0; it < MAXI; ++it)
            if (live[it]) {
                const Taps t = taps[ip[it]];
                float4 v[8];
                issue(t, xa + ig[it] * 8, 1, v);
                blend(t, v, X[it]);
                store_split8(xt + ip[it] * xrow_b + ig[it] * 32, X[it]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) X[it][j] = 0.f;
            }
        __syncthreads();
        // ---- layer 1: relu(E + W1a xw) -> hidden tile (sp16) ----
        {
            floatx16 acc = ego, accl;
#pragma unroll
            for (int q = 0; q < 16; ++q) accl[q] = 0.f;
            layer1(w1a, wave, lane, xrow, steps, acc, accl);
            char *hrow = ht + col * H1_ROW + half * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {                                 // registers 4 i .. 4 i + 3: hidden rows 32 wave + 8 i + 4 half + (0 .. 3) = group 4 wave + i
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(accl[4 * i + j], coalign::kSp16LowInv, acc[4 * i + j]), 0.f);
                uint2 hh, ll;
                coalign::sp16_split2(v[0], v[1], hh.x, ll.x);
                coalign::sp16_split2(v[2], v[3], hh.y, ll.y);
                *reinterpret_cast<uint2 *>(hrow + (4 * wave + i) * 32) = hh;
                *reinterpret_cast<uint2 *>(hrow + (4 * wave + i) * 32 + 16) = ll;
            }
        }
        __syncthreads();
        // ---- wavefront 0: layers 2-4 and the online softmax of its 32 pixels; wavefront 1: the next agent's taps ----
        if (wave == 0) {
            floatx16 acc, accl;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                acc[q] = fp[F_B2 + 8 * (q >> 2) + 4 * half + (q & 3)];
                accl[q] = 0.f;
            }
            const char *hr = ht + col * H1_ROW;
#pragma unroll
            for (int s = 0; s < H1 / 16; ++s) {
                const Pair w = load_pair(w2 + ((size_t)s * 64 + lane) * 32);
                const Pair x = load_pair(hr + (2 * s + half) * 32);
                mfma3(w, x, acc, accl);
            }
            float h2[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) h2[q] = fmaxf(fmaf(accl[q], coalign::kSp16LowInv, acc[q]), 0.f);
            float s = fp[F_B4];
#pragma unroll
            for (int o = 0; o < H3; ++o) {
                const float *w3 = fp + F_W3 + (half * H3 + o) * 16;       // this half's 16 of the 32 columns of row o, in register order
                float p = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) p = fmaf(w3[q], h2[q], p);
                p += __shfl_xor(p, 32);                                    // the pixel's other half (a + b == b + a: both halves hold the same sum)
                s = fmaf(fp[F_W4 + o], fmaxf(p + fp[F_B3 + o], 0.f), s);
            }
            s = fmaxf(s, 0.f);
            const float m = fmaxf(run_max, s);
            const float rescale = __builtin_amdgcn_exp2f((run_max - m) * 1.44269504088896341f);      // first agent: exp2(-inf) = 0
            const float weight = __builtin_amdgcn_exp2f((s - m) * 1.44269504088896341f);
            run_den = fmaf(run_den, rescale, weight);
            run_max = m;
            if (half == 0) {
                s_scale[col] = rescale;
                s_weight[col] = weight;
                s_inv[col] = 1.0f / run_den;
            }
        } else if (wave == 1 && agent + 1 < a.n) {
            write_taps(agent + 1);
        }
        __syncthreads();
        // ---- every lane: acc = acc * rescale + weight * xw for its items ----
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const float rescale = s_scale[ip[it]], weight = s_weight[ip[it]];
#pragma unroll
            for (int j = 0; j < 8; ++j) O[it][j] = fmaf(weight, X[it][j], O[it][j] * rescale);
        }
        // (the next agent's gather overwrites the pixel tile, last read before the barrier above; s_scale / s_weight are rewritten two barriers from here)
    }
#pragma unroll
    for (int it = 0; it < MAXI; ++it)
        if (live[it] && pix0 + ip[it] < HW) {
            const float inv = s_inv[ip[it]];
            float4 *dst = reinterpret_cast<float4 *>(a.out + (size_t)(pix0 + ip[it]) * C + ig[it] * 8);
            coalign::store_stream(dst, make_float4(O[it][0] * inv, O[it][1] * inv, O[it][2] * inv, O[it][3] * inv));
            coalign::store_stream(dst + 1, make_float4(O[it][4] * inv, O[it][5] * inv, O[it][6] * inv, O[it][7] * inv));
        }
}

template <int MAXI>
int launch(const DiscoArgs &a, hipStream_t stream) {
    // C > 336 needs more than the 64 KB of dynamic LDS a kernel gets by default: raised once per device and instantiation, at the first launch
    static PerDevice lds_set;
    if (const int rc = allow_dynamic_lds(lds_set, lds_bytes(COALIGN_DISCO_MAX_CHANNELS), disco_fuse_kernel<MAXI>)) return rc;
    const int tiles = (a.H * a.W + TP - 1) / TP;
    hipLaunchKernelGGL(disco_fuse_kernel<MAXI>, dim3(tiles), dim3(256), lds_bytes(a.C), stream, a);
    return coalign::check_launch();
}

}  // namespace

extern "C" size_t coalign_disco_param_bytes(int C) {
    if (C < 32 || C > COALIGN_DISCO_MAX_CHANNELS || C % 32) return 0;
    return param_bytes(C);
}

extern "C" int coalign_disco_fuse(const float *x, int n, int C, int H, int W, const double *theta, const void *params, size_t params_bytes, float *out,
                                  void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || C < 1 || H < 1 || W < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > 8 || C < 32 || C > COALIGN_DISCO_MAX_CHANNELS || C % 32) return COALIGN_ERR_UNSUPPORTED;
    if (n == 0) return COALIGN_OK;
    if (!x || !theta || !params || !out) return COALIGN_ERR_NULL_POINTER;
    if ((size_t)C * H * W > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (params_bytes != param_bytes(C)) return COALIGN_ERR_BAD_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(params)) & 15) return COALIGN_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(theta) & 7) return COALIGN_ERR_UNSUPPORTED;
    DiscoArgs a;
    a.x = x; a.theta = theta; a.params = static_cast<const unsigned char *>(params); a.out = out;
    a.n = n; a.C = C; a.H = H; a.W = W;
    if (C <= 128) return launch<2>(a, stream);
    if (C <= 256) return launch<4>(a, stream);
    return launch<6>(a, stream);
}
