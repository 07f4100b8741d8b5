// V2X-ViT's feed-forward block on token rows, gfx950: out = x + FeedForward(LayerNorm(x)) in ONE launch.
//
// Reference semantics (eval mode): FeedForward (Linear, GELU, Dropout, Linear, Dropout; sub_modules/base_transformer.py:17-29) under PreNorm
// (base_transformer.py:7-14) with the residual of V2XTEncoder.forward (v2xvit_basic.py:179):
//   yhat = (x - mean) / sqrt(var + 1e-5)
//   h    = GELU(W1' yhat + b1')                 W1' = W1 diag(gamma), b1' = W1 beta + b1 (folded by the host in float64); GELU(z) = 0.5 z (1 + erf(z / sqrt 2))
//   out  = x + W2 h + b2
// A workgroup (4 wavefronts) owns 32 consecutive tokens -- a tile may straddle two maps, tokens are independent:
//   1. the rows of x, LayerNorm's statistics in fp32 over the C / 8 lanes of a token, yhat as sp16 pairs into an LDS tile (rows of x_row_bytes(C));
//   2. the M / 32 row tiles of W1' dealt over the wavefronts on v_mfma_f32_32x32x16_f16 (three products per fp32 product), b1' seeding the accumulators; GELU in
//      fp32; the hidden vector as sp16 pairs into a second LDS tile (rows of x_row_bytes(M)).  A lane holds four consecutive rows of a token, half of an
//      8-channel group: it writes its 8 bytes of the group's h and of its l;
//   3. barrier; the C / 32 row tiles of W2 over that tile, b2 seeding; the residual x (read again: an L2 hit) added, streaming stores.
// The last tile loads zeros for the rows behind `tokens` (yhat = 0, finite throughout) and stores nothing for them.  LDS: 32 (4 C + 16) + 32 (4 M + 16) bytes,
// 33 KB + 66 KB at (256, 512): above 64 KB the limit of dynamic LDS is raised once per device.  No workspace, no atomics: the same input gives the same bits.
// The hidden activations are inside the fp16 range by the packer's static bound (include/coalign_amd_v2x_ffn.h): no range flag.
#include "common.h"
#include "sp16_tiles.h"

#include "coalign_amd_v2x_ffn.h"

namespace {

using namespace coalign;

__host__ __device__ constexpr size_t off_w2(int C, int M) { return image_bytes(M, C); }
__host__ __device__ constexpr size_t off_floats(int C, int M) { return off_w2(C, M) + image_bytes(C, M); }
__host__ __device__ constexpr size_t param_bytes(int C, int M) { return off_floats(C, M) + ((size_t)M + C) * 4; }
__host__ __device__ constexpr size_t lds_bytes(int C, int M) { return (size_t)TP * (x_row_bytes(C) + x_row_bytes(M)); }

struct FfnArgs {
    const float *x;          // [tokens, C]
    const unsigned char *params;
    float *out;              // [tokens, C]
    int tokens, M;
};

__device__ __forceinline__ float gelu(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }

// four consecutive channels 8 g + 4 half .. + 3 of a token's row: the lane's 8 bytes of the group's h and of its l
__device__ __forceinline__ void store_split4(char *group, int half, float v0, float v1, float v2, float v3) {
    uint2 h, l;
    coalign::sp16_split2(v0, v1, h.x, l.x);
    coalign::sp16_split2(v2, v3, h.y, l.y);
    *reinterpret_cast<uint2 *>(group + 8 * half) = h;
    *reinterpret_cast<uint2 *>(group + 16 + 8 * half) = l;
}

template <int C>
__global__ __launch_bounds__(256) void v2x_ffn_kernel(const FfnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int G = C / 8, xrow_b = x_row_bytes(C), MAXI = TP * G / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.M, hrow_b = x_row_bytes(M);
    char *xt = lds, *ht = lds + TP * xrow_b;
    const int tok0 = blockIdx.x * TP;                          // < tokens < 2^31 / 64
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
        const int idx = it * 256 + tid;
        const int ip = idx / G, ig = idx - ip * G;
        float X[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (tok0 + ip < a.tokens) {                            // (the G lanes of a token decide alike)
            const float4 *src = reinterpret_cast<const float4 *>(a.x + (size_t)(tok0 + ip) * C + ig * 8);
            const float4 v0 = src[0], v1 = src[1];
            X[0] = v0.x; X[1] = v0.y; X[2] = v0.z; X[3] = v0.w; X[4] = v1.x; X[5] = v1.y; X[6] = v1.z; X[7] = v1.w;
        }
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
        const float rstd = 1.0f / sqrtf(pixel_sum(d, G) / (float)C + COALIGN_V2X_FFN_LN_EPS);
#pragma unroll
        for (int j = 0; j < 8; ++j) X[j] *= rstd;
        store_split8(xt + ip * xrow_b + ig * 32, X);
    }
    __syncthreads();

    const int col = lane & 31, half = lane >> 5;
    const float *b1 = reinterpret_cast<const float *>(a.params + off_floats(C, M));
    {
        const char *xrow = xt + col * xrow_b;
        char *hrow = ht + col * hrow_b;
        const int tiles = M / 32;
        for (int t = wave; t < tiles; t += 4) {
            const floatx16 r = row_tile(a.params, tiles, t, b1, lane, xrow, C / 16);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                store_split4(hrow + (4 * t + i) * 32, half, gelu(r[4 * i]), gelu(r[4 * i + 1]), gelu(r[4 * i + 2]), gelu(r[4 * i + 3]));
        }
    }
    __syncthreads();

    {
        constexpr int TILES = C / 32;
        const char *hrow = ht + col * hrow_b;
        const unsigned char *img = a.params + off_w2(C, M);
        const int token = tok0 + col;
        for (int t = wave; t < TILES; t += 4) {
            const floatx16 r = row_tile(img, TILES, t, b1 + M, lane, hrow, M / 16);
            if (token < a.tokens) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c0 = 32 * t + 8 * i + 4 * half;
                    const float4 xv = *reinterpret_cast<const float4 *>(a.x + (size_t)token * C + c0);
                    coalign::store_stream(reinterpret_cast<float4 *>(a.out + (size_t)token * C + c0),
                                          make_float4(xv.x + r[4 * i], xv.y + r[4 * i + 1], xv.z + r[4 * i + 2], xv.w + r[4 * i + 3]));
                }
            }
        }
    }
}

template <int C>
int launch(const FfnArgs &a, hipStream_t stream) {
    // M >= 256 (C = 256) or M >= 448 (C = 64) needs more than the 64 KB of dynamic LDS a kernel gets by default: raised once per device and instantiation
    static PerDevice lds_set;
    const size_t lds = lds_bytes(C, a.M);
    if (lds > 65536) {
        if (const int rc = allow_dynamic_lds(lds_set, lds_bytes(C, COALIGN_V2X_FFN_MAX_HIDDEN), v2x_ffn_kernel<C>)) return rc;
    }
    hipLaunchKernelGGL(v2x_ffn_kernel<C>, dim3((unsigned)((a.tokens + TP - 1) / TP)), dim3(256), lds, stream, a);
    return coalign::check_launch();
}

bool shape_ok(int C, int M) { return (C == 64 || C == 256) && M >= 32 && M <= COALIGN_V2X_FFN_MAX_HIDDEN && M % 32 == 0; }

}  // namespace

extern "C" size_t coalign_v2x_ffn_param_bytes(int C, int M) {
    if (!shape_ok(C, M)) return 0;
    return param_bytes(C, M);
}

extern "C" int coalign_v2x_feed_forward(const float *x, int tokens, int C, int M, const void *params, size_t params_bytes, float *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (tokens < 0 || C < 1 || M < 1) return COALIGN_ERR_BAD_SHAPE;
    if (!shape_ok(C, M)) return COALIGN_ERR_UNSUPPORTED;
    if (tokens == 0) return COALIGN_OK;
    if (!x || !params || !out) return COALIGN_ERR_NULL_POINTER;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(params)) & 15) return COALIGN_ERR_NULL_POINTER;
    if (out == x) return COALIGN_ERR_UNSUPPORTED;
    if ((size_t)tokens * (size_t)(C > M ? C : M) > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (params_bytes != param_bytes(C, M)) return COALIGN_ERR_BAD_SHAPE;
    FfnArgs a;
    a.x = x; a.params = static_cast<const unsigned char *>(params); a.out = out;
    a.tokens = tokens; a.M = M;
    return C == 256 ? launch<256>(a, stream) : launch<64>(a, stream);
}
