// When2com's handshake fusion after its 3 x 3 convolutions, gfx950: the pooled key / query heads with the softmax over the agents, and the warp-and-weighted-sum.
//
// Reference semantics: When2commFusion.forward, fuse_modules/fusion_in_one.py:354-431, with km_generator_v2 (fuse_modules/when2com_fuse.py:253-270) and
// AdditiveAttentin (when2com_fuse.py:342-363, sparse=False).  Per frame the reference warps every agent's map into the ego frame, runs policy_net4 and the first
// convolution of the key and the query net (all on coalign_conv3x3_sp / coalign_conv3x3_sp_s2), pools each 128-channel map to 5 x 7, runs a 4480 -> 256 -> 128 ->
// out_size stack per net, projects keys and query to 128 features, takes their dot products, a softmax over the agents, and the weighted sum of the warped maps.
//   w2c_fc1_kernel    pooling + the first fully connected layer.  Its two 256 x 4480 matrices (4.6 MB each) are almost all the bytes of the heads, so the layer is
//                     cut into 2 nets x 16 slices of the 4480 inputs (8 channels = 280 inputs each) x 8 blocks of 32 rows = 256 workgroups; a workgroup pools its
//                     8 channels of every agent into LDS (SplitMaps read in place, sp16 pairs joined exactly), then each wavefront multiplies 8 rows' slices --
//                     loaded once, 16 bytes per lane -- by all agents' vectors.  Partial sums go to the workspace [net][slice][agent][row]: no atomics
//   w2c_tail_kernel   one workgroup of 1024: the partial sums added in slice order + bias + ReLU, the 256 -> 128 layer, the folded 128 x 128 tail (fc.4 and the
//                     attention's linear as one matrix), the dot products, the softmax with the maximum subtracted.  Matrices are stored transposed: lane = output
//                     unit; a layer's inputs are dealt over four thread quarters (its loads are what the launch waits for) and the quarters added in order
//   w2c_fuse_kernel   out = sum_j w_j * warp(x_j): the lane mapping of csrc/v2v_fuse.hip (a wavefront owns 16 pixels and 64 channels, 4 lanes per pixel walk its 8-channel groups),
//                     the taps and the blend of warp_taps.h (the warp of warp_fuse_nhwc.hip bit for bit), streaming stores.  Memory-bound: no LDS, no barriers
// Every sum runs in a fixed order, and agent j's arithmetic never looks at n: the same maps give the same bits, alone or among eight.
#include "common.h"
#include "warp_taps.h"

#include "coalign_amd_w2c.h"

namespace {

using coalign::misaligned;
constexpr int KC = COALIGN_W2C_CHANNELS, PH = COALIGN_W2C_POOL_H, PWD = COALIGN_W2C_POOL_W, BINS = PH * PWD;
constexpr int KF = COALIGN_W2C_FEAT, H1 = COALIGN_W2C_HIDDEN1, H2 = COALIGN_W2C_HIDDEN2, AT = COALIGN_W2C_ATT;
constexpr int SLICES = 16, SLICE_K = KF / SLICES, SLICE_Q = SLICE_K / 4;      // 280 inputs = 70 float4 per slice: 8 channels x 35 bins
constexpr int ROW_BLOCKS = 8, ROWS_PER_WAVE = 8;                              // 8 blocks x 4 wavefronts x 8 rows = 256 rows
constexpr int MAXN = 8;
static_assert(SLICE_K == 8 * BINS && SLICE_K % 4 == 0 && ROW_BLOCKS * 4 * ROWS_PER_WAVE == H1, "slice geometry");

// offsets into the parameter image (floats), the order of include/coalign_amd_w2c.h
constexpr size_t OFF_W1 = 0, OFF_B1 = OFF_W1 + 2 * (size_t)H1 * KF, OFF_FC2 = OFF_B1 + 2 * H1, FC2_BLOCK = (size_t)H1 * H2 + H2;
constexpr size_t OFF_TAIL = OFF_FC2 + 2 * FC2_BLOCK, TAIL_BLOCK = (size_t)H2 * AT + AT;
static_assert(OFF_TAIL + 2 * TAIL_BLOCK == COALIGN_W2C_PARAM_FLOATS, "parameter image");
constexpr size_t WS_FLOATS = (size_t)2 * SLICES * MAXN * H1;

struct ScoreArgs {
    const _Float16 *key, *query;      // SplitMap [n, key_groups * 16, h, w] (the keys: its first 128 channels), [1, 128, h, w]
    const float *params;
    float *part;                      // workspace [net][slice][agent][row]
    float *weights, *logits;
    int n, h, w, key_groups;
};

__global__ __launch_bounds__(256) void w2c_fc1_kernel(const ScoreArgs a) {
    __shared__ float4 pooled4[MAXN * SLICE_Q];
    float *pooled = reinterpret_cast<float *>(pooled4);
    const int rb = blockIdx.x % ROW_BLOCKS, s = (blockIdx.x / ROW_BLOCKS) % SLICES, net = blockIdx.x / (ROW_BLOCKS * SLICES);
    const int nv = net == 0 ? a.n : 1;                                     // the query net sees the ego alone
    const _Float16 *maps = net == 0 ? a.key : a.query;
    const int HW = a.h * a.w, c16 = s >> 1, half = s & 1;
    // ---- AdaptiveAvgPool2d((5, 7)) of this slice's 8 channels, every agent: pooled[agent][8 channels x 35 bins], the order of the flattened vector.  A thread owns one
    // (agent, bin): per pixel of the bin one 16-byte load of the 8 channels' h halves and one of their l halves, four pixels in flight, summed in row-major order
    const uint4 *maps4 = reinterpret_cast<const uint4 *>(maps);
    const int groups = net == 0 ? a.key_groups : KC / 16;
    for (int idx = threadIdx.x; idx < nv * BINS; idx += 256) {
        const int ag = idx / BINS, bin = idx - ag * BINS;
        const int bi = bin / PWD, bj = bin - bi * PWD;
        const int ys = (bi * a.h) / PH, ye = ((bi + 1) * a.h + PH - 1) / PH, xs = (bj * a.w) / PWD, xe = ((bj + 1) * a.w + PWD - 1) / PWD;
        const int bw = xe - xs, cnt = (ye - ys) * bw;
        const uint4 *hi = maps4 + ((size_t)(ag * groups + c16) * 4 + 2 * half) * HW, *lo = hi + HW;
        float sum[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] = 0.f;
        for (int p = 0; p < cnt; p += 4) {
            uint4 hv[4], lv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(p + u, cnt - 1), qy = q / bw;
                const int pix = (ys + qy) * a.w + xs + (q - qy * bw);
                hv[u] = hi[pix];
                lv[u] = lo[pix];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (p + u < cnt) {
                    const unsigned hw_[4] = {hv[u].x, hv[u].y, hv[u].z, hv[u].w}, lw_[4] = {lv[u].x, lv[u].y, lv[u].z, lv[u].w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const unsigned short hb = (unsigned short)(hw_[j >> 1] >> (16 * (j & 1))), lb = (unsigned short)(lw_[j >> 1] >> (16 * (j & 1)));
                        sum[j] += coalign::sp16_join(__builtin_bit_cast(_Float16, hb), __builtin_bit_cast(_Float16, lb));
                    }
                }
        }
        const float fcnt = (float)cnt;
#pragma unroll
        for (int j = 0; j < 8; ++j) pooled[ag * SLICE_K + j * BINS + bin] = sum[j] / fcnt;
    }
    __syncthreads();
    // ---- 8 rows per wavefront: each row's 280-float slice is loaded once and meets every agent's vector
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = rb * (4 * ROWS_PER_WAVE) + wave * ROWS_PER_WAVE;
    const float4 *W = reinterpret_cast<const float4 *>(a.params + OFF_W1 + (size_t)net * H1 * KF) + (size_t)row0 * (KF / 4) + s * SLICE_Q;
    float acc[ROWS_PER_WAVE][MAXN];
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r)
#pragma unroll
        for (int ag = 0; ag < MAXN; ++ag) acc[r][ag] = 0.f;
    for (int q = lane; q < SLICE_Q; q += 64) {
        float4 wv[ROWS_PER_WAVE];
#pragma unroll
        for (int r = 0; r < ROWS_PER_WAVE; ++r) wv[r] = W[(size_t)r * (KF / 4) + q];
#pragma unroll
        for (int ag = 0; ag < MAXN; ++ag)
            if (ag < nv) {
                const float4 p = pooled4[ag * SLICE_Q + q];
#pragma unroll
                for (int r = 0; r < ROWS_PER_WAVE; ++r)
                    acc[r][ag] = fmaf(wv[r].w, p.w, fmaf(wv[r].z, p.z, fmaf(wv[r].y, p.y, fmaf(wv[r].x, p.x, acc[r][ag]))));
            }
    }
    float *part = a.part + ((size_t)(net * SLICES + s) * MAXN) * H1 + row0;
#pragma unroll
    for (int ag = 0; ag < MAXN; ++ag)
        if (ag < nv) {
#pragma unroll
            for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                float v = acc[r][ag];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // a fixed tree: every lane ends with the same sum
                if (lane == r) part[(size_t)ag * H1 + r] = v;
            }
        }
}

// This thread's share of one dense layer: output unit o, KQ consecutive inputs from k0, NV vectors in LDS (LD floats apart): acc[v] = sum_k WT[k][o] x[v][k], k ascending
template <int KQ, int NV>
__device__ __forceinline__ void dense_part(const float *WT, const float *x, int LD, int o, int k0, int ld_out, float (&acc)[MAXN]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.f;
#pragma unroll 16
    for (int k = k0; k < k0 + KQ; ++k) {
        const float wv = WT[(size_t)k * ld_out + o];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = fmaf(wv, x[v * LD + k], acc[v]);
    }
}

constexpr int TAIL_THREADS = 1024, KSPLIT = 4;      // thread = (output unit, net, quarter of the inputs): the quarters are added in order afterwards

__global__ __launch_bounds__(TAIL_THREADS) void w2c_tail_kernel(const ScoreArgs a) {
    __shared__ float h1[(MAXN + 1) * H1];       // vector MAXN: the query's; agents n .. 7 are zero
    __shared__ float part[KSPLIT * (MAXN + 1) * H2];
    __shared__ float h2[(MAXN + 1) * H2];
    __shared__ float kf[(MAXN + 1) * AT];
    __shared__ float lg[MAXN];
    const int t = threadIdx.x, n = a.n;
    // ---- fc.0: the 16 partial sums in slice order, bias, ReLU (thread = row, the vectors dealt over the four thread quarters)
    for (int v = t >> 8; v <= MAXN; v += TAIL_THREADS / H1) {
        const int row = t & (H1 - 1), net = v == MAXN ? 1 : 0, ag = v == MAXN ? 0 : v;
        float r = 0.f;
        if (v == MAXN || v < n) {
            float p[SLICES];
#pragma unroll
            for (int s = 0; s < SLICES; ++s) p[s] = a.part[((size_t)(net * SLICES + s) * MAXN + ag) * H1 + row];
            float sum = p[0];
#pragma unroll
            for (int s = 1; s < SLICES; ++s) sum += p[s];
            r = fmaxf(sum + a.params[OFF_B1 + net * H1 + row], 0.f);
        }
        h1[v * H1 + row] = r;
    }
    __syncthreads();
    // ---- fc.2 and the folded tail: per quarter kq, threads 0 .. 127 the key net on the 8 agent slots, 128 .. 255 the query net on one vector
    const int o = t & 127, net = (t >> 7) & 1, kq = t >> 8, v0 = net == 0 ? 0 : MAXN, nv = net == 0 ? MAXN : 1;
    float acc[MAXN];
    const float *fc2 = a.params + OFF_FC2 + net * FC2_BLOCK;
    if (net == 0) dense_part<H1 / KSPLIT, MAXN>(fc2, h1, H1, o, kq * (H1 / KSPLIT), H2, acc);
    else dense_part<H1 / KSPLIT, 1>(fc2, h1 + MAXN * H1, H1, o, kq * (H1 / KSPLIT), H2, acc);
#pragma unroll
    for (int v = 0; v < MAXN; ++v)
        if (v < nv) part[(kq * (MAXN + 1) + v0 + v) * H2 + o] = acc[v];
    __syncthreads();
    if (kq == 0) {
        const float b = fc2[(size_t)H1 * H2 + o];
#pragma unroll
        for (int v = 0; v < MAXN; ++v)
            if (v < nv) {
                float sum = part[(v0 + v) * H2 + o];
#pragma unroll
                for (int q = 1; q < KSPLIT; ++q) sum += part[(q * (MAXN + 1) + v0 + v) * H2 + o];
                h2[(v0 + v) * H2 + o] = fmaxf(sum + b, 0.f);
            }
    }
    __syncthreads();
    const float *tail = a.params + OFF_TAIL + net * TAIL_BLOCK;
    if (net == 0) dense_part<H2 / KSPLIT, MAXN>(tail, h2, H2, o, kq * (H2 / KSPLIT), AT, acc);
    else dense_part<H2 / KSPLIT, 1>(tail, h2 + MAXN * H2, H2, o, kq * (H2 / KSPLIT), AT, acc);
#pragma unroll
    for (int v = 0; v < MAXN; ++v)
        if (v < nv) part[(kq * (MAXN + 1) + v0 + v) * AT + o] = acc[v];
    __syncthreads();
    if (kq == 0) {
        const float b = tail[(size_t)H2 * AT + o];
#pragma unroll
        for (int v = 0; v < MAXN; ++v)
            if (v < nv) {
                float sum = part[(v0 + v) * AT + o];
#pragma unroll
                for (int q = 1; q < KSPLIT; ++q) sum += part[(q * (MAXN + 1) + v0 + v) * AT + o];
                kf[(v0 + v) * AT + o] = sum + b;
            }
    }
    __syncthreads();
    // ---- logits: <k_j, q> in feature order; softmax over the agents with the maximum subtracted
    if (t < n) {
        float l = 0.f;
        for (int k = 0; k < AT; ++k) l = fmaf(kf[t * AT + k], kf[MAXN * AT + k], l);
        lg[t] = l;
        if (a.logits) a.logits[t] = l;
    }
    __syncthreads();
    if (t < n) {
        float m = lg[0];
        for (int j = 1; j < n; ++j) m = fmaxf(m, lg[j]);
        float den = 0.f;
        for (int j = 0; j < n; ++j) den += expf(lg[j] - m);
        a.weights[t] = expf(lg[t] - m) / den;
    }
}

// ---- warp and weighted sum -----------------------------------------------------------------------------------------------------------------------------------
constexpr int PW = 16;      // pixels per wavefront
constexpr int GL = 4;       // channel groups in flight per pixel (lanes per pixel)
constexpr int CHUNK = 8;    // 8-channel groups per wavefront and pixel tile (blockIdx.y walks the chunks): 64 channels, two per lane


struct FuseArgs {
    const float *x;          // [n, H, W, C]
    const double *theta;     // [n, 2, 3]
    const float *weights;    // [n]
    float *out;              // [H, W, C]
    int n, C, H, W;
};

__global__ __launch_bounds__(256) void w2c_fuse_kernel(const FuseArgs a) {
    const int HW = a.H * a.W, G = a.C / 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile = (long long)blockIdx.x * 4 + wave;
    if (tile >= ((long long)HW + PW - 1) / PW) return;
    const int raw = (int)tile * PW + (lane & (PW - 1));
    const bool live = raw < HW;
    const int pix = live ? raw : HW - 1;      // (a lane past the end reads the last pixel and stores nothing)
    const int oy = pix / a.W, ox = pix - oy * a.W;
    const Geom geo{a.C, a.H, a.W, a.H, a.W};
    Taps t[MAXN];
    float wj[MAXN];
#pragma unroll
    for (int j = 0; j < MAXN; ++j)
        if (j < a.n) {
            t[j] = make_taps(geo, a.theta, j, ox, oy);
            wj[j] = a.weights[j];
        }
    const size_t plane = (size_t)HW * a.C;
    const int g_end = min(G, ((int)blockIdx.y + 1) * CHUNK);
    for (int g = blockIdx.y * CHUNK + lane / PW; g < g_end; g += GL) {
        float acc[8];
#pragma unroll
        for (int j = 0; j < MAXN; ++j)
            if (j < a.n) {
                float4 v[8];
                float X[8];
                issue(t[j], a.x + j * plane + g * 8, 1, v);
                blend(t[j], v, X);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float p = wj[j] * X[k];
                    acc[k] = j == 0 ? p : acc[k] + p;
                }
            }
        if (live) {
            float4 *o = reinterpret_cast<float4 *>(a.out + (size_t)pix * a.C + g * 8);
            coalign::store_stream(o, make_float4(acc[0], acc[1], acc[2], acc[3]));
            coalign::store_stream(o + 1, make_float4(acc[4], acc[5], acc[6], acc[7]));
        }
    }
}


}  // namespace

extern "C" size_t coalign_w2c_workspace_bytes(void) { return WS_FLOATS * sizeof(float); }

extern "C" int coalign_w2c_score(const void *key_sp, int key_channels, const void *query_sp, int n, int h, int w, const float *params, size_t param_bytes, float *weights, float *logits,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0 || h < 1 || w < 1 || key_channels < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > MAXN || key_channels % 16 || key_channels < KC) return COALIGN_ERR_UNSUPPORTED;
    if (param_bytes != (size_t)COALIGN_W2C_PARAM_FLOATS * sizeof(float)) return COALIGN_ERR_BAD_SHAPE;
    if (n == 0) return COALIGN_OK;
    if ((long long)n * key_channels * h * w > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!key_sp || !query_sp || !params || !weights || !workspace) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(key_sp, 15) || misaligned(query_sp, 15) || misaligned(params, 15) || misaligned(workspace, 15) || misaligned(weights, 3) || misaligned(logits, 3))
        return COALIGN_ERR_UNSUPPORTED;
    if (workspace_bytes < WS_FLOATS * sizeof(float)) return COALIGN_ERR_WORKSPACE;
    ScoreArgs a;
    a.key = static_cast<const _Float16 *>(key_sp); a.query = static_cast<const _Float16 *>(query_sp); a.params = params;
    a.part = static_cast<float *>(workspace); a.weights = weights; a.logits = logits;
    a.n = n; a.h = h; a.w = w; a.key_groups = key_channels / 16;
    hipLaunchKernelGGL(w2c_fc1_kernel, dim3(2 * SLICES * ROW_BLOCKS), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    const int rc = coalign::check_launch();
    if (rc != COALIGN_OK) return rc;
    hipLaunchKernelGGL(w2c_tail_kernel, dim3(1), dim3(TAIL_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}

extern "C" int coalign_w2c_fuse(const float *x, int n, int C, int H, int W, const double *theta, const float *weights, float *out, void *stream) {
    if (n < 0 || C < 1 || H < 1 || W < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > MAXN || C % 16) return COALIGN_ERR_UNSUPPORTED;
    if (n == 0) return COALIGN_OK;
    if ((long long)n * C * H * W > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!x || !theta || !weights || !out) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(x, 15) || misaligned(out, 15) || misaligned(theta, 7) || misaligned(weights, 3)) return COALIGN_ERR_UNSUPPORTED;
    FuseArgs a;
    a.x = x; a.theta = theta; a.weights = weights; a.out = out;
    a.n = n; a.C = C; a.H = H; a.W = W;
    const long long tiles = ((long long)H * W + PW - 1) / PW;
    hipLaunchKernelGGL(w2c_fuse_kernel, dim3((unsigned)((tiles + 3) / 4), (unsigned)((C / 8 + CHUNK - 1) / CHUNK)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}
