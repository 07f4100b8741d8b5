// The glue of the pose-robust V2VNet between its 3 x 3 convolutions, gfx950.
//
// Reference semantics: PointPillarV2VNetRobust.train_forward (models/point_pillar_v2vnet_robust.py:205-267) with PoseRegressionWraper, WeightedEM, AttentionWrapper
// (models/sub_modules/v2v_robust_module.py) and V2VNetFusion with agg_operator 'weight' (models/fuse_modules/v2v_fuse.py:51-166).  The convolutions run on
// coalign_conv3x3_sp / coalign_conv3x3_sp_s2 and the warps on coalign_v2v_warp_split; what lies between them is here:
//   v2vr_pool_act      (a_p + e_{p / n}) -> MaxPool 2 -> LeakyReLU -> SplitMap: the tail of every pooled convolution of both nets.  Memory-bound, the lane mapping of
//                      v2v_lanes.h (a wavefront owns 16 output pixels, 4 lanes per pixel walk the 8-channel groups), one pass, streaming stores
//   v2vr_score_head    cropped global max -> LeakyReLU -> Linear h -> 1 -> sigmoid per pair (one workgroup each: bound by the read of its map), then the row sums
//                      and the weights in a second, one-workgroup launch
//   v2vr_pose_head     LeakyReLU -> MaxPool 2 -> mean -> three Linear layers for ALL pairs in one workgroup: a wavefront holds one fc row in registers and applies
//                      it to every pair, so each row is read once per frame; latency-bound (0.5 MB of weights through one CU)
//   v2vr_pairwise      3-dof poses -> pairwise matrices and normalised affines, closed form, float64
//   v2vr_consistency   the whole WeightedEM of a frame in one workgroup, float64: per-agent state in LDS, one lane per agent in the reweighting steps, one lane per
//                      pair in update_weight; latency-bound (10 x 15 dependent 4 x 4 inversions)
//   v2vr_aggregate     v2v_aggregate with the weighted sum over the senders
// No allocation, no host synchronisation, the caller's stream: capturable.  Sums run in fixed orders; the only atomic is the OR into the range word.
#include "common.h"
#include "warp_taps.h"
#include "v2v_lanes.h"

#include "coalign_amd_v2v_robust.h"

namespace {

using coalign::misaligned;
constexpr int kMaxAgents = 8, kMaxCav = 16, kMaxSamples = 2 * (kMaxAgents - 1);
constexpr float kSlope = 0.01f;                     // LeakyReLU(negative_slope=0.01) of both nets
constexpr double kPi = 3.14159265358979323846;


__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * kSlope; }

// ---- (14a) ------------------------------------------------------------------------------------------------------------------------------------------------
struct PoolArgs {
    const float *a, *e;      // [P, H, W, C], [P / n, H, W, C] or NULL
    void *out;               // SplitMap [P, C, H / 2, W / 2] or float [P, H / 2, W / 2, C]
    int *range_flag;
    int P, n, C, H, W, out_kind;
};

__global__ __launch_bounds__(256) void pool_act_kernel(const PoolArgs a) {
    const int Ho = a.H / 2, Wo = a.W / 2, HWo = Ho * Wo, C = a.C, G = C / 8;
    Place p;
    if (!place(a.P, HWo, p)) return;
    const int oy = p.pix / Wo, ox = p.pix - oy * Wo;
    const size_t row = (size_t)a.W * C, first = ((size_t)(2 * oy) * a.W + 2 * ox) * C, plane = (size_t)a.H * a.W * C;
    const float *ap = a.a + (size_t)p.map * plane + first;
    const float *ep = a.e ? a.e + (size_t)(p.map / a.n) * plane + first : nullptr;
    bool big = false;
    for (int g = p.g0; g < G; g += GL) {
        float v[4][8], o[8];
        load8(ap + g * 8, v[0]);
        load8(ap + C + g * 8, v[1]);
        load8(ap + row + g * 8, v[2]);
        load8(ap + row + C + g * 8, v[3]);
        if (ep) {
            float t[4][8];
            load8(ep + g * 8, t[0]);
            load8(ep + C + g * 8, t[1]);
            load8(ep + row + g * 8, t[2]);
            load8(ep + row + C + g * 8, t[3]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int k = 0; k < 8; ++k) v[q][k] = v[q][k] + t[q][k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float m = v[0][k];                                            // max_pool2d's scan: row by row, a later value wins only if it is greater (or NaN)
#pragma unroll
            for (int q = 1; q < 4; ++q) m = (v[q][k] > m || v[q][k] != v[q][k]) ? v[q][k] : m;
            o[k] = lrelu(m);
        }
        if (a.out_kind == COALIGN_V2V_OUT_SP) {
            big = store_split8<true>(static_cast<uint4 *>(a.out), p.map, C / 16, g, HWo, p.pix, o, p.live) || big;
        } else if (p.live) {
            float4 *q = reinterpret_cast<float4 *>(static_cast<float *>(a.out) + ((size_t)p.map * HWo + p.pix) * C + g * 8);
            coalign::store_stream(q, make_float4(o[0], o[1], o[2], o[3]));
            coalign::store_stream(q + 1, make_float4(o[4], o[5], o[6], o[7]));
        }
    }
    if (a.range_flag && big) atomicOr(a.range_flag, 1);
}

// ---- (14b) ------------------------------------------------------------------------------------------------------------------------------------------------
struct ScoreArgs {
    const float *y, *w, *b, *alpha;
    float *scores, *weight;
    int n, L, h, H, W;
};

// one workgroup per [L, L] entry; 256 threads = (256 / (h / 4)) pixel groups x h / 4 float4 channel lanes
__global__ __launch_bounds__(256) void score_kernel(const ScoreArgs a) {
    __shared__ float4 part[256];
    __shared__ float red[256];
    const int pr = blockIdx.x, i = pr / a.L, j = pr - i * a.L, tid = threadIdx.x;
    if (i >= a.n || j >= a.n) {                                           // (uniform per workgroup)
        if (tid == 0) a.scores[pr] = 0.f;
        return;
    }
    const int q = a.h / 4, PG = 256 / q, c4 = tid % q, pg = tid / q;
    const int Hc = a.H & ~1, Wc = a.W & ~1, count = Hc * Wc;              // MaxPool 2 then the global max = the max over the floor-cropped map
    const float ninf = -__builtin_inff();
    float4 m = make_float4(ninf, ninf, ninf, ninf);
    if (pg < PG) {
        const float4 *yp = reinterpret_cast<const float4 *>(a.y + (size_t)(i * a.n + j) * a.H * a.W * a.h) + c4;
        for (int k = pg; k < count; k += PG) {
            const int r = k / Wc, c = k - r * Wc;
            const float4 v = yp[(size_t)(r * a.W + c) * q];
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    part[tid] = m;
    __syncthreads();
    float dot = 0.f;
    if (tid < q) {
        for (int k = 1; k < PG; ++k) {
            const float4 v = part[tid + k * q];
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
        const float4 w = reinterpret_cast<const float4 *>(a.w)[tid];
        dot = ((lrelu(m.x) * w.x + lrelu(m.y) * w.y) + lrelu(m.z) * w.z) + lrelu(m.w) * w.w;
    }
    red[tid] = dot;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {                                   // a fixed tree: the same sum on every run
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.scores[pr] = 1.0f / (1.0f + expf(-(red[0] + a.b[0])));
}

__global__ __launch_bounds__(256) void score_weight_kernel(const ScoreArgs a) {
    const int t = threadIdx.x;
    if (t >= a.L * a.L) return;
    const int i = t / a.L;
    float sum = 0.f;
    for (int j = 0; j < a.L; ++j) sum = sum + a.scores[i * a.L + j];
    a.weight[t] = a.scores[t] / ((sum + a.alpha[0]) + 1e-4f);
}

// ---- (14d) ------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kHeadThreads = 512, kHeadWaves = kHeadThreads / 64, kHeadPairs = 8;

struct HeadArgs {
    const _Float16 *y4;      // SplitMap [P, h, H4, W4]
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const double *T;
    float *corr, *ws;
    double *Tn;
    int n, L, h, H4, W4;
};

// out[p][r] = act(bias[r] + sum_k W[r][k] in[p][k]) for every pair p: a wavefront takes the rows r = wave, wave + 8, ..; its lanes hold the row (k = 4 lane + 256 t)
__device__ __forceinline__ void fc_layer(const float *Wt, const float *bias, const float *in, float *out, int P, int h, int rows, int out_stride, bool act) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < rows; r += kHeadWaves) {
        float4 w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = lane * 4 + 256 * t;
            w[t] = k < h ? *reinterpret_cast<const float4 *>(Wt + (size_t)r * h + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float br = bias[r];
        for (int p0 = 0; p0 < P; p0 += kHeadPairs) {                      // kHeadPairs pairs at a time: their loads are in flight together (the loop is latency-bound)
            float acc[kHeadPairs];
#pragma unroll
            for (int u = 0; u < kHeadPairs; ++u) {
                acc[u] = 0.f;
                const int p = min(p0 + u, P - 1);                         // (a pair past the end repeats the last one and stores nothing)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int k = lane * 4 + 256 * t;
                    if (k < h) {
                        const float4 z = *reinterpret_cast<const float4 *>(in + (size_t)p * h + k);
                        acc[u] = fmaf(w[t].x, z.x, acc[u]); acc[u] = fmaf(w[t].y, z.y, acc[u]); acc[u] = fmaf(w[t].z, z.z, acc[u]); acc[u] = fmaf(w[t].w, z.w, acc[u]);
                    }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
#pragma unroll
                for (int u = 0; u < kHeadPairs; ++u) acc[u] = acc[u] + __shfl_xor(acc[u], off);
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < kHeadPairs; ++u)
                    if (p0 + u < P) {
                        const float v = acc[u] + br;
                        out[(size_t)(p0 + u) * out_stride + r] = act ? lrelu(v) : v;
                    }
            }
        }
    }
}

__global__ __launch_bounds__(kHeadThreads) void pose_head_kernel(const HeadArgs a) {
    const int P = a.n * a.n, h = a.h, H4 = a.H4, W4 = a.W4, Hp = H4 / 2, Wp = W4 / 2, tid = threadIdx.x;
    float *z0 = a.ws, *z1 = a.ws + (size_t)P * h, *z2 = a.ws + (size_t)2 * P * h;      // [P, h], [P, h], [P, 4]
    const size_t hw = (size_t)H4 * W4;
    for (int idx = tid; idx < P * h; idx += kHeadThreads) {
        const int p = idx / h, c = idx - p * h;
        const _Float16 *hi = a.y4 + ((((size_t)p * (h / 16) + c / 16) * 4 + ((c & 15) >> 3) * 2) * hw) * 8 + (c & 7), *lo = hi + hw * 8;
        float sum = 0.f;
        for (int py = 0; py < Hp; ++py)
            for (int px = 0; px < Wp; ++px) {
                const size_t o = ((size_t)(2 * py) * W4 + 2 * px) * 8;
                const float v00 = coalign::sp16_join(hi[o], lo[o]), v01 = coalign::sp16_join(hi[o + 8], lo[o + 8]);
                const float v10 = coalign::sp16_join(hi[o + (size_t)W4 * 8], lo[o + (size_t)W4 * 8]), v11 = coalign::sp16_join(hi[o + (size_t)W4 * 8 + 8], lo[o + (size_t)W4 * 8 + 8]);
                sum = sum + lrelu(fmaxf(fmaxf(v00, v01), fmaxf(v10, v11)));
            }
        z0[idx] = sum / (float)(Hp * Wp);
    }
    __syncthreads();
    fc_layer(a.w1, a.b1, z0, z1, P, h, h, h, true);
    __syncthreads();
    fc_layer(a.w2, a.b2, z1, z0, P, h, h, h, true);
    __syncthreads();
    fc_layer(a.w3, a.b3, z0, z2, P, h, 3, 4, false);
    __syncthreads();
    for (int pr = tid; pr < a.L * a.L; pr += kHeadThreads) {
        const int i = pr / a.L, j = pr - i * a.L;
        double M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        float c3[3] = {0.f, 0.f, 0.f};
        if (i < a.n && j < a.n) {
            const float *z = z2 + (size_t)(i * a.n + j) * 4;
            c3[0] = z[0]; c3[1] = z[1]; c3[2] = z[2];
            const double *T = a.T + (size_t)pr * 16;
            const double yaw = (double)c3[2] * (kPi / 180.0), c = cos(yaw), s = sin(yaw), x = c3[0], y = c3[1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {                                 // pose_to_tfm(corr) @ T: rows 0 and 1 mix, rows 2 and 3 pass through
                M[q] = c * T[q] - s * T[4 + q] + x * T[12 + q];
                M[4 + q] = s * T[q] + c * T[4 + q] + y * T[12 + q];
                M[8 + q] = T[8 + q];
                M[12 + q] = T[12 + q];
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) a.corr[(size_t)pr * 3 + q] = c3[q];
#pragma unroll
        for (int q = 0; q < 16; ++q) a.Tn[(size_t)pr * 16 + q] = M[q];
    }
}

// ---- (14e), (14f) -----------------------------------------------------------------------------------------------------------------------------------------
constexpr int kEmThreads = 64;

struct PoseArgs {
    const double *poses, *Tn;
    double *poses_out, *pairwise, *affine;
    double H, W, den_x, den_y;
    int n, L;
};

// pose [n][3] (x, y, yaw in degrees) in LDS -> the [L, L] pairwise matrices T_j^-1 T_i (closed form of two planar rigid transforms) and their normalised affines
__device__ void write_matrices(const PoseArgs &g, const double (*pose)[3], double (*cs)[2]) {
    const int t = threadIdx.x;
    if (t < g.n) {
        const double yaw = pose[t][2] * (kPi / 180.0);
        cs[t][0] = cos(yaw);
        cs[t][1] = sin(yaw);
    }
    __syncthreads();
    for (int pr = t; pr < g.L * g.L; pr += blockDim.x) {
        const int i = pr / g.L, j = pr - i * g.L;
        double M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (i < g.n && j < g.n && i != j) {
            const double ci = cs[i][0], si = cs[i][1], cj = cs[j][0], sj = cs[j][1], dx = pose[i][0] - pose[j][0], dy = pose[i][1] - pose[j][1];
            M[0] = cj * ci + sj * si;  M[1] = -cj * si + sj * ci;  M[3] = cj * dx + sj * dy;
            M[4] = -sj * ci + cj * si; M[5] = sj * si + cj * ci;   M[7] = -sj * dx + cj * dy;
        }
        double *pw = g.pairwise + (size_t)pr * 16, *af = g.affine + (size_t)pr * 6;
#pragma unroll
        for (int q = 0; q < 16; ++q) pw[q] = M[q];
        af[0] = M[0];                                 // normalize_pairwise_tfm (pose.py), the same operations in the same order
        af[1] = M[1] * g.H / g.W;
        af[2] = M[3] / g.den_x * 2;
        af[3] = M[4] * g.W / g.H;
        af[4] = M[5];
        af[5] = M[7] / g.den_y * 2;
    }
}

__global__ __launch_bounds__(kEmThreads) void pairwise_kernel(const PoseArgs g) {
    __shared__ double pose[kMaxAgents][3], cs[kMaxAgents][2];
    const int t = threadIdx.x;
    if (t < g.n)
        for (int q = 0; q < 3; ++q) pose[t][q] = g.poses[t * 3 + q];
    __syncthreads();
    write_matrices(g, pose, cs);
}

// inverse and determinant of a 4 x 4 matrix by cofactors: every index is a constant, the sixteen values live in registers
__device__ __forceinline__ double invert4(const double (&m)[16], double (&inv)[16]) {
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12], r = 1.0 / det;
#pragma unroll
    for (int q = 0; q < 16; ++q) inv[q] = inv[q] * r;
    return det;
}

__device__ __forceinline__ double quad4(const double (&S)[16], const double (&d)[4]) {      // d^T S d
    double q = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) q += d[r] * S[r * 4 + c] * d[c];
    return q;
}

// xycs of [[c, -s, x], [s, c, y]] @ A, A = (a00, a01, a03, a10, a11, a13) of a planar 4 x 4 matrix (tfm_to_xycs_torch: x, y, M00, M10)
__device__ __forceinline__ void compose_xycs(double c, double s, double x, double y, const double *A, double (&o)[4]) {
    o[0] = c * A[2] - s * A[5] + x;
    o[1] = s * A[2] + c * A[5] + y;
    o[2] = c * A[0] - s * A[3];
    o[3] = s * A[0] + c * A[3];
}

__device__ __forceinline__ void invert_planar(const double *B, double (&A)[6]) {      // the inverse of a planar rigid matrix: R^T | -R^T t
    A[0] = B[0]; A[1] = B[3]; A[3] = B[1]; A[4] = B[4];
    A[2] = -(B[0] * B[2] + B[3] * B[5]);
    A[5] = -(B[1] * B[2] + B[4] * B[5]);
}

__global__ __launch_bounds__(kEmThreads) void consistency_kernel(const PoseArgs g) {
    // the per-agent state lives in LDS: lanes index it by agent / sample, nothing indexed dynamically stays in registers
    __shared__ double pose[kMaxAgents][3], cs[kMaxAgents][2], A[kMaxAgents][kMaxAgents][6], Wt[kMaxAgents][kMaxAgents];
    __shared__ double S[kMaxAgents][kMaxSamples][4], ETA[kMaxAgents][kMaxSamples], MU[kMaxAgents][4], SI[kMaxAgents][16], LD[kMaxAgents];
    const int t = threadIdx.x, n = g.n, m = 2 * (n - 1);
    if (t < n) {
        for (int q = 0; q < 3; ++q) pose[t][q] = g.poses[t * 3 + q];
        const double yaw = pose[t][2] * (kPi / 180.0);
        cs[t][0] = cos(yaw);
        cs[t][1] = sin(yaw);
    }
    if (t < n * n) {
        const int i = t / n, j = t - i * n;
        const double *T = g.Tn + (size_t)(i * g.L + j) * 16;
        A[i][j][0] = T[0]; A[i][j][1] = T[1]; A[i][j][2] = T[3];
        A[i][j][3] = T[4]; A[i][j][4] = T[5]; A[i][j][5] = T[7];
        Wt[i][j] = 1.0;
    }
    __syncthreads();
    if (n > 1) {
        // the samples (WeightedMLE is called with the INPUT poses in every round: they never change)
        for (int e = t; e < n * m; e += kEmThreads) {
            const int i = e / m, s = e - i * m, kk = s < n - 1 ? s : s - (n - 1), k = kk < i ? kk : kk + 1;
            double R[6], o[4];
            if (s < n - 1) {
#pragma unroll
                for (int q = 0; q < 6; ++q) R[q] = A[i][k][q];
            } else {
                invert_planar(A[k][i], R);
            }
            compose_xycs(cs[k][0], cs[k][1], pose[k][0], pose[k][1], R, o);
#pragma unroll
            for (int q = 0; q < 4; ++q) S[i][s][q] = o[q];
        }
        __syncthreads();
        for (int round = 0; round < 10; ++round) {
            if (t < n) {                                                  // WeightedMLE of agent t
                double mu[4], Sg[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, Si[16];
#pragma unroll
                for (int d = 0; d < 4; ++d) {                             // torch.median over the samples: the lower median
                    double med = S[t][0][d];
                    for (int p = 0; p < m; ++p) {
                        const double v = S[t][p][d];
                        int rank = 0;
                        for (int q = 0; q < m; ++q) rank += (S[t][q][d] < v || (S[t][q][d] == v && q < p)) ? 1 : 0;
                        if (rank == (m - 1) / 2) med = v;
                    }
                    mu[d] = med;
                }
                for (int it = 0; it < 15; ++it) {
                    invert4(Sg, Si);
                    double num[4] = {0, 0, 0, 0}, den = 0.0;
                    for (int p = 0; p < m; ++p) {
                        const int kk = p < n - 1 ? p : p - (n - 1), k = kk < t ? kk : kk + 1;
                        double d[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) d[q] = mu[q] - S[t][p][q];
                        const double eta = 6.0 / (2.0 + quad4(Si, d)), we = Wt[t][k] * eta;
                        ETA[t][p] = eta;
#pragma unroll
                        for (int q = 0; q < 4; ++q) num[q] += we * S[t][p][q];
                        den += we;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) mu[q] = num[q] / den;
#pragma unroll
                    for (int q = 0; q < 16; ++q) Sg[q] = 0.0;
                    for (int p = 0; p < m; ++p) {
                        double d[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) d[q] = mu[q] - S[t][p][q];
                        const double eta = ETA[t][p];
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int c = 0; c < 4; ++c) Sg[r * 4 + c] += eta * d[r] * d[c];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) Sg[r * 4 + c] = Sg[r * 4 + c] / (double)m + (r == c ? 0.05 : 0.0);
                }
                const double det = invert4(Sg, Si);
#pragma unroll
                for (int q = 0; q < 16; ++q) SI[t][q] = Si[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) MU[t][q] = mu[q];
                LD[t] = log(det);
            }
            __syncthreads();
            if (t < n * n && t / n != t % n) {                            // update_weight of pair (i, j): log_t with df = 2, p = 4
                const int i = t / n, j = t - i * n;
                double Rinv[6], e1[4], e2[4], Si[16];
                compose_xycs(MU[j][2], MU[j][3], MU[j][0], MU[j][1], A[i][j], e1);
                invert_planar(A[i][j], Rinv);
                compose_xycs(MU[i][2], MU[i][3], MU[i][0], MU[i][1], Rinv, e2);
#pragma unroll
                for (int q = 0; q < 16; ++q) Si[q] = SI[i][q];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    e1[q] = e1[q] - MU[i][q];
                    e2[q] = e2[q] - MU[i][q];
                }
                const double base = log(2.0) - (2.0 * (log(2.0) + log(kPi)) + 0.5 * LD[i]);      // lgamma(3) - (lgamma(1) + p / 2 (log v + log pi) + logdet / 2)
                const double lt = (base - 3.0 * log(1.0 + quad4(Si, e1) / 2.0)) + (base - 3.0 * log(1.0 + quad4(Si, e2) / 2.0));
                Wt[i][j] = 120.0 * 0.01 / (120.0 - lt);                   // k * intersection / (k - sum log_t); the intersection is the constant 0.01
            }
            __syncthreads();
        }
        if (t < n) {
            pose[t][0] = MU[t][0];
            pose[t][1] = MU[t][1];
            pose[t][2] = atan2(MU[t][3], MU[t][2]) * (180.0 / kPi);
        }
        __syncthreads();
    }
    if (t < n)
        for (int q = 0; q < 3; ++q) g.poses_out[t * 3 + q] = pose[t][q];
    write_matrices(g, pose, cs);
}

// ---- (14g) ------------------------------------------------------------------------------------------------------------------------------------------------
struct AggArgs {
    const float *a, *e, *x, *weight;      // [R n, H, W, C], [R, H, W, C], [>= R, H, W, C], [.., L]
    const double *theta;
    void *out;                            // SplitMap [R, 2C, H, W] or float [R, H, W, C]
    int *range_flag;
    int n, R, C, H, W, L, out_kind;
};

__global__ __launch_bounds__(256) void aggregate_kernel(const AggArgs a) {
    const int HW = a.H * a.W, C = a.C, G = C / 8;
    Place p;
    if (!place(a.R, HW, p)) return;
    const int i = p.map, oy = p.pix / a.W, ox = p.pix - oy * a.W;
    const Geom geo{C, a.H, a.W, a.H, a.W};
    float mask[8], wt[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mask[j] = 0.f;
        wt[j] = 0.f;
        if (j < a.n) {
            const Taps t = make_taps(geo, a.theta, i * a.n + j, ox, oy);
            mask[j] = t.w00 + t.w01 + t.w10 + t.w11;      // the blend of a map of ones, left to right
            wt[j] = a.weight[i * a.L + j];
        }
    }
    const size_t plane = (size_t)HW * C;
    bool big = false;
    for (int g = p.g0; g < G; g += GL) {
        const size_t po = (size_t)p.pix * C + g * 8;
        float e[8], acc[8], xi[8];
        load8(a.e + i * plane + po, e);
        load8(a.x + i * plane + po, xi);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < a.n) {
                float m[8];
                load8(a.a + ((size_t)i * a.n + j) * plane + po, m);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    m[k] = ((m[k] + e[k]) * mask[j]) * wt[j];
                    acc[k] = j == 0 ? m[k] : acc[k] + m[k];
                }
            }
        if (a.out_kind == COALIGN_V2V_OUT_SP) {
            uint4 *y = static_cast<uint4 *>(a.out);
            big = store_split8(y, i, C / 8, g, HW, p.pix, xi, p.live) || big;               // channels [0, C): x_i
            big = store_split8(y, i, C / 8, G + g, HW, p.pix, acc, p.live) || big;          // channels [C, 2C): agg_i
        } else if (p.live) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = xi[k] + acc[k];
            store8(static_cast<float *>(a.out) + i * plane + po, acc);
        }
    }
    if (a.range_flag && big) atomicOr(a.range_flag, 1);
}


int check_agents(int n, int L) {
    if (n < 1 || L < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > kMaxAgents || L > kMaxCav) return COALIGN_ERR_UNSUPPORTED;
    if (L < n) return COALIGN_ERR_BAD_SHAPE;
    return COALIGN_OK;
}

}  // namespace

extern "C" int coalign_v2vr_pool_act(const float *a_, const float *e, int P, int n, int C, int H, int W, int out_kind, void *out, int32_t *range_flag, void *stream) {
    if (P < 0 || C < 1 || H < 2 || W < 2) return COALIGN_ERR_BAD_SHAPE;
    if (e && (n < 1 || P % n)) return COALIGN_ERR_BAD_SHAPE;
    if (C % 16 || (out_kind != COALIGN_V2V_OUT_NHWC && out_kind != COALIGN_V2V_OUT_SP)) return COALIGN_ERR_UNSUPPORTED;
    if (P == 0) return COALIGN_OK;
    if ((long long)C * H * W * P > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!a_ || !out) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(a_, 15) || misaligned(e, 15) || misaligned(out, 15) || misaligned(range_flag, 3)) return COALIGN_ERR_UNSUPPORTED;
    PoolArgs a;
    a.a = a_; a.e = e; a.out = out; a.range_flag = out_kind == COALIGN_V2V_OUT_SP ? range_flag : nullptr;
    a.P = P; a.n = e ? n : 1; a.C = C; a.H = H; a.W = W; a.out_kind = out_kind;
    hipLaunchKernelGGL(pool_act_kernel, dim3(blocks_of(P, H / 2, W / 2)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}

extern "C" int coalign_v2vr_score_head(const float *y, int n, int L, int h, int H, int W, const float *w, const float *b, const float *alpha, float *scores,
                                       float *weight, void *stream) {
    const int rc = check_agents(n, L);
    if (rc != COALIGN_OK) return rc;
    if (h < 1 || H < 2 || W < 2) return COALIGN_ERR_BAD_SHAPE;
    if (h % 64 || h > 1024) return COALIGN_ERR_UNSUPPORTED;
    if ((long long)h * H * W * n * n > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!y || !w || !b || !alpha || !scores || !weight) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(y, 15) || misaligned(w, 15) || misaligned(b, 3) || misaligned(alpha, 3) || misaligned(scores, 3) || misaligned(weight, 3)) return COALIGN_ERR_UNSUPPORTED;
    const ScoreArgs a{y, w, b, alpha, scores, weight, n, L, h, H, W};
    hipLaunchKernelGGL(score_kernel, dim3(L * L), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    int st = coalign::check_launch();
    if (st != COALIGN_OK) return st;
    hipLaunchKernelGGL(score_weight_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}

extern "C" size_t coalign_v2vr_pose_head_workspace_bytes(int n, int h) {
    if (n < 1 || n > kMaxAgents || h < 1 || h > 1024) return 0;
    return ((size_t)2 * n * n * h + (size_t)4 * n * n) * sizeof(float);
}

extern "C" int coalign_v2vr_pose_head(const void *y4_sp, int n, int L, int h, int H4, int W4, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                                      const float *fc2_b, const float *fc3_w, const float *fc3_b, const double *T, float *pose_corr, double *T_new, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    const int rc = check_agents(n, L);
    if (rc != COALIGN_OK) return rc;
    if (h < 1 || H4 < 2 || W4 < 2) return COALIGN_ERR_BAD_SHAPE;
    if (h % 64 || h > 1024) return COALIGN_ERR_UNSUPPORTED;
    if ((long long)h * H4 * W4 * n * n > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!y4_sp || !fc1_w || !fc1_b || !fc2_w || !fc2_b || !fc3_w || !fc3_b || !T || !pose_corr || !T_new || !workspace) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(y4_sp, 15) || misaligned(fc1_w, 15) || misaligned(fc2_w, 15) || misaligned(fc3_w, 15) || misaligned(workspace, 15) || misaligned(fc1_b, 3) || misaligned(fc2_b, 3) ||
        misaligned(fc3_b, 3) || misaligned(T, 7) || misaligned(T_new, 7) || misaligned(pose_corr, 3))
        return COALIGN_ERR_UNSUPPORTED;
    if (workspace_bytes < coalign_v2vr_pose_head_workspace_bytes(n, h)) return COALIGN_ERR_WORKSPACE;
    const HeadArgs a{static_cast<const _Float16 *>(y4_sp), fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b, T, pose_corr, static_cast<float *>(workspace), T_new, n, L, h, H4, W4};
    hipLaunchKernelGGL(pose_head_kernel, dim3(1), dim3(kHeadThreads), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}

static int check_pose_args(int n, int L, int H, int W, double den_x, double den_y) {
    const int rc = check_agents(n, L);
    if (rc != COALIGN_OK) return rc;
    if (H < 1 || W < 1 || !(den_x > 0) || !(den_y > 0)) return COALIGN_ERR_BAD_SHAPE;
    return COALIGN_OK;
}

extern "C" int coalign_v2vr_pairwise(const double *poses, int n, int L, int H, int W, double den_x, double den_y, double *pairwise, double *affine, void *stream) {
    const int rc = check_pose_args(n, L, H, W, den_x, den_y);
    if (rc != COALIGN_OK) return rc;
    if (!poses || !pairwise || !affine) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(poses, 7) || misaligned(pairwise, 7) || misaligned(affine, 7)) return COALIGN_ERR_UNSUPPORTED;
    const PoseArgs g{poses, nullptr, nullptr, pairwise, affine, (double)H, (double)W, den_x, den_y, n, L};
    hipLaunchKernelGGL(pairwise_kernel, dim3(1), dim3(kEmThreads), 0, static_cast<hipStream_t>(stream), g);
    return coalign::check_launch();
}

extern "C" int coalign_v2vr_consistency(const double *poses, const double *T_new, int n, int L, int H, int W, double den_x, double den_y, double *poses_out,
                                        double *pairwise, double *affine, void *stream) {
    const int rc = check_pose_args(n, L, H, W, den_x, den_y);
    if (rc != COALIGN_OK) return rc;
    if (!poses || !T_new || !poses_out || !pairwise || !affine) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(poses, 7) || misaligned(T_new, 7) || misaligned(poses_out, 7) || misaligned(pairwise, 7) || misaligned(affine, 7)) return COALIGN_ERR_UNSUPPORTED;
    const PoseArgs g{poses, T_new, poses_out, pairwise, affine, (double)H, (double)W, den_x, den_y, n, L};
    hipLaunchKernelGGL(consistency_kernel, dim3(1), dim3(kEmThreads), 0, static_cast<hipStream_t>(stream), g);
    return coalign::check_launch();
}

extern "C" int coalign_v2vr_aggregate(const float *a_, const float *e, const float *x, int n, int R, int C, int H, int W, const double *theta, const float *weight, int L,
                                      int out_kind, void *out, int32_t *range_flag, void *stream) {
    if (n < 0 || R < 0 || C < 1 || H < 1 || W < 1 || L < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > kMaxAgents || L > kMaxCav || C % 16 || (out_kind != COALIGN_V2V_OUT_NHWC && out_kind != COALIGN_V2V_OUT_SP)) return COALIGN_ERR_UNSUPPORTED;
    if (R > n || L < n) return COALIGN_ERR_BAD_SHAPE;
    if (n == 0 || R == 0) return COALIGN_OK;
    if ((long long)C * H * W * R * n > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!a_ || !e || !x || !theta || !weight || !out) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(a_, 15) || misaligned(e, 15) || misaligned(x, 15) || misaligned(out, 15) || misaligned(theta, 7) || misaligned(weight, 3) || misaligned(range_flag, 3))
        return COALIGN_ERR_UNSUPPORTED;
    AggArgs a;
    a.a = a_; a.e = e; a.x = x; a.weight = weight; a.theta = theta; a.out = out; a.range_flag = out_kind == COALIGN_V2V_OUT_SP ? range_flag : nullptr;
    a.n = n; a.R = R; a.C = C; a.H = H; a.W = W; a.L = L; a.out_kind = out_kind;
    hipLaunchKernelGGL(aggregate_kernel, dim3(blocks_of(R, H, W)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}
