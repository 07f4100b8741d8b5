// Lift-Splat's frustum pooling, gfx950: camera features x depth distribution summed into the BEV cells, through an inverted index instead of the reference's
// materialised outer product, argsort and running-sum difference (lss_submodule.py:134-136, lift_splat_shoot.py:116-169).
//
//   lss_cells       once per camera rig: the voxel of every frustum point, a float64 evaluation of get_geometry (lift_splat_shoot.py:80-102) and of voxel_pooling's
//                   index line and bounds test (:126, :133-135).  A workgroup belongs to one camera: its first lane inverts post_rots and intrins by their adjugates
//                   into LDS, every lane then takes one point.
//   lss_depth_prob  per frame: softmax over the D depth bins of a pixel, written pixel-major ([pixels, D]) so that a point's probability is one indexed float.
//   lss_pool        per frame: one wavefront per output cell, lanes across the C channels (float2 per lane at C = 128).  The wavefront loads 64 index entries
//                   with one coalesced load and their 64 probabilities with one gather, then walks them with v_readlane, eight feature rows in flight, adding in
//                   list order.  Cells whose list is longer than COALIGN_LSS_CHUNK are left to the workgroups in FRONT of the grid (they start first: the longest
//                   work is not the tail): four wavefronts take chunks of 512 points, a chunk's sum goes to LDS, wavefront 0 adds the sums in chunk order.
//                   Every cell's row is written, zeros for an empty list; the output is channels-last, so a row is one contiguous store.
// The index is built on the host side of the ABI (coalign_amd.ops.build_lss_index).  No workspace, no atomics, no environment variable.
#include "common.h"

#include "coalign_amd_lss.h"

namespace {

using coalign::misaligned;
constexpr int CHUNK = COALIGN_LSS_CHUNK;

struct CellArgs {
    const float *rots, *trans, *intrins, *post_rots, *post_trans, *xs, *ys, *ds;
    int *cell;
    double lower[3], dx[3];
    int cams, N, D, fH, fW, nx, ny, nz, blocks_per_cam;
};

__device__ __forceinline__ void inverse3(const double *a, double *o) {      // adjugate / determinant: a singular matrix gives inf / NaN, which drops its points
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    o[0] = c00 / det; o[1] = (a[2] * a[7] - a[1] * a[8]) / det; o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = c01 / det; o[4] = (a[0] * a[8] - a[2] * a[6]) / det; o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = c02 / det; o[7] = (a[1] * a[6] - a[0] * a[7]) / det; o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

__global__ __launch_bounds__(256) void lss_cells(const CellArgs a) {
    __shared__ double undo[9], comb[9], shift[6];
    const int m = blockIdx.x / a.blocks_per_cam;               // < cams
    if (threadIdx.x == 0) {
        double pr[9], in[9], iin[9];
        for (int k = 0; k < 9; ++k) {
            pr[k] = (double)a.post_rots[(size_t)m * 9 + k];
            in[k] = (double)a.intrins[(size_t)m * 9 + k];
        }
        inverse3(pr, undo);
        inverse3(in, iin);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
                for (int k = 0; k < 3; ++k) s += (double)a.rots[(size_t)m * 9 + r * 3 + k] * iin[k * 3 + c];
                comb[r * 3 + c] = s;
            }
        for (int k = 0; k < 3; ++k) {
            shift[k] = (double)a.post_trans[(size_t)m * 3 + k];
            shift[3 + k] = (double)a.trans[(size_t)m * 3 + k];
        }
    }
    __syncthreads();
    const int per = a.D * a.fH * a.fW;
    const int i = (blockIdx.x - m * a.blocks_per_cam) * 256 + threadIdx.x;
    if (i >= per) return;
    const int w = i % a.fW, t = i / a.fW, h = t % a.fH, d = t / a.fH;
    const double f0 = (double)a.xs[w] - shift[0], f1 = (double)a.ys[h] - shift[1], f2 = (double)a.ds[d] - shift[2];
    double q0 = undo[0] * f0 + undo[1] * f1 + undo[2] * f2, q1 = undo[3] * f0 + undo[4] * f1 + undo[5] * f2;
    const double q2 = undo[6] * f0 + undo[7] * f1 + undo[8] * f2;
    q0 *= q2;
    q1 *= q2;
    const double g[3] = {comb[0] * q0 + comb[1] * q1 + comb[2] * q2 + shift[3], comb[3] * q0 + comb[4] * q1 + comb[5] * q2 + shift[4],
                         comb[6] * q0 + comb[7] * q1 + comb[8] * q2 + shift[5]};
    const int n[3] = {a.nx, a.ny, a.nz};
    int idx[3];
    bool kept = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = (g[k] - a.lower[k]) / a.dx[k];
        const bool ok = fabs(v) < 2147483648.0;                // false for NaN and for +-inf as well
        idx[k] = ok ? (int)v : -1;                             // the conversion truncates towards zero, like .long()
        kept = kept && ok && idx[k] >= 0 && idx[k] < n[k];
    }
    a.cell[(size_t)m * per + i] = kept ? (idx[2] * a.ny + idx[1]) * a.nx + idx[0] : -1;
}

struct ProbArgs {
    const float *logit;
    float *prob;
    int pixels, hw, D, channels_last;
};

__global__ __launch_bounds__(256) void lss_depth_prob(const ProbArgs a) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.pixels) return;
    const int m = pix / a.hw, p = pix - m * a.hw;
    const float *src = a.logit + (a.channels_last ? (size_t)pix * a.D : (size_t)m * a.D * a.hw + p);
    const size_t step = a.channels_last ? 1 : (size_t)a.hw;
    float mx = src[0];
    for (int d = 1; d < a.D; ++d) mx = fmaxf(mx, src[d * step]);
    float s = 0.f;
    for (int d = 0; d < a.D; ++d) s += __expf(src[d * step] - mx);
    float *dst = a.prob + (size_t)pix * a.D;
    for (int d = 0; d < a.D; ++d) dst[d] = __expf(src[d * step] - mx) / s;
}

struct PoolArgs {
    const float *x;          // [rows, C]
    const float *prob;       // [rows * D]
    const int2 *points;      // [n_points] (row, prob)
    const int *starts;       // [cells + 1]
    const int *long_cells;   // [n_long]
    float *out;              // [cells, C]
    int rows, prob_len, n_points, cells, n_long;
};

template <int C>
struct Row {                 // a lane's share of a C-channel row: two floats at C = 128, one at C = 64
    float v0, v1;
};

template <int C>
__device__ __forceinline__ Row<C> load_row(const float *x, int r, int lane) {
    Row<C> o;
    if constexpr (C == 128) {
        const float2 v = *reinterpret_cast<const float2 *>(x + (size_t)r * C + 2 * lane);
        o.v0 = v.x; o.v1 = v.y;
    } else {
        o.v0 = x[(size_t)r * C + lane]; o.v1 = 0.f;
    }
    return o;
}

template <int C>
__device__ __forceinline__ void store_row(float *dst, int lane, float v0, float v1) {
    if constexpr (C == 128) *reinterpret_cast<float2 *>(dst + 2 * lane) = make_float2(v0, v1);
    else dst[lane] = v0;
}

__device__ __forceinline__ float lane_value(float v, int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j)); }

// points [b, e) of the index, added in list order to (s0, s1); b, e wave-uniform
template <int C>
__device__ __forceinline__ void sum_points(const PoolArgs &a, int b, int e, int lane, float &s0, float &s1) {
    for (int i = b; i < e; i += 64) {
        const int cnt = min(64, e - i);
        int row = 0;
        float pv = 0.f;
        bool ok = false, outside = false;
        if (lane < cnt) {
            const int2 pt = a.points[i + lane];
            ok = (unsigned)pt.x < (unsigned)a.rows && (unsigned)pt.y < (unsigned)a.prob_len;
            outside = !ok;
            row = ok ? pt.x : 0;
            pv = ok ? a.prob[pt.y] : 0.f;
        }
        if (__builtin_amdgcn_ballot_w64(outside)) {            // an entry outside the buffers (an inconsistent index): it is SKIPPED -- not 0 x row 0, which is NaN when
            unsigned long long take = __builtin_amdgcn_ballot_w64(ok);
            while (take) {                                     // that row holds inf or NaN; the entries that are left are added one by one, in the same order
                const int j = __builtin_ctzll(take);
                take &= take - 1;
                const Row<C> v = load_row<C>(a.x, __builtin_amdgcn_readlane(row, j), lane);
                const float pw = lane_value(pv, j);
                s0 = fmaf(pw, v.v0, s0);
                if constexpr (C == 128) s1 = fmaf(pw, v.v1, s1);
            }
            continue;
        }
        int j = 0;
        for (; j + 8 <= cnt; j += 8) {
            Row<C> v[8];
            float pw[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u] = load_row<C>(a.x, __builtin_amdgcn_readlane(row, j + u), lane);
                pw[u] = lane_value(pv, j + u);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s0 = fmaf(pw[u], v[u].v0, s0);
                if constexpr (C == 128) s1 = fmaf(pw[u], v[u].v1, s1);
            }
        }
        for (; j < cnt; ++j) {
            const Row<C> v = load_row<C>(a.x, __builtin_amdgcn_readlane(row, j), lane);
            const float pw = lane_value(pv, j);
            s0 = fmaf(pw, v.v0, s0);
            if constexpr (C == 128) s1 = fmaf(pw, v.v1, s1);
        }
    }
}

// the list of key k, clamped into the index: (begin, end), empty for anything inconsistent
__device__ __forceinline__ void list_of(const PoolArgs &a, int k, int &b, int &e) {
    b = __builtin_amdgcn_readfirstlane(a.starts[k]);
    e = __builtin_amdgcn_readfirstlane(a.starts[k + 1]);
    if (b < 0 || e > a.n_points || e < b) b = e = 0;
}

template <int C>
__global__ __launch_bounds__(256) void lss_pool(const PoolArgs a) {
    __shared__ float part[4][C];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)blockIdx.x >= a.n_long) {                         // one wavefront per cell
        const long long k64 = ((long long)blockIdx.x - a.n_long) * 4 + wave;
        if (k64 >= a.cells) return;
        const int k = (int)k64;
        int b, e;
        list_of(a, k, b, e);
        if (e - b > CHUNK) return;                             // a workgroup in front of the grid owns it
        float s0 = 0.f, s1 = 0.f;
        sum_points<C>(a, b, e, lane, s0, s1);
        store_row<C>(a.out + (size_t)k * C, lane, s0, s1);
        return;
    }
    const int k = __builtin_amdgcn_readfirstlane(a.long_cells[blockIdx.x]);
    if ((unsigned)k >= (unsigned)a.cells) return;              // (the whole workgroup alike)
    int b, e;
    list_of(a, k, b, e);
    if (e - b <= CHUNK) return;                                // (not a long list after all: its own wavefront wrote it)
    const int chunks = (e - b + CHUNK - 1) / CHUNK;
    float t0 = 0.f, t1 = 0.f;
    for (int c0 = 0; c0 < chunks; c0 += 4) {
        const int c = c0 + wave;
        float s0 = 0.f, s1 = 0.f;
        if (c < chunks) sum_points<C>(a, b + c * CHUNK, min(e, b + (c + 1) * CHUNK), lane, s0, s1);
        store_row<C>(part[wave], lane, s0, s1);
        __syncthreads();
        if (wave == 0) {
            const int have = min(4, chunks - c0);
            for (int w = 0; w < have; ++w) {                   // chunk order
                if constexpr (C == 128) {
                    t0 += part[w][2 * lane];
                    t1 += part[w][2 * lane + 1];
                } else {
                    t0 += part[w][lane];
                }
            }
        }
        __syncthreads();
    }
    if (wave == 0) store_row<C>(a.out + (size_t)k * C, lane, t0, t1);
}

bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int coalign_lss_cells(const float *rots, const float *trans, const float *intrins, const float *post_rots, const float *post_trans, int A, int N,
                                 const float *xs, const float *ys, const float *ds, int D, int fH, int fW, float lower_x, float lower_y, float lower_z, float dx_x,
                                 float dx_y, float dx_z, int nx, int ny, int nz, int *cell, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (A < 1 || N < 1 || D < 1 || fH < 1 || fW < 1 || nx < 1 || ny < 1 || nz < 1) return COALIGN_ERR_BAD_SHAPE;
    if ((size_t)A * (size_t)N * (size_t)D * (size_t)fH * (size_t)fW > (size_t)INT32_MAX || (size_t)nx * (size_t)ny * (size_t)nz > (size_t)INT32_MAX)
        return COALIGN_ERR_BAD_SHAPE;
    if (!(dx_x > 0.f && dx_y > 0.f && dx_z > 0.f) || !finite_f(dx_x) || !finite_f(dx_y) || !finite_f(dx_z) || !finite_f(lower_x) || !finite_f(lower_y) || !finite_f(lower_z))
        return COALIGN_ERR_BAD_SHAPE;
    const void *ptrs[] = {rots, trans, intrins, post_rots, post_trans, xs, ys, ds, cell};
    for (const void *p : ptrs)
        if (!p || misaligned(p, 3)) return COALIGN_ERR_NULL_POINTER;
    CellArgs a;
    a.rots = rots; a.trans = trans; a.intrins = intrins; a.post_rots = post_rots; a.post_trans = post_trans; a.xs = xs; a.ys = ys; a.ds = ds; a.cell = cell;
    a.lower[0] = (double)lower_x; a.lower[1] = (double)lower_y; a.lower[2] = (double)lower_z;
    a.dx[0] = (double)dx_x; a.dx[1] = (double)dx_y; a.dx[2] = (double)dx_z;
    a.cams = A * N; a.N = N; a.D = D; a.fH = fH; a.fW = fW; a.nx = nx; a.ny = ny; a.nz = nz;
    a.blocks_per_cam = (D * fH * fW + 255) / 256;
    if ((size_t)a.cams * (size_t)a.blocks_per_cam > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(lss_cells, dim3((unsigned)(a.cams * a.blocks_per_cam)), dim3(256), 0, stream, a);
    return coalign::check_launch();
}

extern "C" int coalign_lss_depth_prob(const float *depth_logit, int M, int D, int fH, int fW, int channels_last, float *prob, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || fH < 0 || fW < 0 || D < 1) return COALIGN_ERR_BAD_SHAPE;
    if (D > COALIGN_LSS_MAX_DEPTH || (channels_last != 0 && channels_last != 1)) return COALIGN_ERR_UNSUPPORTED;
    if ((size_t)M * (size_t)fH * (size_t)fW * (size_t)D > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    const int pixels = M * fH * fW;
    if (pixels == 0) return COALIGN_OK;
    if (!depth_logit || !prob || misaligned(depth_logit, 3) || misaligned(prob, 3)) return COALIGN_ERR_NULL_POINTER;
    ProbArgs a;
    a.logit = depth_logit; a.prob = prob; a.pixels = pixels; a.hw = fH * fW; a.D = D; a.channels_last = channels_last;
    hipLaunchKernelGGL(lss_depth_prob, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, a);
    return coalign::check_launch();
}

extern "C" int coalign_lss_pool(const float *x_rows, const float *prob, int rows, int C, int D, const int *points, int n_points, const int *starts, int cells,
                                const int *long_cells, int n_long, float *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (rows < 0 || n_points < 0 || cells < 0 || n_long < 0 || n_long > cells || D < 1 || C < 1) return COALIGN_ERR_BAD_SHAPE;
    if ((C != 64 && C != 128) || D > COALIGN_LSS_MAX_DEPTH) return COALIGN_ERR_UNSUPPORTED;
    if ((size_t)rows * (size_t)D > (size_t)INT32_MAX || (n_points > 0 && rows == 0)) return COALIGN_ERR_BAD_SHAPE;
    if (cells == 0) return COALIGN_OK;
    if (!out || !starts || misaligned(out, 15) || misaligned(starts, 3)) return COALIGN_ERR_NULL_POINTER;
    if (n_points > 0 && (!x_rows || !prob || !points || misaligned(x_rows, 15) || misaligned(prob, 3) || misaligned(points, 7))) return COALIGN_ERR_NULL_POINTER;
    if (n_long > 0 && (!long_cells || misaligned(long_cells, 3))) return COALIGN_ERR_NULL_POINTER;
    const size_t blocks = (size_t)n_long + ((size_t)cells + 3) / 4;
    if (blocks > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    PoolArgs a;
    a.x = x_rows; a.prob = prob; a.points = reinterpret_cast<const int2 *>(points); a.starts = starts; a.long_cells = long_cells; a.out = out;
    a.rows = rows; a.prob_len = rows * D; a.n_points = n_points; a.cells = cells; a.n_long = n_long;
    if (C == 128) hipLaunchKernelGGL(lss_pool<128>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(lss_pool<64>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return coalign::check_launch();
}
