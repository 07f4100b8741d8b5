// Anchor decode: sigmoid + threshold + box decode + direction fix + corners + projection + sanity filters,
// order-preserving compaction without atomics (deterministic), gfx950.
//
// Reference semantics (see include/coalign_amd.h): VoxelPostprocessor.post_process
// (opencood/data_utils/post_processor/voxel_postprocessor.py:275-377) and the box_utils helpers it calls.
// The reference runs ~40 tiny PyTorch ops plus boolean-mask compactions here; this is two launches:
//   count_kernel  one thread per anchor, sigmoid(cls) > thr, per-block popcounts
//   emit_kernel   same predicate, block offset = sum of the preceding block counts, wave-ballot prefix inside
//                 the block -> the candidate list keeps the reference's flat (h, w, anchor) order; only the
//                 passing anchors (a few %) run the full decode.
// The file is compiled with -ffp-contract=off: every a*b+c below rounds twice, like the op-by-op float32
// evaluation of the reference.
// Non-finite values: the reference takes the corner extents with torch.max / torch.min, which propagate NaN, and every
// comparison with NaN is false -- a candidate with a NaN corner coordinate fails its filters.  fminf / fmaxf return the
// non-NaN operand instead, so the NaN test is explicit: cand_keep = 0 whenever any projected corner coordinate is NaN (a
// NaN delta; a size delta above 88.72, where expf overflows and the transform's zeros give 0 * inf).  The row is still
// written and counted.  Infinite extents need nothing extra: inf - (-inf) = inf and inf - inf = NaN both fail "<= 6".
#include "common.h"
#include "stage1_internal.h"

namespace {

constexpr int kBlock = 256;

struct DecodeArgs {
    const float *cls, *reg, *dir, *anchors, *T;
    int A, HW, nb, total, hwl, capacity;
    float thr, dir_offset;
    const int *count_in;
    int *count_out, *cand_index;
    float *cand_score, *cand_box7, *cand_corners;
    uint8_t *cand_keep;
    uint32_t *status;
    int *block_counts;
    uint32_t *clear;          // round 6: the frame's counters / status words, zeroed by the FIRST decode launch of a frame (no fill launch of their own)
    int n_clear;
};

// Correctly rounded float32 sigmoid (evaluated in float64): the value every faithful float32 implementation
// (the reference's vectorised CPU one included) is within an ulp or two of.
__device__ __forceinline__ float sigmoid_f32(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

__device__ __forceinline__ bool passes(const DecodeArgs &a, int i, float &prob) {
    const int hw = i / a.A, an = i - hw * a.A;
    prob = sigmoid_f32(a.cls[(size_t)an * a.HW + hw]);
    return prob > a.thr;
}

__device__ __forceinline__ float limit_period(float v, float offset, float period) {
    return v - floorf(v / period + offset) * period;  // common_utils.py:70-79
}

__device__ void decode_and_store(const DecodeArgs &a, int i, float prob, int pos) {
    const int hw = i / a.A, an = i - hw * a.A;
    float d[7], r[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        d[k] = a.reg[(size_t)(an * 7 + k) * a.HW + hw];
        r[k] = a.anchors[(size_t)i * 7 + k];
    }
    // delta_to_boxes3d, voxel_postprocessor.py:405-450
    const float diag = sqrtf(r[4] * r[4] + r[5] * r[5]);
    float b[7];
    b[0] = d[0] * diag + r[0];
    b[1] = d[1] * diag + r[1];
    b[2] = d[2] * r[3] + r[2];
    b[3] = expf(d[3]) * r[3];
    b[4] = expf(d[4]) * r[4];
    b[5] = expf(d[5]) * r[5];
    b[6] = d[6] + r[6];
    if (a.dir) {  // direction-bin correction, voxel_postprocessor.py:317-333
        int label = 0;
        float best = a.dir[(size_t)(an * a.nb) * a.HW + hw];
        for (int q = 1; q < a.nb; ++q) {
            const float v = a.dir[(size_t)(an * a.nb + q) * a.HW + hw];
            if (v > best) { best = v; label = q; }
        }
        const float period = (float)(2.0 * M_PI / a.nb);
        const float rot = limit_period(b[6] - a.dir_offset, 0.f, period);
        b[6] = (rot + a.dir_offset) + period * (float)label;
        b[6] = limit_period(b[6], 0.5f, (float)(2.0 * M_PI));
    }
    // boxes_to_corners_3d, box_utils.py:152-204: (l, w, h) scaled +-1/2 template, rotate about z, add centre
    const float L = a.hwl ? b[5] : b[3], Wd = b[4], Hh = a.hwl ? b[3] : b[5];
    const float ca = cosf(b[6]), sa = sinf(b[6]);
    const float sx[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sy[8] = {-1, 1, 1, -1, -1, 1, 1, -1}, sz[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
    float T[12];
    if (a.T) {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = a.T[k];
    }
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, zmin = INFINITY, zmax = -INFINITY;
    bool ordered = true;      // no NaN among the 24 projected coordinates
    float *co = a.cand_corners + (size_t)pos * 24;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float lx = L * (sx[k] / 2), ly = Wd * (sy[k] / 2), lz = Hh * (sz[k] / 2);
        float X = (lx * ca + ly * (-sa)) + b[0];
        float Y = (lx * sa + ly * ca) + b[1];
        float Z = lz + b[2];
        if (a.T) {  // project_box3d, box_utils.py:278-316
            const float px = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
            const float py = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
            const float pz = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
            X = px; Y = py; Z = pz;
        }
        co[3 * k] = X; co[3 * k + 1] = Y; co[3 * k + 2] = Z;
        ordered = ordered && (X == X) && (Y == Y) && (Z == Z);
        xmin = fminf(xmin, X); xmax = fmaxf(xmax, X);
        ymin = fminf(ymin, Y); ymax = fmaxf(ymax, Y);
        zmin = fminf(zmin, Z); zmax = fmaxf(zmax, Z);
    }
    // remove_large_pred_bbx (box_utils.py:840-869, its "z_len" is the y extent used as a truthy mask) and
    // remove_bbx_abnormal_z (:872-890)
    const float x_len = xmax - xmin, y_len = ymax - ymin;
    const bool keep = ordered && (x_len <= 6.f) && (y_len <= 6.f) && (y_len != 0.f) && (zmin >= -3.f) && (zmax <= 1.f);
    a.cand_keep[pos] = keep ? 1 : 0;
    a.cand_score[pos] = prob;
    if (a.cand_index) a.cand_index[pos] = i;
    if (a.cand_box7) {
#pragma unroll
        for (int k = 0; k < 7; ++k) a.cand_box7[(size_t)pos * 7 + k] = b[k];
    }
}

// One block's share of the count pass: thread -> anchor `i` of the head maps in `a` (i >= a.total: none), the block's popcount to *out.
__device__ __forceinline__ void count_block(const DecodeArgs &a, int i, int *out) {
    __shared__ int wave_cnt[kBlock / 64];
    float p;
    const bool ok = i < a.total && passes(a, i, p);
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kBlock / 64; ++w) s += wave_cnt[w];
        *out = s;
    }
}

// Candidates emitted by the blocks in front of this one (`before`) and by all `nblocks` blocks (`all`), to every thread of the block.
__device__ __forceinline__ void block_prefix(const int *block_counts, int nblocks, int self, int &before_out, int &all_out) {
    __shared__ int wave_cnt[kBlock / 64];
    __shared__ int red[kBlock / 64];
    __shared__ int s_before, s_all;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int before = 0, all = 0;
    for (int bq = threadIdx.x; bq < nblocks; bq += kBlock) {
        const int c = block_counts[bq];
        all += c;
        if (bq < self) before += c;
    }
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
    if (lane == 0) { wave_cnt[wv] = before; red[wv] = all; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sb = 0, sa = 0;
        for (int w = 0; w < kBlock / 64; ++w) { sb += wave_cnt[w]; sa += red[w]; }
        s_before = sb; s_all = sa;
    }
    __syncthreads();
    before_out = s_before; all_out = s_all;
}

// One block's share of the emit pass: the same predicate as count_block, the passing anchors decoded to rows base, base + 1, ... in thread order.
__device__ __forceinline__ void emit_block(const DecodeArgs &a, int i, int base) {
    __shared__ int wave_cnt[kBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float p = 0.f;
    const bool ok = i < a.total && passes(a, i, p);
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_cnt[wv] = __popcll(m);
    __syncthreads();
    int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) pos += wave_cnt[w];
    if (ok && pos < a.capacity) decode_and_store(a, i, p, pos);
}

__global__ __launch_bounds__(kBlock) void count_kernel(DecodeArgs a) {
    if (blockIdx.x == 0 && (int)threadIdx.x < a.n_clear) a.clear[threadIdx.x] = 0u;      // (nothing of this launch reads them; emit_kernel, the next launch, does)
    count_block(a, blockIdx.x * kBlock + threadIdx.x, a.block_counts + blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void emit_kernel(DecodeArgs a) {
    // candidates emitted by earlier blocks (and, in the last block, by everybody: the new total)
    int before, all;
    block_prefix(a.block_counts, (int)gridDim.x, (int)blockIdx.x, before, all);
    const int start = a.count_in ? *a.count_in : 0;
    const int base = start + before;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const long tot = (long)start + all;
        *a.count_out = (int)(tot < a.capacity ? tot : a.capacity);
        if (tot > a.capacity && a.status) atomicOr(a.status, COALIGN_FLAG_CANDIDATE_OVERFLOW);
    }
    __syncthreads();
    emit_block(a, blockIdx.x * kBlock + threadIdx.x, base);
}

// ---- stage 1 of ALL agents in one pass (include/coalign_amd_stage1.h): the two kernels above with an agent dimension.  Agent g owns the `bpa` consecutive blocks
// g * bpa ..: no block straddles two agents, and the chained block offsets make agent g's candidates ONE contiguous segment [seg_start[g], seg_start[g + 1]) of
// the candidate buffer, in the agent's own (h, w, anchor) order -- row for row what a decode call on that agent alone leaves at rows 0 ...
struct SegArgs {
    int n_agents, bpa;
    size_t cls_stride, reg_stride, dir_stride;      // floats between two agents' head maps
    int *seg_start;                                 // [n_agents + 1]
};

__device__ __forceinline__ DecodeArgs agent_args(DecodeArgs a, const SegArgs &s, int agent) {
    a.cls += (size_t)agent * s.cls_stride;
    a.reg += (size_t)agent * s.reg_stride;
    if (a.dir) a.dir += (size_t)agent * s.dir_stride;
    return a;
}

__global__ __launch_bounds__(kBlock) void count_seg_kernel(DecodeArgs a, SegArgs s) {
    const int agent = blockIdx.x / s.bpa, lb = blockIdx.x - agent * s.bpa;
    if (blockIdx.x == 0 && (int)threadIdx.x < a.n_clear) a.clear[threadIdx.x] = 0u;      // the store's status word (the last launch of the pass ORs into it)
    count_block(agent_args(a, s, agent), lb * kBlock + threadIdx.x, a.block_counts + blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void emit_seg_kernel(DecodeArgs a, SegArgs s) {
    const int agent = blockIdx.x / s.bpa, lb = blockIdx.x - agent * s.bpa;
    int before, all;
    block_prefix(a.block_counts, (int)gridDim.x, (int)blockIdx.x, before, all);
    if (threadIdx.x == 0) {
        if (lb == 0) s.seg_start[agent] = before;
        if (blockIdx.x == gridDim.x - 1) s.seg_start[s.n_agents] = all;
    }
    emit_block(agent_args(a, s, agent), lb * kBlock + threadIdx.x, before);
}

}  // namespace

size_t coalign::stage1_decode_blocks(int n_agents, int A, int H, int W) {
    return (size_t)n_agents * (((size_t)A * H * W + kBlock - 1) / kBlock);
}

int coalign::stage1_decode_segments(const float *cls, const float *reg, const float *dir, const float *anchors, size_t cls_stride, size_t reg_stride, size_t dir_stride,
                           int n_agents, int A, int H, int W, int num_bins,
                                    float score_thr, float dir_offset, int order_hwl, int32_t *block_counts, int32_t *seg_start, int32_t *cand_index,
                                    float *cand_score, float *cand_corners, uint8_t *cand_keep, uint32_t *clear_word, hipStream_t stream) {
    DecodeArgs a;
    a.cls = cls; a.reg = reg; a.dir = dir; a.anchors = anchors; a.T = nullptr;
    a.A = A; a.HW = H * W; a.nb = num_bins; a.total = A * H * W; a.hwl = order_hwl; a.capacity = n_agents * a.total;
    a.thr = score_thr; a.dir_offset = dir_offset;
    a.count_in = nullptr; a.count_out = nullptr; a.cand_index = cand_index; a.cand_score = cand_score;
    a.cand_box7 = nullptr; a.cand_corners = cand_corners; a.cand_keep = cand_keep; a.status = nullptr;
    a.block_counts = block_counts;
    a.clear = clear_word;
    a.n_clear = 1;
    SegArgs s;
    s.n_agents = n_agents; s.bpa = (a.total + kBlock - 1) / kBlock;
    s.cls_stride = cls_stride; s.reg_stride = reg_stride; s.dir_stride = dir_stride;
    s.seg_start = seg_start;
    const int blocks = n_agents * s.bpa;
    hipLaunchKernelGGL(count_seg_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, s);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(emit_seg_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, s);
    return check_launch();
}

extern "C" {

size_t coalign_anchor_decode_workspace_bytes(int A, int H, int W) {
    if (A <= 0 || H <= 0 || W <= 0) return 0;
    const size_t total = (size_t)A * H * W;
    return coalign::align_up(((total + kBlock - 1) / kBlock) * sizeof(int), 256);
}

static int anchor_decode_impl(const float *cls, const float *reg, const float *dir, const float *anchors, int A, int H, int W,
                              int num_bins, float score_thr, float dir_offset, int order_hwl, const float *transform,
                              int capacity, const int32_t *count_in, int32_t *count_out, int32_t *cand_index,
                              float *cand_score, float *cand_box7, float *cand_corners, uint8_t *cand_keep, uint32_t *status,
                              void *workspace, size_t workspace_bytes, uint32_t *clear_words, int n_clear, void *stream_);

int coalign_anchor_decode(const float *cls, const float *reg, const float *dir, const float *anchors, int A, int H, int W,
                          int num_bins, float score_thr, float dir_offset, int order_hwl, const float *transform,
                          int capacity, const int32_t *count_in, int32_t *count_out, int32_t *cand_index,
                          float *cand_score, float *cand_box7, float *cand_corners, uint8_t *cand_keep, uint32_t *status,
                          void *workspace, size_t workspace_bytes, void *stream_) {
    return anchor_decode_impl(cls, reg, dir, anchors, A, H, W, num_bins, score_thr, dir_offset, order_hwl, transform, capacity, count_in, count_out, cand_index, cand_score, cand_box7,
                              cand_corners, cand_keep, status, workspace, workspace_bytes, nullptr, 0, stream_);
}

// Round 6: the FIRST decode call of a frame also zeroes the frame's counter / status words (n_clear <= 256 32-bit words at clear_words: count_in, count_out and status
// normally point into them) -- the fill launch in front of the post-processing chain is gone.
int coalign_anchor_decode_first(const float *cls, const float *reg, const float *dir, const float *anchors, int A, int H, int W,
                                int num_bins, float score_thr, float dir_offset, int order_hwl, const float *transform,
                                int capacity, const int32_t *count_in, int32_t *count_out, int32_t *cand_index,
                                float *cand_score, float *cand_box7, float *cand_corners, uint8_t *cand_keep, uint32_t *status,
                                void *workspace, size_t workspace_bytes, uint32_t *clear_words, int n_clear, void *stream_) {
    if (!clear_words) return COALIGN_ERR_NULL_POINTER;
    if (n_clear < 1 || n_clear > kBlock) return COALIGN_ERR_BAD_SHAPE;
    return anchor_decode_impl(cls, reg, dir, anchors, A, H, W, num_bins, score_thr, dir_offset, order_hwl, transform, capacity, count_in, count_out, cand_index, cand_score, cand_box7,
                              cand_corners, cand_keep, status, workspace, workspace_bytes, clear_words, n_clear, stream_);
}

static int anchor_decode_impl(const float *cls, const float *reg, const float *dir, const float *anchors, int A, int H, int W,
                              int num_bins, float score_thr, float dir_offset, int order_hwl, const float *transform,
                              int capacity, const int32_t *count_in, int32_t *count_out, int32_t *cand_index,
                              float *cand_score, float *cand_box7, float *cand_corners, uint8_t *cand_keep, uint32_t *status,
                              void *workspace, size_t workspace_bytes, uint32_t *clear_words, int n_clear, void *stream_) {
    using namespace coalign;
    hipStream_t stream = (hipStream_t)stream_;
    if (A <= 0 || H <= 0 || W <= 0 || capacity < 0 || (dir && num_bins <= 0)) return COALIGN_ERR_BAD_SHAPE;
    if ((size_t)A * H * W * 7 > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!cls || !reg || !anchors || !count_out || !cand_score || !cand_corners || !cand_keep || !workspace)
        return COALIGN_ERR_NULL_POINTER;
    if (workspace_bytes < coalign_anchor_decode_workspace_bytes(A, H, W)) return COALIGN_ERR_WORKSPACE;
    DecodeArgs a;
    a.cls = cls; a.reg = reg; a.dir = dir; a.anchors = anchors; a.T = transform;
    a.A = A; a.HW = H * W; a.nb = num_bins; a.total = A * H * W; a.hwl = order_hwl; a.capacity = capacity;
    a.thr = score_thr; a.dir_offset = dir_offset;
    a.count_in = count_in; a.count_out = count_out; a.cand_index = cand_index; a.cand_score = cand_score;
    a.cand_box7 = cand_box7; a.cand_corners = cand_corners; a.cand_keep = cand_keep; a.status = status;
    a.block_counts = (int *)workspace;
    a.clear = clear_words;
    a.n_clear = clear_words ? n_clear : 0;
    const int blocks = (a.total + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(count_kernel, dim3(blocks), dim3(kBlock), 0, stream, a);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(emit_kernel, dim3(blocks), dim3(kBlock), 0, stream, a);
    return check_launch();
}

}  // extern "C"
