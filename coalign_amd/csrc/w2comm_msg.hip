// Where2comm's messages on gfx950: what an agent transmits once its communication mask is known (a bitmap and the masked pixels' rows, packed in raster order)
// and a fusion whose bilinear taps read it.  The reference has no counterpart: Communication.forward (opencood/models/comm_modules/where2comm.py:34-78) and
// Where2comm.forward (opencood/models/fuse_modules/where2comm_attn.py:224-341) multiply dense maps by masks and stop.  The format, and its layout on a wire, are
// stated in coalign_amd_where2comm_msg.h.
//
// (1) w2comm_msg_index_kernel.  One workgroup of 256 lanes per (agent, level).  A lane owns one 32-pixel word per pass: it builds the word from the mask bytes
// (sender) or reads it (receiver), counts it with __popc, the wavefront scans the counts over its 64 lanes with __shfl_up, the four wavefronts' totals meet in
// LDS, and a carry runs from pass to pass: rank[word] = set bits before the word in raster order, count = the carry at the end.  Integers: exact in any order.
//
// (2) w2comm_msg_pack_kernel.  The lane layout of the fusion tile (C / 8 lanes per pixel, two float4 per lane): a set pixel's channels go to row
// rank[word] + popc(word & lower bits) with 16-byte loads and stores, an unset pixel's lanes leave.  Deterministic: the row number is a function of the bits.
//
// (3) w2comm_fuse_packed_kernel.  w2comm_fuse_tile.h's tile -- that of w2comm.hip, instruction for instruction -- with a source per agent and scale.  The lane
// that computes agent j's taps looks each tap's source pixel up: a dense source multiplies the weight by the mask byte, as w2comm.hip does; a packed source turns
// the tap's offset into that of the pixel's row, or, when the bit is clear, into "not sent" (a negative offset and a zero weight).  A tap that was not sent loads
// row 0 and its value is REPLACED by zero before the blend: rows behind the count are never written and may hold NaN, and NaN * 0 is NaN.
#include "common.h"
#include "warp_taps.h"
#include "nhwc_lanes.h"
#include "w2comm_fuse_tile.h"
#include "coalign_amd_where2comm_msg.h"

namespace {

using coalign::misaligned;
constexpr int kMsgLevels = 3, kMsgAgents = 8;

// ---- (1) index ------------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kIndexThreads = 256;

struct IndexArgs {
    const uint8_t *m[kMsgLevels];      // [n, H, W] or all NULL (receiver form)
    uint32_t *bits[kMsgLevels];        // [n, H, Wd]
    int32_t *rank[kMsgLevels];         // [n, H, Wd]
    int32_t *count;                    // [n, levels]
    int H[kMsgLevels], W[kMsgLevels];
    int levels;
};

__global__ __launch_bounds__(kIndexThreads) void w2comm_msg_index_kernel(const IndexArgs a) {
    __shared__ int wave_sum[kIndexThreads / 64];
    const int agent = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint8_t *m = a.m[0];
    uint32_t *bits = a.bits[0];
    int32_t *rank = a.rank[0];
    int H = a.H[0], W = a.W[0];
#pragma unroll
    for (int i = 1; i < kMsgLevels; ++i)
        if (l == i) { m = a.m[i]; bits = a.bits[i]; rank = a.rank[i]; H = a.H[i]; W = a.W[i]; }          // workgroup-uniform
    const int Wd = (W + 31) >> 5, nwords = H * Wd;
    if (m) m += (size_t)agent * H * W;
    bits += (size_t)agent * nwords;
    rank += (size_t)agent * nwords;
    const bool by4 = m && ((reinterpret_cast<uintptr_t>(m) | (uintptr_t)W) & 3) == 0;      // every word of every row starts at a 4-byte boundary: 8 loads, not 32
    int carry = 0;
    for (int base = 0; base < nwords; base += kIndexThreads) {      // workgroup-uniform trip count
        const int i = base + tid;
        uint32_t word = 0;
        if (i < nwords) {
            const int y = i / Wd, wx = i - y * Wd, x0 = wx * 32, nb = min(32, W - x0);
            if (m) {
                const uint8_t *p = m + (size_t)y * W + x0;
                if (by4) {
                    for (int q = 0; 4 * q < nb; ++q) {                // nb is a multiple of 4 here
                        const uint32_t v = reinterpret_cast<const uint32_t *>(p)[q];
                        const uint32_t four = ((v & 0xffu) ? 1u : 0u) | ((v & 0xff00u) ? 2u : 0u) | ((v & 0xff0000u) ? 4u : 0u) | ((v & 0xff000000u) ? 8u : 0u);
                        word |= four << (4 * q);
                    }
                } else {
                    for (int b = 0; b < nb; ++b) word |= (p[b] ? 1u : 0u) << b;
                }
                bits[i] = word;
            } else {
                word = bits[i] & (nb == 32 ? 0xffffffffu : (1u << nb) - 1u);      // a receiver trusts no padding bit
            }
        }
        const int c = __popc(word);
        int inc = c;                                                   // inclusive scan over the wavefront
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        if (lane == 63) wave_sum[wv] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kIndexThreads / 64; ++w) {
            const int s = wave_sum[w];
            before += w < wv ? s : 0;
            total += s;
        }
        if (i < nwords) rank[i] = carry + before + inc - c;
        carry += total;
        __syncthreads();                                               // wave_sum is written again in the next pass
    }
    if (tid == 0) a.count[agent * a.levels + l] = carry;
}

// ---- (2) pack -------------------------------------------------------------------------------------------------------------------------------------------------------
struct PackLevel {
    const float *x;            // [n, H, W, C]
    const uint32_t *bits;      // [n, H, Wd]
    const int32_t *rank;       // [n, H, Wd]
    float *rows;               // [n, H W, C]
    int C, H, W, first_block, n_blocks, blocks_per_agent;
};

struct PackArgs {
    PackLevel s[kMsgLevels];
    int levels;
};

template <int LPP>
__device__ __forceinline__ void pack_pixels(const PackLevel &a, int agent, int blk, int wave, int lane) {
    constexpr int PPW = 64 / LPP;
    const int li = lane % LPP, pi = lane / LPP;
    const int HW = a.H * a.W, Wd = (a.W + 31) >> 5;
    const int p = (blk * 4 + wave) * PPW + pi;
    if (p >= HW) return;
    const int y = p / a.W, x = p - y * a.W, b = x & 31;
    const size_t wi = ((size_t)agent * a.H + y) * Wd + (x >> 5);
    const uint32_t word = a.bits[wi];
    if (!((word >> b) & 1u)) return;
    const int row = a.rank[wi] + __popc(word & ((1u << b) - 1u));
    if ((unsigned)row >= (unsigned)HW) return;                          // a rank table that is not these bits': nothing is written outside the buffer
    const float4 *src = reinterpret_cast<const float4 *>(a.x + ((size_t)agent * HW + p) * a.C + 4 * li);
    float4 *dst = reinterpret_cast<float4 *>(a.rows + ((size_t)agent * HW + row) * a.C + 4 * li);
    const int hi4 = a.C / 8;
    const float4 lo = src[0], hi = src[hi4];
    dst[0] = lo;
    dst[hi4] = hi;
}

__global__ __launch_bounds__(256) void w2comm_msg_pack_kernel(const PackArgs f) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int bid = blockIdx.x;
#pragma unroll
    for (int k = 0; k < kMsgLevels; ++k) {
        if (k < f.levels && bid >= f.s[k].first_block && bid < f.s[k].first_block + f.s[k].n_blocks) {
            const PackLevel &a = f.s[k];
            const int r = bid - a.first_block, agent = r / a.blocks_per_agent, blk = r - agent * a.blocks_per_agent;
            const int lpp = a.C / 8;
            if (lpp == 8) pack_pixels<8>(a, agent, blk, wave, lane);
            else if (lpp == 16) pack_pixels<16>(a, agent, blk, wave, lane);
            else pack_pixels<32>(a, agent, blk, wave, lane);
            return;
        }
    }
}

// ---- (3) fusion from dense and packed sources -----------------------------------------------------------------------------------------------------------------------
struct Source {
    const float *x;          // dense: the plane [H, W, C]; packed: rows [H W, C]
    const void *aux;         // dense: mask bytes [H, W] or NULL; packed: bits [H, Wd]
    const int32_t *rank;     // packed: [H, Wd]; NULL = a dense source
};

struct PackedFuseArgs {
    ScaleArgs s[kMaxScales];
    const double *theta;  // [n, 2, 3]
    int n_scales, n, mode;
    Source src[kMaxScales][kMsgAgents];
    static constexpr bool kPacked = true;

    // one tap of a packed source: its pixel's row when the bit is set, "not sent" otherwise
    static __device__ __forceinline__ void look(const ScaleArgs &a, const uint32_t *bits, const int32_t *rank, int y, int x, int &o, float &w) {
        const int wi = y * ((a.W + 31) >> 5) + (x >> 5), b = x & 31;
        const uint32_t word = bits[wi];
        const int row = rank[wi] + __popc(word & ((1u << b) - 1u));
        const bool on = ((word >> b) & 1u) && (unsigned)row < (unsigned)(a.H * a.W);      // (a row outside the buffer: a rank table that is not these bits')
        o = on ? row << a.log2C : -1;
        w = on ? w : 0.f;
    }

    __device__ __forceinline__ void mask_taps(const ScaleArgs &a, int k, int agent, Taps &t) const {
        Source s = src[k][0];
#pragma unroll
        for (int i = 1; i < kMsgAgents; ++i)
            if (agent == i) s = src[k][i];
        if (s.rank) {
            const uint32_t *bits = static_cast<const uint32_t *>(s.aux);
            const int p0 = t.o00 >> a.log2C, p1 = t.o11 >> a.log2C;          // (yc0, xc0) and (yc1, xc1): the other two taps share their coordinates
            const int y0 = p0 / a.W, x0 = p0 - y0 * a.W, y1 = p1 / a.W, x1 = p1 - y1 * a.W;
            look(a, bits, s.rank, y0, x0, t.o00, t.w00);
            look(a, bits, s.rank, y0, x1, t.o01, t.w01);
            look(a, bits, s.rank, y1, x0, t.o10, t.w10);
            look(a, bits, s.rank, y1, x1, t.o11, t.w11);
        } else if (s.aux) {                                                  // w2comm.hip's tap
            const uint8_t *m = static_cast<const uint8_t *>(s.aux);
            t.w00 *= (float)m[t.o00 >> a.log2C];
            t.w01 *= (float)m[t.o01 >> a.log2C];
            t.w10 *= (float)m[t.o10 >> a.log2C];
            t.w11 *= (float)m[t.o11 >> a.log2C];
        }
    }
    __device__ __forceinline__ const float *plane(const ScaleArgs &, int k, int n) const { return src[k][n].x; }
};

template <int NA>
__global__ __launch_bounds__(256) void w2comm_fuse_packed_kernel(const PackedFuseArgs f) {
    COALIGN_W2COMM_FUSE_BLOCK(NA, f);
}


// the checks the three entry points share: -> COALIGN_OK or the refusal
inline int check_counts(int n, int levels) {
    if (n < 1 || levels < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > kMsgAgents || levels > kMsgLevels) return COALIGN_ERR_UNSUPPORTED;
    return COALIGN_OK;
}

}  // namespace

extern "C" int coalign_w2comm_msg_index(int n, int levels, const int32_t *H, const int32_t *W, const uint8_t *const *masks, uint32_t *const *bits,
                                        int32_t *const *rank, int32_t *count, void *stream_) {
    using namespace coalign;
    hipStream_t stream = (hipStream_t)stream_;
    if (const int bad = check_counts(n, levels)) return bad;
    if (!H || !W || !bits || !rank || !count) return COALIGN_ERR_NULL_POINTER;
    IndexArgs a;
    for (int l = 0; l < kMsgLevels; ++l) {
        a.m[l] = nullptr; a.bits[l] = nullptr; a.rank[l] = nullptr; a.H[l] = a.W[l] = 1;
        if (l >= levels) continue;
        if (!bits[l] || !rank[l] || (masks && !masks[l])) return COALIGN_ERR_NULL_POINTER;
        if (H[l] < 1 || W[l] < 1 || (size_t)H[l] * W[l] > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
        if (misaligned(bits[l], 3) || misaligned(rank[l], 3)) return COALIGN_ERR_UNSUPPORTED;
        a.m[l] = masks ? masks[l] : nullptr; a.bits[l] = bits[l]; a.rank[l] = rank[l]; a.H[l] = H[l]; a.W[l] = W[l];
    }
    if (misaligned(count, 3)) return COALIGN_ERR_UNSUPPORTED;
    a.count = count; a.levels = levels;
    hipLaunchKernelGGL(w2comm_msg_index_kernel, dim3(n, levels), dim3(kIndexThreads), 0, stream, a);
    return check_launch();
}

extern "C" int coalign_w2comm_msg_pack(int n, int levels, const float *const *x, const int32_t *C, const int32_t *H, const int32_t *W,
                                       const uint32_t *const *bits, const int32_t *const *rank, float *const *rows, void *stream_) {
    using namespace coalign;
    hipStream_t stream = (hipStream_t)stream_;
    if (const int bad = check_counts(n, levels)) return bad;
    if (!x || !C || !H || !W || !bits || !rank || !rows) return COALIGN_ERR_NULL_POINTER;
    PackArgs f;
    f.levels = levels;
    int next_block = 0;
    for (int l = 0; l < levels; ++l) {
        if (!x[l] || !bits[l] || !rank[l] || !rows[l]) return COALIGN_ERR_NULL_POINTER;
        if (C[l] < 1 || H[l] < 1 || W[l] < 1) return COALIGN_ERR_BAD_SHAPE;
        if (C[l] != 64 && C[l] != 128 && C[l] != 256) return COALIGN_ERR_UNSUPPORTED;
        if ((size_t)C[l] * H[l] * W[l] > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
        if (misaligned(x[l], 15) || misaligned(rows[l], 15) || misaligned(bits[l], 3) || misaligned(rank[l], 3)) return COALIGN_ERR_UNSUPPORTED;
        PackLevel &a = f.s[l];
        a.x = x[l]; a.bits = bits[l]; a.rank = rank[l]; a.rows = rows[l]; a.C = C[l]; a.H = H[l]; a.W = W[l];
        const int per_block = 4 * (512 / C[l]);                        // 4 wavefronts of 64 / (C / 8) pixels
        a.blocks_per_agent = (H[l] * W[l] + per_block - 1) / per_block;
        a.n_blocks = n * a.blocks_per_agent;
        a.first_block = next_block;
        next_block += a.n_blocks;
    }
    for (int l = levels; l < kMsgLevels; ++l) f.s[l] = f.s[0];
    hipLaunchKernelGGL(w2comm_msg_pack_kernel, dim3(next_block), dim3(256), 0, stream, f);
    return check_launch();
}

extern "C" int coalign_w2comm_fuse_packed(int n_scales, const int32_t *C, const int32_t *H, const int32_t *W, const int32_t *kind, const float *const *src,
                                          const void *const *aux, const int32_t *const *rank, float *const *out, const int32_t *Ho, const int32_t *Wo, int n,
                                          const double *theta, int mode, void *stream_) {
    using namespace coalign;
    hipStream_t stream = (hipStream_t)stream_;
    if (const int bad = check_counts(n, n_scales)) return bad;
    if (mode != COALIGN_FUSE_ATT && mode != COALIGN_FUSE_MAX) return COALIGN_ERR_UNSUPPORTED;
    if (!C || !H || !W || !kind || !src || !aux || !rank || !out || !Ho || !Wo || !theta) return COALIGN_ERR_NULL_POINTER;
    for (int i = 0; i < n_scales; ++i) {
        if (!out[i]) return COALIGN_ERR_NULL_POINTER;
        if (C[i] < 1 || H[i] < 1 || W[i] < 1 || Ho[i] < 1 || Wo[i] < 1) return COALIGN_ERR_BAD_SHAPE;
        if (C[i] != 64 && C[i] != 128 && C[i] != 256) return COALIGN_ERR_UNSUPPORTED;
        if ((size_t)C[i] * H[i] * W[i] > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
        if (misaligned(out[i], 15)) return COALIGN_ERR_UNSUPPORTED;
        for (int j = 0; j < n; ++j) {
            const int e = i * n + j;
            if (kind[e] != COALIGN_W2COMM_SRC_DENSE && kind[e] != COALIGN_W2COMM_SRC_PACKED) return COALIGN_ERR_UNSUPPORTED;
            if (!src[e]) return COALIGN_ERR_NULL_POINTER;
            if (misaligned(src[e], 15)) return COALIGN_ERR_UNSUPPORTED;
            if (kind[e] == COALIGN_W2COMM_SRC_PACKED) {
                if (!aux[e] || !rank[e]) return COALIGN_ERR_NULL_POINTER;
                if (misaligned(aux[e], 3) || misaligned(rank[e], 3)) return COALIGN_ERR_UNSUPPORTED;
            }
        }
    }
    PackedFuseArgs f;
    f.theta = theta; f.n = n; f.mode = mode; f.n_scales = n_scales;
    int order[kMaxScales];
    const int n_blocks = plan_scales(f.s, order, n_scales, C, H, W, Ho, Wo, out);      // heaviest tiles first
    for (int k = 0; k < kMaxScales; ++k)
        for (int j = 0; j < kMsgAgents; ++j) {
            const int e = order[k < n_scales ? k : 0] * n + (j < n ? j : 0);
            const bool packed = kind[e] == COALIGN_W2COMM_SRC_PACKED;
            f.src[k][j] = Source{src[e], aux[e], packed ? rank[e] : nullptr};
        }
    for (int k = n_scales; k < kMaxScales; ++k) f.s[k] = f.s[0];
    const dim3 grid(n_blocks), block(256);
    if (n == 1) hipLaunchKernelGGL(w2comm_fuse_packed_kernel<1>, grid, block, 0, stream, f);
    else if (n == 2) hipLaunchKernelGGL(w2comm_fuse_packed_kernel<2>, grid, block, 0, stream, f);
    else if (n == 3) hipLaunchKernelGGL(w2comm_fuse_packed_kernel<3>, grid, block, 0, stream, f);
    else if (n <= 5) hipLaunchKernelGGL(w2comm_fuse_packed_kernel<5>, grid, block, 0, stream, f);
    else hipLaunchKernelGGL(w2comm_fuse_packed_kernel<8>, grid, block, 0, stream, f);
    return check_launch();
}
