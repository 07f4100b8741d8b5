// The sparse 3-D trunk of the SECOND detectors, gfx950: MeanVFE, spconv's SubMConv3d / SparseConv3d restated as a gather-GEMM over site lists, and the dense map
// of HeightCompression (mean_vfe.py:26-30, sparse_backbone_3d.py:48-91, height_compression.py:20-23).  spconv is not linked.
//
//   sp3d_mean_vfe        one lane per (voxel, channel): the T slots added in slot order, divided by max(num_points, 1).
//   the site index       cell -> row of a site list: a dense bitmap over the linear cell index, one prefix count per 32-bit word, a rank -> row table.  Built by
//                        fill_words (common.h), sp3d_mark / sp3d_mark_strided (integer atomicOr), sp3d_block_sums + sp3d_scan_sums + sp3d_word_prefix (the count over
//                        the words: 1024 words per workgroup, the workgroups' sums scanned by one workgroup, which also leaves the site count ON THE DEVICE) and
//                        sp3d_perm (rank -> row of an arbitrary-order list) or sp3d_enumerate (a strided layer's output rows, ascending in the cell index).
//   sp3d_neighbors       per output row and tap the input row or -1 (tap-major), one lane per (row, tap); the submanifold layers of a level share the table.
//   sp3d_conv_mfma       output-stationary: a wavefront owns 32 output rows x 32 output channels.  Per tap a lane reads its row's neighbour and, when any of the 32
//                        has one, 8 of the neighbour's channels (32 contiguous bytes), splits them into an sp16 pair in registers (the B operand of
//                        v_mfma_f32_32x32x16_f16) and multiplies with the weight image's 32-byte piece (the A operand), three instructions per fp32 product
//                        (sp16_tiles.h).  Every row of the weight image is divided by a power of two 2^k_c on the host so that its largest |w| lies in [1, 2) -- an UNSCALED pair keeps
//                        an absolute 2^-34 of a weight below 2^-14, which costs a channel whose folded batch-norm scale is small most of its digits -- and the epilogue
//                        multiplies the joined sum by 2^k_c from the image's tail (exact: a layer whose pairs were all normal gives the same bits).  Taps in ascending order, a missing neighbour is a zero row, a tap none of the 32 rows has is skipped (it adds zeros); a row without any neighbour is no site and is written as zeros.  No LDS,
//                        no barrier, no atomics.  Epilogue: x 2^k_c, + shift, ReLU, four 16-byte stores per lane.
//   sp3d_conv_c4         the 4 -> 16 input layer on fp32 vector arithmetic: one lane per output row, the 27 x 4 x 16 weights in LDS.
//   sp3d_to_dense        one wavefront per (b, y, x): lanes across the C D channels, a lookup per (lane, d); every element written.
//   vox_*                raw point clouds -> the trunk's input tensor (mean features, indices, count) with its site index already built: at the end of this file.
// Counts are read from the device by every kernel (grids are sized by capacity); rows at or past the count are never touched.
#include "common.h"
#include "sp16_tiles.h"

#include "coalign_amd_sparse3d.h"
#include "coalign_amd_sp3d_voxelize.h"

namespace {

using coalign::align_up;
using coalign::misaligned;

constexpr int WORDS_PER_BLOCK = 1024;      // 256 lanes x 4 words

struct Grid {
    int N, D, H, W;
};

struct IndexLayout {
    size_t words, blocks, off_prefix, off_sums, off_perm, bytes;
};

bool grid_ok(int N, int D, int H, int W) {
    return N >= 1 && D >= 1 && H >= 1 && W >= 1 && (size_t)N * (size_t)D * (size_t)H * (size_t)W <= (size_t)INT32_MAX;
}

IndexLayout layout_of(int N, int D, int H, int W, int capacity) {
    IndexLayout l;
    const size_t cells = (size_t)N * (size_t)D * (size_t)H * (size_t)W;
    l.words = (cells + 31) / 32;
    l.blocks = (l.words + WORDS_PER_BLOCK - 1) / WORDS_PER_BLOCK;
    l.off_prefix = align_up(l.words * 4, 256);
    l.off_sums = l.off_prefix + align_up(l.words * 4, 256);
    l.off_perm = l.off_sums + align_up((l.blocks + 1) * 4, 256);
    l.bytes = l.off_perm + align_up((size_t)(capacity > 0 ? capacity : 1) * 4, 256);
    return l;
}

struct Index {                 // the device view of a site index
    unsigned *bits;
    int *prefix, *sums, *perm;
    Grid g;
    int cap, words, blocks;
};

Index view_of(void *base, int N, int D, int H, int W, int capacity) {
    const IndexLayout l = layout_of(N, D, H, W, capacity);
    char *p = static_cast<char *>(base);
    Index ix;
    ix.bits = reinterpret_cast<unsigned *>(p);
    ix.prefix = reinterpret_cast<int *>(p + l.off_prefix);
    ix.sums = reinterpret_cast<int *>(p + l.off_sums);
    ix.perm = reinterpret_cast<int *>(p + l.off_perm);
    ix.g = Grid{N, D, H, W};
    ix.cap = capacity;
    ix.words = (int)l.words;
    ix.blocks = (int)l.blocks;
    return ix;
}

__device__ __forceinline__ int clamped(const int *count, int cap) {
    const int n = *count;
    return n < 0 ? 0 : n > cap ? cap : n;
}

__device__ __forceinline__ bool inside(const Grid &g, int b, int z, int y, int x) {
    return (unsigned)b < (unsigned)g.N && (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W;
}

__device__ __forceinline__ int cell_of(const Grid &g, int b, int z, int y, int x) { return ((b * g.D + z) * g.H + y) * g.W + x; }

// the row of cell (b, z, y, x) or -1
__device__ __forceinline__ int lookup(const Index &ix, int b, int z, int y, int x) {
    if (!inside(ix.g, b, z, y, x)) return -1;
    const int cell = cell_of(ix.g, b, z, y, x);
    const unsigned m = ix.bits[cell >> 5], bit = (unsigned)cell & 31u;
    if (!((m >> bit) & 1u)) return -1;
    const int rank = ix.prefix[cell >> 5] + __popc(m & ((1u << bit) - 1u));
    if ((unsigned)rank >= (unsigned)ix.cap) return -1;
    return ix.perm[rank];
}

__global__ __launch_bounds__(256) void sp3d_mean_vfe(const float *__restrict__ voxels, const int *__restrict__ num_points, int M, int T, int C, float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * C) return;
    const int m = i / C, c = i - m * C;
    const float *src = voxels + (size_t)m * T * C + c;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += src[(size_t)t * C];
    const int n = num_points[m];
    out[i] = s / (float)(n < 1 ? 1 : n);
}

__global__ __launch_bounds__(256) void sp3d_mark(const int4 *__restrict__ indices, const int *__restrict__ count, const Index ix) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= clamped(count, ix.cap)) return;
    const int4 v = indices[r];                                 // (b, z, y, x)
    if (!inside(ix.g, v.x, v.y, v.z, v.w)) return;
    const int cell = cell_of(ix.g, v.x, v.y, v.z, v.w);
    atomicOr(&ix.bits[cell >> 5], 1u << (cell & 31));
}

struct Geometry {
    int k[3], s[3], p[3];
};

// every output site that an input row reaches: o = (i + p - kappa) / s where that division is exact and o is inside the output grid
__global__ __launch_bounds__(256) void sp3d_mark_strided(const int4 *__restrict__ indices, const int *__restrict__ count, int cap_in, const Grid in, const Geometry ge,
                                                         const Index ox) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= clamped(count, cap_in)) return;
    const int4 v = indices[r];
    if (!inside(in, v.x, v.y, v.z, v.w)) return;
    for (int kz = 0; kz < ge.k[0]; ++kz) {
        const int tz = v.y + ge.p[0] - kz;
        if (tz < 0 || tz % ge.s[0] != 0 || tz / ge.s[0] >= ox.g.D) continue;
        for (int ky = 0; ky < ge.k[1]; ++ky) {
            const int ty = v.z + ge.p[1] - ky;
            if (ty < 0 || ty % ge.s[1] != 0 || ty / ge.s[1] >= ox.g.H) continue;
            for (int kx = 0; kx < ge.k[2]; ++kx) {
                const int tx = v.w + ge.p[2] - kx;
                if (tx < 0 || tx % ge.s[2] != 0 || tx / ge.s[2] >= ox.g.W) continue;
                const int cell = cell_of(ox.g, v.x, tz / ge.s[0], ty / ge.s[1], tx / ge.s[2]);
                atomicOr(&ox.bits[cell >> 5], 1u << (cell & 31));
            }
        }
    }
}

// exclusive scan of one value per lane over the 256 lanes of a workgroup; total in every lane's `total`
__device__ __forceinline__ int block_scan(int v, int *lds, int &total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = t >= o ? lds[t - o] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const int incl = lds[t];
    total = lds[255];
    __syncthreads();
    return incl - v;
}

// (`gate`, in the three kernels of the prefix count: NULL, or a device word -- 0 there makes the launch a no-op; the voxeliser's recount after a max_voxels cut)
__global__ __launch_bounds__(256) void sp3d_block_sums(const Index ix, const int *__restrict__ gate) {
    __shared__ int lds[256];
    if (gate && *gate == 0) return;
    const int w0 = blockIdx.x * WORDS_PER_BLOCK + threadIdx.x * 4;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (w0 + j < ix.words) c += __popc(ix.bits[w0 + j]);
    int total;
    (void)block_scan(c, lds, total);
    if (threadIdx.x == 0) ix.sums[blockIdx.x] = total;
}

// one workgroup: sums[b] <- the sites in front of word block b, sums[blocks] <- all sites; the count (clipped to the capacity) and the overflow bit
__global__ __launch_bounds__(256) void sp3d_scan_sums(const Index ix, int *__restrict__ count_out, unsigned *__restrict__ status, const int *__restrict__ gate) {
    __shared__ int lds[256];
    if (gate && *gate == 0) return;
    int carry = 0;
    for (int b0 = 0; b0 < ix.blocks; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int v = b < ix.blocks ? ix.sums[b] : 0;
        int total;
        const int excl = block_scan(v, lds, total);
        if (b < ix.blocks) ix.sums[b] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) {
        ix.sums[ix.blocks] = carry;
        if (count_out) *count_out = carry > ix.cap ? ix.cap : carry;
        if (status && carry > ix.cap) *status = *status | COALIGN_SP3D_STATUS_OVERFLOW;
    }
}

__global__ __launch_bounds__(256) void sp3d_word_prefix(const Index ix, const int *__restrict__ gate) {
    __shared__ int lds[256];
    if (gate && *gate == 0) return;
    const int w0 = blockIdx.x * WORDS_PER_BLOCK + threadIdx.x * 4;
    int c[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = w0 + j < ix.words ? __popc(ix.bits[w0 + j]) : 0;
        s += c[j];
    }
    int total;
    int base = ix.sums[blockIdx.x] + block_scan(s, lds, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (w0 + j < ix.words) ix.prefix[w0 + j] = base;
        base += c[j];
    }
}

// rank -> row of a list in arbitrary order (indices are unique)
__global__ __launch_bounds__(256) void sp3d_perm(const int4 *__restrict__ indices, const int *__restrict__ count, const Index ix) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= clamped(count, ix.cap)) return;
    const int4 v = indices[r];
    if (!inside(ix.g, v.x, v.y, v.z, v.w)) return;
    const int cell = cell_of(ix.g, v.x, v.y, v.z, v.w);
    const unsigned m = ix.bits[cell >> 5], bit = (unsigned)cell & 31u;
    const int rank = ix.prefix[cell >> 5] + __popc(m & ((1u << bit) - 1u));
    if ((unsigned)rank < (unsigned)ix.cap) ix.perm[rank] = r;
}

// the set bits of one word per lane -> rows `rank` of the output list (ascending in the cell index); rank = row
__global__ __launch_bounds__(256) void sp3d_enumerate(const Index ix, int4 *__restrict__ out_indices) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= ix.words) return;
    unsigned m = ix.bits[w];
    int rank = ix.prefix[w];
    while (m) {
        const int bit = __builtin_ctz(m);
        m &= m - 1;
        if ((unsigned)rank >= (unsigned)ix.cap) return;
        const int cell = w * 32 + bit;
        const int x = cell % ix.g.W, t = cell / ix.g.W, y = t % ix.g.H, u = t / ix.g.H, z = u % ix.g.D, b = u / ix.g.D;
        out_indices[rank] = make_int4(b, z, y, x);
        ix.perm[rank] = rank;
        ++rank;
    }
}

__global__ __launch_bounds__(256) void sp3d_neighbors(const int4 *__restrict__ out_indices, const int *__restrict__ out_count, int cap_out, const Grid og, const Index in,
                                                      const Geometry ge, int *__restrict__ nbr) {
    const int r = blockIdx.x * 256 + threadIdx.x, tap = blockIdx.y;
    if (r >= clamped(out_count, cap_out)) return;
    const int4 o = out_indices[r];
    int row = -1;
    if (inside(og, o.x, o.y, o.z, o.w)) {
        const int kx = tap % ge.k[2], t = tap / ge.k[2], ky = t % ge.k[1], kz = t / ge.k[1];
        row = lookup(in, o.x, o.y * ge.s[0] - ge.p[0] + kz, o.z * ge.s[1] - ge.p[1] + ky, o.w * ge.s[2] - ge.p[2] + kx);
    }
    nbr[(size_t)tap * cap_out + r] = row;
}

struct ConvArgs {
    const float *in;
    const int *nbr, *count;
    const unsigned char *img;
    const float *shift, *tail;             // tail: 2^k_c per output channel, behind the operand image (sp3d_conv_mfma)
    float *out;
    int cap_in, cap_out, taps, tiles, cout;
};

template <int CIN>
__global__ __launch_bounds__(256) void sp3d_conv_mfma(const ConvArgs a) {
    constexpr int STEPS = CIN / 16;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = clamped(a.count, a.cap_out);
    const long long task = (long long)blockIdx.x * 4 + wave;
    const int ts = (int)(task / a.tiles), ct = (int)(task - (long long)ts * a.tiles);
    if ((long long)ts * 32 >= n) return;                        // (the whole wavefront alike)
    const int r = ts * 32 + (lane & 31), h = lane >> 5;
    const bool live = r < n;
    bool any = false;                                           // a row no tap of which has an input is no site (its coordinates lie outside the grid): zeros
    floatx16 acc, accl;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = accl[q] = 0.f;
    for (int tap = 0; tap < a.taps; ++tap) {
        const int nb = live ? a.nbr[(size_t)tap * a.cap_out + r] : -1;
        const bool has = (unsigned)nb < (unsigned)a.cap_in;
        any = any || has;
        if (!__builtin_amdgcn_ballot_w64(has)) continue;        // no row of the tile has this neighbour: the tap adds zeros
        const float *src = a.in + (size_t)(has ? nb : 0) * CIN + 8 * h;
        const unsigned char *wp = a.img + (((size_t)tap * STEPS * a.tiles + ct) * 64 + lane) * 32;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (has) {
                const float4 lo = *reinterpret_cast<const float4 *>(src + 16 * s), hi = *reinterpret_cast<const float4 *>(src + 16 * s + 4);
                v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
            }
            uint4 xh, xl;
            coalign::sp16_split8(v, xh, xl);
            Pair x;
            x.h = __builtin_bit_cast(halfx8, xh);
            x.l = __builtin_bit_cast(halfx8, xl);
            const Pair w = load_pair(wp + (size_t)s * a.tiles * 64 * 32);
            mfma3(w, x, acc, accl);
        }
    }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 32 * ct + 8 * i + 4 * h;                  // the lane's registers 4 i .. 4 i + 3: channels c .. c + 3 of row r
        if (c >= a.cout) continue;
        const float4 sh = *reinterpret_cast<const float4 *>(a.shift + c), p2 = *reinterpret_cast<const float4 *>(a.tail + c);
        float4 o;
        o.x = fmaxf(fmaf(accl[4 * i], coalign::kSp16LowInv, acc[4 * i]) * p2.x + sh.x, 0.f);
        o.y = fmaxf(fmaf(accl[4 * i + 1], coalign::kSp16LowInv, acc[4 * i + 1]) * p2.y + sh.y, 0.f);
        o.z = fmaxf(fmaf(accl[4 * i + 2], coalign::kSp16LowInv, acc[4 * i + 2]) * p2.z + sh.z, 0.f);
        o.w = fmaxf(fmaf(accl[4 * i + 3], coalign::kSp16LowInv, acc[4 * i + 3]) * p2.w + sh.w, 0.f);
        if (!any) o = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(a.out + (size_t)r * a.cout + c) = o;
    }
}

constexpr int C4_IN = 4, C4_OUT = 16, C4_TAPS = 27;

__global__ __launch_bounds__(256) void sp3d_conv_c4(const ConvArgs a) {
    __shared__ float w[C4_TAPS * C4_IN * C4_OUT];
    const float *wsrc = reinterpret_cast<const float *>(a.img);
    for (int i = threadIdx.x; i < C4_TAPS * C4_IN * C4_OUT; i += 256) w[i] = wsrc[i];
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= clamped(a.count, a.cap_out)) return;
    float acc[C4_OUT];
#pragma unroll
    for (int c = 0; c < C4_OUT; ++c) acc[c] = 0.f;
    bool any = false;
    for (int tap = 0; tap < C4_TAPS; ++tap) {
        const int nb = a.nbr[(size_t)tap * a.cap_out + r];
        if ((unsigned)nb >= (unsigned)a.cap_in) continue;
        any = true;
        const float4 x = *reinterpret_cast<const float4 *>(a.in + (size_t)nb * C4_IN);
        const float *wt = w + tap * C4_IN * C4_OUT;
#pragma unroll
        for (int c = 0; c < C4_OUT; ++c) {
            float s = acc[c];
            s = fmaf(x.x, wt[c], s);
            s = fmaf(x.y, wt[C4_OUT + c], s);
            s = fmaf(x.z, wt[2 * C4_OUT + c], s);
            s = fmaf(x.w, wt[3 * C4_OUT + c], s);
            acc[c] = s;
        }
    }
    float *dst = a.out + (size_t)r * C4_OUT;
#pragma unroll
    for (int c = 0; c < C4_OUT; c += 4)
        *reinterpret_cast<float4 *>(dst + c) = !any ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(fmaxf(acc[c] + a.shift[c], 0.f), fmaxf(acc[c + 1] + a.shift[c + 1], 0.f), fmaxf(acc[c + 2] + a.shift[c + 2], 0.f),
                                                           fmaxf(acc[c + 3] + a.shift[c + 3], 0.f));
}

__global__ __launch_bounds__(256) void sp3d_to_dense(const float *__restrict__ feat, const int *__restrict__ count, int C, const Index ix, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int pixels = ix.g.N * ix.g.H * ix.g.W;
    if (pix >= pixels) return;
    const int n = clamped(count, ix.cap);
    const int x = (int)(pix % ix.g.W), t = (int)(pix / ix.g.W), y = t % ix.g.H, b = t / ix.g.H;
    const int CD = C * ix.g.D;
    float *dst = out + (size_t)pix * CD;
    for (int ch = lane; ch < CD; ch += 64) {
        const int c = ch / ix.g.D, d = ch - c * ix.g.D;
        const int row = lookup(ix, b, d, y, x);
        dst[ch] = (unsigned)row < (unsigned)n ? feat[(size_t)row * C + c] : 0.f;
    }
}

unsigned blocks_for(size_t n, size_t per) { return (unsigned)(n == 0 ? 1 : (n + per - 1) / per); }

// the three launches of the prefix count, common to both index builders
int prefix_count(const Index &ix, int *count_out, unsigned *status, hipStream_t stream, const int *gate = nullptr) {
    hipLaunchKernelGGL(sp3d_block_sums, dim3((unsigned)ix.blocks), dim3(256), 0, stream, ix, gate);
    int rc = coalign::check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(sp3d_scan_sums, dim3(1), dim3(256), 0, stream, ix, count_out, status, gate);
    rc = coalign::check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(sp3d_word_prefix, dim3((unsigned)ix.blocks), dim3(256), 0, stream, ix, gate);
    return coalign::check_launch();
}

bool geometry_ok(const Geometry &g) {
    for (int a = 0; a < 3; ++a)
        if (g.k[a] < 1 || g.k[a] > 3 || g.s[a] < 1 || g.p[a] < 0) return false;
    return true;
}

int out_extent(int n, int k, int s, int p) { return n + 2 * p - k < 0 ? 0 : (n + 2 * p - k) / s + 1; }

// the sp16 operand image of a (Cin >= 16) layer; the per-channel powers of two follow it
size_t operand_image_bytes(int Cin, int Cout, int taps) { return (size_t)taps * (Cin / 16) * ((Cout + 31) / 32) * 64 * 32; }

bool supported(int Cin, int Cout, int taps) {
    if (taps == 27) return (Cin == 4 && Cout == 16) || (Cin == 16 && (Cout == 16 || Cout == 32)) || (Cin == 32 && (Cout == 32 || Cout == 64)) || (Cin == 64 && Cout == 64);
    if (taps == 3) return Cin == 64 && (Cout == 64 || Cout == 128);
    return false;
}

}  // namespace

extern "C" int coalign_sp3d_mean_vfe(const float *voxels, const int *num_points, int M, int T, int C, float *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || T < 1 || C < 1 || (size_t)M * (size_t)T * (size_t)C > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (M == 0) return COALIGN_OK;
    if (!voxels || !num_points || !out || misaligned(voxels, 3) || misaligned(num_points, 3) || misaligned(out, 3)) return COALIGN_ERR_NULL_POINTER;
    hipLaunchKernelGGL(sp3d_mean_vfe, dim3(blocks_for((size_t)M * C, 256)), dim3(256), 0, stream, voxels, num_points, M, T, C, out);
    return coalign::check_launch();
}

extern "C" size_t coalign_sp3d_index_workspace_bytes(int N, int D, int H, int W, int capacity) {
    if (!grid_ok(N, D, H, W) || capacity < 0) return 0;
    return layout_of(N, D, H, W, capacity).bytes;
}

extern "C" int coalign_sp3d_index_build(const int *indices, const int *count, int capacity, int N, int D, int H, int W, void *index, size_t index_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!grid_ok(N, D, H, W) || capacity < 0) return COALIGN_ERR_BAD_SHAPE;
    if (index_bytes < layout_of(N, D, H, W, capacity).bytes) return COALIGN_ERR_WORKSPACE;
    if (!count || !index || (capacity > 0 && !indices) || misaligned(index, 15) || misaligned(indices, 15) || misaligned(count, 3)) return COALIGN_ERR_NULL_POINTER;
    const Index ix = view_of(index, N, D, H, W, capacity);
    int rc = coalign::fill_words(ix.bits, (size_t)ix.words, 0u, stream);
    if (rc) return rc;
    const int4 *idx = reinterpret_cast<const int4 *>(indices);
    hipLaunchKernelGGL(sp3d_mark, dim3(blocks_for((size_t)capacity, 256)), dim3(256), 0, stream, idx, count, ix);
    rc = coalign::check_launch();
    if (rc) return rc;
    rc = prefix_count(ix, nullptr, nullptr, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(sp3d_perm, dim3(blocks_for((size_t)capacity, 256)), dim3(256), 0, stream, idx, count, ix);
    return coalign::check_launch();
}

extern "C" int coalign_sp3d_strided_sites(const int *in_indices, const int *in_count, int cap_in, int N, int D, int H, int W, int kd, int kh, int kw, int sd, int sh, int sw,
                                          int pd, int ph, int pw, int *out_indices, int *out_count, int cap_out, void *out_index, size_t out_index_bytes, unsigned *status,
                                          void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const Geometry ge = {{kd, kh, kw}, {sd, sh, sw}, {pd, ph, pw}};
    if (!grid_ok(N, D, H, W) || cap_in < 0 || cap_out < 0 || !geometry_ok(ge)) return COALIGN_ERR_BAD_SHAPE;
    const int oD = out_extent(D, kd, sd, pd), oH = out_extent(H, kh, sh, ph), oW = out_extent(W, kw, sw, pw);
    if (!grid_ok(N, oD, oH, oW)) return COALIGN_ERR_BAD_SHAPE;
    if (out_index_bytes < layout_of(N, oD, oH, oW, cap_out).bytes) return COALIGN_ERR_WORKSPACE;
    if (!in_count || !out_count || !out_index || !status || (cap_in > 0 && !in_indices) || (cap_out > 0 && !out_indices)) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(in_indices, 15) || misaligned(out_indices, 15) || misaligned(out_index, 15) || misaligned(in_count, 3) || misaligned(out_count, 3) || misaligned(status, 3))
        return COALIGN_ERR_NULL_POINTER;
    const Index ox = view_of(out_index, N, oD, oH, oW, cap_out);
    int rc = coalign::fill_words(ox.bits, (size_t)ox.words, 0u, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(sp3d_mark_strided, dim3(blocks_for((size_t)cap_in, 256)), dim3(256), 0, stream, reinterpret_cast<const int4 *>(in_indices), in_count, cap_in,
                       Grid{N, D, H, W}, ge, ox);
    rc = coalign::check_launch();
    if (rc) return rc;
    rc = prefix_count(ox, out_count, status, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(sp3d_enumerate, dim3(blocks_for((size_t)ox.words, 256)), dim3(256), 0, stream, ox, reinterpret_cast<int4 *>(out_indices));
    return coalign::check_launch();
}

extern "C" int coalign_sp3d_neighbors(const int *out_indices, const int *out_count, int cap_out, int N, int oD, int oH, int oW, const void *in_index, size_t in_index_bytes,
                                      int cap_in, int D, int H, int W, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int *nbr, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const Geometry ge = {{kd, kh, kw}, {sd, sh, sw}, {pd, ph, pw}};
    if (!grid_ok(N, D, H, W) || !grid_ok(N, oD, oH, oW) || cap_in < 0 || cap_out < 0 || !geometry_ok(ge)) return COALIGN_ERR_BAD_SHAPE;
    const int taps = kd * kh * kw;
    if ((size_t)cap_out * (size_t)taps > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (in_index_bytes < layout_of(N, D, H, W, cap_in).bytes) return COALIGN_ERR_WORKSPACE;
    if (!out_count || !in_index || (cap_out > 0 && (!out_indices || !nbr))) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(out_indices, 15) || misaligned(in_index, 15) || misaligned(out_count, 3) || misaligned(nbr, 3)) return COALIGN_ERR_NULL_POINTER;
    if (cap_out == 0) return COALIGN_OK;
    const Index in = view_of(const_cast<void *>(in_index), N, D, H, W, cap_in);
    hipLaunchKernelGGL(sp3d_neighbors, dim3(blocks_for((size_t)cap_out, 256), (unsigned)taps), dim3(256), 0, stream, reinterpret_cast<const int4 *>(out_indices), out_count,
                       cap_out, Grid{N, oD, oH, oW}, in, ge, nbr);
    return coalign::check_launch();
}

extern "C" size_t coalign_sp3d_weight_bytes(int Cin, int Cout, int taps) {
    if (!supported(Cin, Cout, taps)) return 0;
    if (Cin == C4_IN) return (size_t)taps * Cin * Cout * 4;
    return operand_image_bytes(Cin, Cout, taps) + (size_t)((Cout + 31) / 32) * 32 * sizeof(float);
}

extern "C" int coalign_sp3d_conv(const float *in_feat, int cap_in, const int *nbr, int taps, const int *out_count, int cap_out, int Cin, int Cout, const void *weights,
                                 size_t weight_bytes, const float *shift, float *out_feat, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (cap_in < 0 || cap_out < 0 || taps < 1 || Cin < 1 || Cout < 1 || (size_t)cap_out * (size_t)taps > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!supported(Cin, Cout, taps)) return COALIGN_ERR_UNSUPPORTED;
    if (weight_bytes < coalign_sp3d_weight_bytes(Cin, Cout, taps)) return COALIGN_ERR_WORKSPACE;
    if (!out_count || !weights || !shift || (cap_in > 0 && !in_feat) || (cap_out > 0 && (!nbr || !out_feat))) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(in_feat, 15) || misaligned(out_feat, 15) || misaligned(weights, 15) || misaligned(shift, 15) || misaligned(nbr, 3) || misaligned(out_count, 3))
        return COALIGN_ERR_NULL_POINTER;
    if (cap_out == 0) return COALIGN_OK;
    ConvArgs a;
    a.in = in_feat; a.nbr = nbr; a.count = out_count; a.img = static_cast<const unsigned char *>(weights); a.shift = shift; a.out = out_feat;
    a.cap_in = cap_in; a.cap_out = cap_out; a.taps = taps; a.tiles = (Cout + 31) / 32; a.cout = Cout;
    a.tail = Cin == C4_IN ? nullptr : reinterpret_cast<const float *>(a.img + operand_image_bytes(Cin, Cout, taps));
    if (Cin == C4_IN) {
        hipLaunchKernelGGL(sp3d_conv_c4, dim3(blocks_for((size_t)cap_out, 256)), dim3(256), 0, stream, a);
        return coalign::check_launch();
    }
    const size_t tasks = (((size_t)cap_out + 31) / 32) * (size_t)a.tiles;
    const dim3 grid(blocks_for(tasks, 4));
    if (Cin == 16) hipLaunchKernelGGL(sp3d_conv_mfma<16>, grid, dim3(256), 0, stream, a);
    else if (Cin == 32) hipLaunchKernelGGL(sp3d_conv_mfma<32>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(sp3d_conv_mfma<64>, grid, dim3(256), 0, stream, a);
    return coalign::check_launch();
}

extern "C" int coalign_sp3d_to_dense(const float *feat, const int *count, int capacity, int C, const void *index, size_t index_bytes, int N, int D, int H, int W, float *out,
                                     void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!grid_ok(N, D, H, W) || capacity < 0 || C < 1) return COALIGN_ERR_BAD_SHAPE;
    if ((size_t)N * (size_t)H * (size_t)W * (size_t)C * (size_t)D > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (index_bytes < layout_of(N, D, H, W, capacity).bytes) return COALIGN_ERR_WORKSPACE;
    if (!count || !index || !out || (capacity > 0 && !feat)) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(feat, 15) || misaligned(index, 15) || misaligned(out, 15) || misaligned(count, 3)) return COALIGN_ERR_NULL_POINTER;
    const Index ix = view_of(const_cast<void *>(index), N, D, H, W, capacity);
    hipLaunchKernelGGL(sp3d_to_dense, dim3(blocks_for((size_t)N * H * W, 4)), dim3(256), 0, stream, feat, count, C, ix, out);
    return coalign::check_launch();
}

// ---- points -> the input sparse tensor with its site index (include_open/coalign_amd_sp3d_voxelize.h) -----------------------------------------------------------
// The dense grid is far too large for per-cell tables (90 M cells per agent), but the site index turns a cell into a small number: marking the points' cells in the
// bitmap and running the prefix count gives every point a PROVISIONAL ROW (the rank of its cell among the occupied cells, ascending in the cell index) by one
// lookup.  Everything per voxel then lives in tables of P_cap rows:
//   vox_mark        per point: the cloud (device offsets, clamped and made non-decreasing), filters, cell -> cell[p]; atomicOr into the bitmap; sel[.][p] <- INT_MAX.
//   (prefix count)  provisional rows.
//   vox_first       per point: prow[p] = the provisional row; atomicMin(sel[0][row], p): the opening point of the cell.
//   vox_round t     t = 1 .. T - 1: atomicMin(sel[t][row], p) over the points with p > sel[t - 1][row]: the T smallest point indices of a cell, ascending.
//   vox_head_count  per 1024-point block of a cloud: its opening points.
//   vox_cut         voxel number = opening points of the cloud in front (block counts + scan); a cell whose number >= max_voxels loses its bit and raises `dirty`;
//                   per-cloud kept counts, the max_voxels status bit.
//   (prefix count)  again, gated by `dirty`: three empty launches for a frame no cloud of which was cut.
//   vox_emit        per provisional row whose bit survives: final row = its rank; mean of its <= T points in ascending point order, indices, perm[row] = row; the
//                   count and the overflow bit.
// Integer atomics only; every result is a minimum or a bit, so the order of arrival does not matter.
namespace {

constexpr int VOX_CHUNK = 1024;            // points per workgroup of the head kernels: 256 lanes x 4 consecutive points
constexpr int VOX_NONE = 0x7fffffff;

struct VoxSites {
    const float4 *pts;
    const int *offsets;
    int P_cap, n_clouds, max_blocks;
    float lo[3], vs[3];
    int grid[3];                            // the voxel grid (x, y, z)
    int T, max_voxels, flags;
    float flo[3], fhi[3];
    int *cell, *prow, *sel, *blocksum, *dirty;
    float4 *features;
    int4 *indices;
    int *count, *cloud_counts;
    unsigned *status;
};

__device__ __forceinline__ int vox_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the cloud that owns point p, or -1 (offsets clamped to [0, P_cap], non-decreasing by a running maximum)
__device__ __forceinline__ int vox_cloud_of(const VoxSites &a, int p) {
    int start = vox_clamp(a.offsets[0], a.P_cap), cloud = -1;
    for (int c = 0; c < a.n_clouds; ++c) {
        int end = vox_clamp(a.offsets[c + 1], a.P_cap);
        end = end < start ? start : end;
        if (p >= start && p < end) cloud = c;
        start = end;
    }
    return cloud;
}

__device__ __forceinline__ void vox_span_of(const VoxSites &a, int cloud, int &begin, int &end) {
    int start = vox_clamp(a.offsets[0], a.P_cap);
    begin = end = start;
    for (int c = 0; c <= cloud; ++c) {
        int e = vox_clamp(a.offsets[c + 1], a.P_cap);
        e = e < start ? start : e;
        begin = start;
        end = e;
        start = e;
    }
}

// the voxel (x, y, z) of a point or false: the expression of cell_of() in voxelize.hip
__device__ __forceinline__ bool vox_coords(const VoxSites &a, const float4 p, int &x, int &y, int &z) {
    if (a.flags & COALIGN_VOX_FILTER_EGO) {      // pcd_utils.py:69-88, closed box
        if (p.x >= -1.95f && p.x <= 2.95f && p.y >= -1.1f && p.y <= 1.1f) return false;
    }
    if (a.flags & COALIGN_VOX_FILTER_RANGE) {    // pcd_utils.py:41-66, strict
        if (!(p.x > a.flo[0] && p.x < a.fhi[0] && p.y > a.flo[1] && p.y < a.fhi[1] && p.z > a.flo[2] && p.z < a.fhi[2])) return false;
    }
    const float cx = floorf((p.x - a.lo[0]) / a.vs[0]);
    const float cy = floorf((p.y - a.lo[1]) / a.vs[1]);
    const float cz = floorf((p.z - a.lo[2]) / a.vs[2]);
    // NaN coordinates fail every comparison and are rejected
    if (!(cx >= 0.0f && cx < (float)a.grid[0] && cy >= 0.0f && cy < (float)a.grid[1] && cz >= 0.0f && cz < (float)a.grid[2])) return false;
    x = (int)cx; y = (int)cy; z = (int)cz;
    return true;
}

// the rank of an occupied cell among the occupied cells (no capacity, no rank -> row table)
__device__ __forceinline__ int vox_rank(const Index &ix, int cell, bool &set) {
    const unsigned m = ix.bits[cell >> 5], bit = (unsigned)cell & 31u;
    set = (m >> bit) & 1u;
    return ix.prefix[cell >> 5] + __popc(m & ((1u << bit) - 1u));
}

__global__ __launch_bounds__(256) void vox_mark(const VoxSites a, const Index ix) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0) *a.dirty = 0;
    if (p >= a.P_cap) return;
    for (int t = 0; t < a.T; ++t) a.sel[(size_t)t * a.P_cap + p] = VOX_NONE;
    const int cloud = vox_cloud_of(a, p);
    int cell = -1, x, y, z;
    if (cloud >= 0 && vox_coords(a, a.pts[p], x, y, z)) {
        cell = cell_of(ix.g, cloud, z, y, x);
        atomicOr(&ix.bits[cell >> 5], 1u << (cell & 31));
    }
    a.cell[p] = cell;
}

__global__ __launch_bounds__(256) void vox_first(const VoxSites a, const Index ix) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.P_cap) return;
    const int cell = a.cell[p];
    int row = -1;
    if (cell >= 0) {
        bool set;
        row = vox_rank(ix, cell, set);
        if (!set || (unsigned)row >= (unsigned)a.P_cap) row = -1;      // (cannot happen: every marked cell holds a point, so there are at most P_cap of them)
        else atomicMin(&a.sel[row], p);
    }
    a.prow[p] = row;
}

__global__ __launch_bounds__(256) void vox_round(const VoxSites a, int t) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.P_cap) return;
    const int row = a.prow[p];
    if (row < 0) return;
    if (p > a.sel[(size_t)(t - 1) * a.P_cap + row]) atomicMin(&a.sel[(size_t)t * a.P_cap + row], p);
}

// bit k: point i0 + k of the cloud opens its cell
__device__ __forceinline__ unsigned vox_heads(const VoxSites &a, int begin, int n, int i0) {
    unsigned h = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + k;
        if (i >= n) continue;
        const int row = a.prow[begin + i];
        if (row >= 0 && a.sel[row] == begin + i) h |= 1u << k;
    }
    return h;
}

__global__ __launch_bounds__(256) void vox_head_count(const VoxSites a) {
    __shared__ int lds[256];
    const int cloud = blockIdx.y;
    int begin, end;
    vox_span_of(a, cloud, begin, end);
    const unsigned h = vox_heads(a, begin, end - begin, blockIdx.x * VOX_CHUNK + threadIdx.x * 4);
    int total;
    (void)block_scan(__popc(h), lds, total);
    if (threadIdx.x == 0) a.blocksum[cloud * a.max_blocks + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void vox_cut(const VoxSites a, const Index ix) {
    __shared__ int lds[256];
    __shared__ int opened[COALIGN_SP3D_VOXELIZE_MAX_CLOUDS];
    const int cloud = blockIdx.y;
    if (blockIdx.x == 0 && blockIdx.y == 0) {          // the kept voxels of every cloud, their sum, the max_voxels bit
        if ((int)threadIdx.x < a.n_clouds) {
            int s = 0;
            for (int b = 0; b < a.max_blocks; ++b) s += a.blocksum[threadIdx.x * a.max_blocks + b];
            opened[threadIdx.x] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = 0;
            bool reached = false;
            for (int c = 0; c < a.n_clouds; ++c) {
                const int kept = opened[c] < a.max_voxels ? opened[c] : a.max_voxels;
                reached = reached || opened[c] >= a.max_voxels;
                a.cloud_counts[c] = kept;
                sum += kept;
            }
            a.cloud_counts[a.n_clouds] = sum;
            if (reached) *a.status = *a.status | COALIGN_SP3D_STATUS_MAX_VOXELS;
        }
    }
    int before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) before += a.blocksum[cloud * a.max_blocks + b];
    int in_front;
    (void)block_scan(before, lds, in_front);
    int begin, end;
    vox_span_of(a, cloud, begin, end);
    const int i0 = blockIdx.x * VOX_CHUNK + threadIdx.x * 4;
    const unsigned h = vox_heads(a, begin, end - begin, i0);
    int total;
    int number = in_front + block_scan(__popc(h), lds, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(h >> k & 1u)) continue;
        if (number >= a.max_voxels) {                  // the cell would open voxel number >= max_voxels: dropped with all its points
            const int cell = a.cell[begin + i0 + k];
            atomicAnd(&ix.bits[cell >> 5], ~(1u << (cell & 31)));
            *a.dirty = 1;
        }
        ++number;
    }
}

__global__ __launch_bounds__(256) void vox_emit(const VoxSites a, const Index ix) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) {
        const int kept = ix.sums[ix.blocks];
        *a.count = kept > ix.cap ? ix.cap : kept;
        if (kept > ix.cap) *a.status = *a.status | COALIGN_SP3D_STATUS_OVERFLOW;
    }
    if (r >= a.P_cap) return;
    const int p0 = a.sel[r];
    if ((unsigned)p0 >= (unsigned)a.P_cap) return;     // no such provisional row
    const int cell = a.cell[p0];
    if (cell < 0) return;
    bool set;
    const int row = vox_rank(ix, cell, set);
    if (!set || (unsigned)row >= (unsigned)ix.cap) return;      // cut by max_voxels, or past the capacity
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int n = 0;
    for (int t = 0; t < a.T; ++t) {
        const int p = a.sel[(size_t)t * a.P_cap + r];
        if ((unsigned)p >= (unsigned)a.P_cap) break;
        const float4 v = a.pts[p];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        ++n;
    }
    const float d = (float)n;
    a.features[row] = make_float4(s.x / d, s.y / d, s.z / d, s.w / d);
    const int x = cell % ix.g.W, t = cell / ix.g.W, y = t % ix.g.H, u = t / ix.g.H, z = u % ix.g.D, b = u / ix.g.D;
    a.indices[row] = make_int4(b, z, y, x);
    ix.perm[row] = row;
}

struct VoxWorkspace {
    size_t cell, prow, sel, blocksum, dirty, total;
};

VoxWorkspace vox_layout(int P_cap, int n_clouds, int T) {
    VoxWorkspace w;
    size_t o = 0;
    auto take = [&](size_t ints) { const size_t at = o; o = align_up(o + ints * sizeof(int), 256); return at; };
    w.cell = take((size_t)P_cap);
    w.prow = take((size_t)P_cap);
    w.sel = take((size_t)P_cap * T);
    w.blocksum = take((size_t)n_clouds * ((P_cap + VOX_CHUNK - 1) / VOX_CHUNK));
    w.dirty = take(1);
    w.total = o;
    return w;
}

bool vox_sizes_ok(int P_cap, int n_clouds, int T) {
    return P_cap >= 1 && P_cap <= COALIGN_SP3D_VOXELIZE_MAX_P_CAP && n_clouds >= 1 && n_clouds <= COALIGN_SP3D_VOXELIZE_MAX_CLOUDS && T >= 1 &&
           T <= COALIGN_SP3D_VOXELIZE_MAX_POINTS;
}

}  // namespace

extern "C" size_t coalign_sp3d_voxelize_workspace_bytes(int P_cap, int n_clouds, int max_points) {
    if (!vox_sizes_ok(P_cap, n_clouds, max_points)) return 0;
    return vox_layout(P_cap, n_clouds, max_points).total;
}

extern "C" int coalign_sp3d_voxelize(const float *points, const int *offsets, int P_cap, int n_clouds, const double *voxel_size, const double *lidar_range, int D, int H,
                                     int W, int max_points, int max_voxels, int flags, const double *filter_range, float *features, int *indices, int *count,
                                     int *cloud_counts, int capacity, void *index, size_t index_bytes, unsigned *status, void *workspace, size_t workspace_bytes,
                                     void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!voxel_size || !lidar_range) return COALIGN_ERR_NULL_POINTER;
    if (P_cap < 1 || P_cap > COALIGN_SP3D_VOXELIZE_MAX_P_CAP || capacity < 1 || n_clouds < 1 || max_voxels < 1 || max_points < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n_clouds > COALIGN_SP3D_VOXELIZE_MAX_CLOUDS || max_points > COALIGN_SP3D_VOXELIZE_MAX_POINTS) return COALIGN_ERR_UNSUPPORTED;
    if (flags & ~(COALIGN_VOX_FILTER_EGO | COALIGN_VOX_FILTER_RANGE)) return COALIGN_ERR_UNSUPPORTED;
    if ((flags & COALIGN_VOX_FILTER_RANGE) && !filter_range) return COALIGN_ERR_NULL_POINTER;
    VoxSites a{};
    for (int j = 0; j < 3; ++j) {   // float32 round((max - min) / voxel), sp_voxel_preprocessor.py:40-42, as coalign_voxelize
        const float q = ((float)lidar_range[3 + j] - (float)lidar_range[j]) / (float)voxel_size[j];
        if (!(q >= 0.5f && q < 65536.0f)) return COALIGN_ERR_BAD_SHAPE;
        a.grid[j] = (int)nearbyintf(q);
    }
    if (!grid_ok(n_clouds, D, H, W) || W != a.grid[0] || H != a.grid[1] || D < a.grid[2]) return COALIGN_ERR_BAD_SHAPE;
    if (index_bytes < layout_of(n_clouds, D, H, W, capacity).bytes) return COALIGN_ERR_WORKSPACE;
    const VoxWorkspace w = vox_layout(P_cap, n_clouds, max_points);
    if (workspace_bytes < w.total) return COALIGN_ERR_WORKSPACE;
    if (!points || !offsets || !features || !indices || !count || !cloud_counts || !index || !status || !workspace) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(points, 15) || misaligned(features, 15) || misaligned(indices, 15) || misaligned(index, 15) || misaligned(workspace, 15) || misaligned(offsets, 3) ||
        misaligned(count, 3) || misaligned(cloud_counts, 3) || misaligned(status, 3))
        return COALIGN_ERR_NULL_POINTER;
    char *ws = static_cast<char *>(workspace);
    a.pts = reinterpret_cast<const float4 *>(points);
    a.offsets = offsets;
    a.P_cap = P_cap;
    a.n_clouds = n_clouds;
    a.max_blocks = (P_cap + VOX_CHUNK - 1) / VOX_CHUNK;
    for (int j = 0; j < 3; ++j) {
        a.lo[j] = (float)lidar_range[j];
        a.vs[j] = (float)voxel_size[j];
        if (flags & COALIGN_VOX_FILTER_RANGE) {
            a.flo[j] = (float)filter_range[j];
            a.fhi[j] = (float)filter_range[3 + j];
        }
    }
    a.T = max_points;
    a.max_voxels = max_voxels;
    a.flags = flags;
    a.cell = reinterpret_cast<int *>(ws + w.cell);
    a.prow = reinterpret_cast<int *>(ws + w.prow);
    a.sel = reinterpret_cast<int *>(ws + w.sel);
    a.blocksum = reinterpret_cast<int *>(ws + w.blocksum);
    a.dirty = reinterpret_cast<int *>(ws + w.dirty);
    a.features = reinterpret_cast<float4 *>(features);
    a.indices = reinterpret_cast<int4 *>(indices);
    a.count = count;
    a.cloud_counts = cloud_counts;
    a.status = status;
    const Index ix = view_of(index, n_clouds, D, H, W, capacity);
    const dim3 per_point(blocks_for((size_t)P_cap, 256)), per_chunk((unsigned)a.max_blocks, (unsigned)n_clouds);
    int rc = coalign::fill_words(ix.bits, (size_t)ix.words, 0u, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(vox_mark, per_point, dim3(256), 0, stream, a, ix);
    rc = coalign::check_launch();
    if (rc) return rc;
    rc = prefix_count(ix, nullptr, nullptr, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(vox_first, per_point, dim3(256), 0, stream, a, ix);
    for (int t = 1; t < max_points; ++t) hipLaunchKernelGGL(vox_round, per_point, dim3(256), 0, stream, a, t);
    hipLaunchKernelGGL(vox_head_count, per_chunk, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(vox_cut, per_chunk, dim3(256), 0, stream, a, ix);
    rc = coalign::check_launch();
    if (rc) return rc;
    rc = prefix_count(ix, nullptr, nullptr, stream, a.dirty);
    if (rc) return rc;
    hipLaunchKernelGGL(vox_emit, per_point, dim3(256), 0, stream, a, ix);
    return coalign::check_launch();
}
