// V2X-ViT's pyramid window attention with split attention on CHANNELS-LAST maps, gfx950: x + PyramidWindowAttention(LayerNorm(x)) for the n maps of one frame.
//
// Reference semantics (eval mode): PyramidWindowAttention over BaseWindowAttention, sub_modules/mswin.py:19-121, SplitAttn with RadixSoftmax, split_attn.py:6-63,
// under PreNorm (base_transformer.py:7-14) and the residual of V2XFusionBlock.forward (v2xvit_basic.py:118-122).  Branch b = 0, 1, 2 has windows of ws = 4, 8, 16
// tokens a side and heads of dh = 16, 32, 64 channels:
//   y     = LayerNorm(x)
//   o_b   = softmax_j( q_i . k_j / sqrt(dh) + pos_b[xj - xi + ws - 1][yj - yi + ws - 1] ) v_j        inside every window, per head
//   out   = x + sum_b a_b * (Wout_b o_b + bout_b)          a_b = 1 / 3, or the split attention's softmax over the branches per (map, channel)
// The host folds gamma / beta and the three scales into ONE 9C x C projection (float64, once per parameter change).  The split attention pools
// sum_b (Wout_b o_b + bout_b) over the map; that is linear in o_b, so the per-map channel means of o_b suffice and no second pass over projected maps is needed.
//
// Launch 1 (project): v2x_attn.hip's project kernel with 9C rows and no warp: a workgroup (4 wavefronts) owns 32 consecutive pixels of one map, yhat as sp16 pairs in
//   an LDS tile, the 9C / 32 row tiles dealt over the wavefronts on v_mfma_f32_32x32x16_f16, [q | k | v] x 3 to the workspace [map][pixel][9C] as fp32.
// Launch 2 (attend): one thread per (map, branch, window, head, query token), the query and its output row in registers, the keys of the window visited in blocks
//   of 16 with an online softmax (one rescale per block).  For ws = 8 and 16 a wavefront's 64 queries share window and head, so every key / value address is
//   wavefront-uniform: k and v come through the scalar data cache into scalar registers, no LDS and no vector memory traffic for them.  ws = 4 (four windows x heads
//   per wavefront, 5 % of the products) loads them per lane.  The position table sits in LDS.  Scores, bias, softmax (hardware exponential) and the weighted sum are
//   fp32 on the VALU.  o_b goes out in raster token order [map][pixel][3C]; with split attention every (window, head) group of lanes also adds its o over its tokens
//   (a fixed butterfly) and writes that partial sum.
// Launch 3 (split weights, split attention only): one workgroup per map adds the partial sums in a fixed order (four slices in index order each), then gap, fc1, LayerNorm, ReLU, fc2 and the softmax
//   over the branches in fp32 -> a [map][3][C].
// Launch 4 (output): per 32-pixel tile and branch, o_b as sp16 pairs into the LDS tile, Wout_b through the row tiles with bout_b seeding the accumulators, scaled per
//   channel by a_b; after the third branch the residual x is added and the sum stored with streaming stores.
// No atomics: the same input gives the same bits.  The caller's stream, no allocation: capturable.
#include "common.h"
#include "sp16_tiles.h"

#include "coalign_amd_v2x_window.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));


__host__ __device__ constexpr size_t off_wout(int C) { return image_bytes(9 * C, C); }
__host__ __device__ constexpr size_t off_floats(int C) { return off_wout(C) + 3 * image_bytes(C, C); }
__host__ __device__ constexpr size_t off_split(int C) { return off_floats(C) + ((size_t)12 * C + COALIGN_V2X_WINDOW_POS_FLOATS) * 4; }
__host__ __device__ constexpr size_t param_bytes(int C, int fuse) { return off_split(C) + (fuse ? ((size_t)7 * C * C + 2 * C) * 4 : 0); }
__host__ __device__ constexpr size_t lds_bytes(int C) { return (size_t)TP * x_row_bytes(C); }

struct WinArgs {
    const float *x;          // [n, H, W, C]
    const unsigned char *params;
    float *qkv;              // workspace [n, H W, 9C]
    float *o;                // workspace [n, H W, 3C]
    float *part;             // workspace [n, 3, H W / 16, C]
    float *a;                // workspace [n, 3, C]
    float *out;              // [n, H, W, C]
    int n, C, H, W, fuse;
};

// ---- launch 1: [q | k | v] of the three branches for one map's 32 pixels -> workspace (H W is a multiple of 256: every tile is whole) -----------------------------
template <int MAXI>      // items (pixel, 8-channel group) per lane: 32 * (C / 8) / 256
__global__ __launch_bounds__(256) void window_project_kernel(const WinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = a.C, G = C / 8, steps = C / 16, xrow_b = x_row_bytes(C);
    char *xt = lds;
    const int HW = a.H * a.W;
    const int tiles_px = HW / TP;
    const int agent = blockIdx.x / tiles_px;
    const int pix0 = (blockIdx.x - agent * tiles_px) * TP;
    const float *plane = a.x + (size_t)agent * HW * C;
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
        const int idx = it * 256 + tid;
        const int ip = idx / G, ig = idx - ip * G;
        const float4 *src = reinterpret_cast<const float4 *>(plane + (size_t)(pix0 + ip) * C + ig * 8);
        const float4 v0 = src[0], v1 = src[1];
        float X[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
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
        const float rstd = 1.0f / sqrtf(pixel_sum(d, G) / (float)C + COALIGN_V2X_WINDOW_LN_EPS);
#pragma unroll
        for (int j = 0; j < 8; ++j) X[j] *= rstd;
        store_split8(xt + ip * xrow_b + ig * 32, X);
    }
    __syncthreads();

    const int col = lane & 31, half = lane >> 5;
    const char *xrow = xt + col * xrow_b;
    const int tiles = 9 * C / 32;
    const float *bias = reinterpret_cast<const float *>(a.params + off_floats(C));
    float *dst = a.qkv + ((size_t)agent * HW + pix0 + col) * (9 * C);
    for (int t = wave; t < tiles; t += 4) {
        const floatx16 r = row_tile(a.params, tiles, t, bias, lane, xrow, steps);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4 *>(dst + 32 * t + 8 * i + 4 * half) = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
    }
}

// ---- launch 2: attention inside the windows -------------------------------------------------------------------------------------------------------------------
// four floats of the projections: through the scalar data cache where the address is the same in every lane (this launch only reads the projections)
template <bool UNI>
__device__ __forceinline__ f4 load4(const float *p) {
    if constexpr (UNI) {
        return *(const __attribute__((address_space(4))) f4 *)(p);
    } else {
        return *reinterpret_cast<const f4 *>(p);
    }
}

template <int WS, int DH, bool UNI>
__device__ __forceinline__ void attend_branch(const WinArgs &a, const int b, const int block, float *pos) {
    constexpr int T = WS * WS, PW = 2 * WS - 1, KB = 16;      // keys per online-softmax block
    const int tid = threadIdx.x;
    const int C = a.C, heads = C / DH, HW = a.H * a.W, nw = a.W / WS, nwin = (a.H / WS) * nw;
    const size_t tok = (size_t)9 * C;
    {
        const float *tab = reinterpret_cast<const float *>(a.params + off_floats(C)) + 12 * C + (b == 0 ? 0 : b == 1 ? 49 : 49 + 225);      // 7 x 7, 15 x 15, 31 x 31
        for (int i = tid; i < PW * PW; i += 256) pos[i] = tab[i];
        __syncthreads();
    }
    const int g = block * 256 + tid;                           // < n H W heads <= 2^30
    int unit = g / T;
    const int qi = g - unit * T;
    if constexpr (UNI) unit = __builtin_amdgcn_readfirstlane(unit);
    const int win = unit / heads, head = unit - win * heads;
    const int agent = win / nwin, wr = win - agent * nwin;
    const int wy = wr / nw, wx = wr - wy * nw;
    const int qr = qi / WS, qc = qi - qr * WS;
    const float *base = a.qkv + ((size_t)agent * HW + (size_t)wy * WS * a.W + wx * WS) * tok + b * 3 * C + head * DH;
    const int qpix = qr * a.W + qc;                            // the query's pixel relative to the window's corner
    const float *ptab = pos + ((WS - 1) * PW + (WS - 1) - (qr * PW + qc));

    float q[DH], o[DH];
    {
        const f4 *src = reinterpret_cast<const f4 *>(base + (size_t)qpix * tok);
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
            const f4 v = src[c];
            q[4 * c] = v[0]; q[4 * c + 1] = v[1]; q[4 * c + 2] = v[2]; q[4 * c + 3] = v[3];
        }
    }
#pragma unroll
    for (int c = 0; c < DH; ++c) o[c] = 0.f;
    float m = -INFINITY, l = 0.f;
#pragma unroll 1
    for (int jb = 0; jb < T; jb += KB) {
        float s[KB];
#pragma unroll
        for (int jj = 0; jj < KB; ++jj) {
            const int j = jb + jj, jr = j / WS, jc = j - jr * WS;
            const float *kp = base + (size_t)(jr * a.W + jc) * tok + C;
            float d = ptab[jr * PW + jc];
#pragma unroll
            for (int c = 0; c < DH / 4; ++c) {
                const f4 v = load4<UNI>(kp + 4 * c);
                d = fmaf(q[4 * c], v[0], d); d = fmaf(q[4 * c + 1], v[1], d); d = fmaf(q[4 * c + 2], v[2], d); d = fmaf(q[4 * c + 3], v[3], d);
            }
            s[jj] = d;
        }
        float mb = s[0];
#pragma unroll
        for (int jj = 1; jj < KB; ++jj) mb = fmaxf(mb, s[jj]);
        const float mn = fmaxf(m, mb);
        const float rescale = __expf(m - mn);                  // (first block: exp(-inf) = 0 on zeros)
        m = mn;
        l *= rescale;
#pragma unroll
        for (int c = 0; c < DH; ++c) o[c] *= rescale;
#pragma unroll
        for (int jj = 0; jj < KB; ++jj) {
            const int j = jb + jj, jr = j / WS, jc = j - jr * WS;
            const float *vp = base + (size_t)(jr * a.W + jc) * tok + 2 * C;
            const float p = __expf(s[jj] - mn);
            l += p;
#pragma unroll
            for (int c = 0; c < DH / 4; ++c) {
                const f4 v = load4<UNI>(vp + 4 * c);
                o[4 * c] = fmaf(p, v[0], o[4 * c]); o[4 * c + 1] = fmaf(p, v[1], o[4 * c + 1]);
                o[4 * c + 2] = fmaf(p, v[2], o[4 * c + 2]); o[4 * c + 3] = fmaf(p, v[3], o[4 * c + 3]);
            }
        }
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int c = 0; c < DH; ++c) o[c] *= inv;
    {
        const size_t pix = (size_t)wy * WS * a.W + wx * WS + qpix;
        f4 *dst = reinterpret_cast<f4 *>(a.o + ((size_t)agent * HW + pix) * (3 * C) + b * C + head * DH);
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) dst[c] = f4{o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]};
    }
    if (a.fuse) {
        // the sum of o over the group's tokens: 64 lanes (one wavefront) for ws = 8 / 16, 16 lanes for ws = 4; a butterfly, so the order is fixed
        constexpr int GL = UNI ? 64 : 16;
#pragma unroll
        for (int c = 0; c < DH; ++c)
#pragma unroll
            for (int off = GL >> 1; off > 0; off >>= 1) o[c] += __shfl_xor(o[c], off);
        if ((tid & (GL - 1)) == 0) {
            const int chunk = WS == 16 ? wr * 4 + (qi >> 6) : wr;
            f4 *dst = reinterpret_cast<f4 *>(a.part + (((size_t)agent * 3 + b) * (HW / 16) + chunk) * C + head * DH);
#pragma unroll
            for (int c = 0; c < DH / 4; ++c) dst[c] = f4{o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]};
        }
    }
}

__global__ __launch_bounds__(256) void window_attend_kernel(const WinArgs a) {
    __shared__ float pos[31 * 31];
    // the blocks of the 16 x 16 branch first: they run longest
    const int per = a.n * a.H * a.W / 256;                     // blocks per head of a branch
    const int nb2 = per * (a.C / 64), nb1 = per * (a.C / 32);
    const int block = blockIdx.x;
    if (block < nb2) attend_branch<16, 64, true>(a, 2, block, pos);
    else if (block < nb2 + nb1) attend_branch<8, 32, true>(a, 1, block - nb2, pos);
    else attend_branch<4, 16, false>(a, 0, block - nb2 - nb1, pos);
}

// ---- launch 3: the split attention's branch weights per map (4 C threads: channel c = tid % C, slice ks = tid / C of every sum) ------------------------------------
// Every sum over chunks or input channels is cut into four slices, one per ks, each added in index order; the four slice sums are added in slice order.
__global__ __launch_bounds__(1024) void window_split_kernel(const WinArgs a) {
    __shared__ float mean[3 * 256], vec[256], hid[256], red[4 * 3 * 256];
    const int C = a.C, HW = a.H * a.W, agent = blockIdx.x;
    const int ks = threadIdx.x / C, c = threadIdx.x - ks * C;
    const float *fl = reinterpret_cast<const float *>(a.params + off_floats(C));
    const float *bout = fl + 9 * C;
    const float *sp = reinterpret_cast<const float *>(a.params + off_split(C));
    const float *woutT = sp, *fc1T = sp + (size_t)3 * C * C, *lng = fc1T + (size_t)C * C, *lnb = lng + C, *fc2T = lnb + C;
    const int k0 = ks * (C / 4), k1 = k0 + C / 4;
    for (int b = 0; b < 3; ++b) {
        const int chunks = b == 0 ? HW / 16 : HW / 64;         // (multiples of four: H W is a multiple of 256)
        const float *p = a.part + ((size_t)agent * 3 + b) * (HW / 16) * C + c;
        float s = 0.f;
#pragma unroll 8
        for (int i = ks * (chunks / 4); i < (ks + 1) * (chunks / 4); ++i) s += p[(size_t)i * C];
        red[(ks * 3 + b) * C + c] = s;
    }
    __syncthreads();
    if (ks == 0)
        for (int b = 0; b < 3; ++b) mean[b * C + c] = (((red[b * C + c] + red[(3 + b) * C + c]) + red[(6 + b) * C + c]) + red[(9 + b) * C + c]) / (float)HW;
    __syncthreads();
    {
        float d = 0.f;
        for (int b = 0; b < 3; ++b)
#pragma unroll 8
            for (int k = k0; k < k1; ++k) d = fmaf(woutT[((size_t)b * C + k) * C + c], mean[b * C + k], d);
        red[ks * C + c] = d;
    }
    __syncthreads();
    if (ks == 0) vec[c] = ((bout[c] + bout[C + c]) + bout[2 * C + c]) + (((red[c] + red[C + c]) + red[2 * C + c]) + red[3 * C + c]);
    __syncthreads();
    {
        float h = 0.f;
#pragma unroll 8
        for (int k = k0; k < k1; ++k) h = fmaf(fc1T[(size_t)k * C + c], vec[k], h);
        red[4 * C + ks * C + c] = h;                           // (a second quarter of red: the first may still be read)
    }
    __syncthreads();
    if (ks == 0) hid[c] = ((red[4 * C + c] + red[5 * C + c]) + red[6 * C + c]) + red[7 * C + c];
    __syncthreads();
    float mu = 0.f;
    for (int k = 0; k < C; ++k) mu += hid[k];
    mu /= (float)C;
    float var = 0.f;
    for (int k = 0; k < C; ++k) var = fmaf(hid[k] - mu, hid[k] - mu, var);
    var /= (float)C;
    if (ks == 0) vec[c] = fmaxf((hid[c] - mu) / sqrtf(var + COALIGN_V2X_WINDOW_LN_EPS) * lng[c] + lnb[c], 0.f);
    __syncthreads();
    {
        float z0 = 0.f, z1 = 0.f, z2 = 0.f;
#pragma unroll 8
        for (int k = k0; k < k1; ++k) {
            const float *row = fc2T + (size_t)k * 3 * C + c;
            z0 = fmaf(row[0], vec[k], z0); z1 = fmaf(row[C], vec[k], z1); z2 = fmaf(row[2 * C], vec[k], z2);
        }
        red[(ks * 3 + 0) * C + c] = z0; red[(ks * 3 + 1) * C + c] = z1; red[(ks * 3 + 2) * C + c] = z2;
    }
    __syncthreads();
    if (ks == 0) {
        float z[3];
        for (int j = 0; j < 3; ++j) z[j] = ((red[j * C + c] + red[(3 + j) * C + c]) + red[(6 + j) * C + c]) + red[(9 + j) * C + c];
        const float zm = fmaxf(z[0], fmaxf(z[1], z[2]));
        const float e0 = __expf(z[0] - zm), e1 = __expf(z[1] - zm), e2 = __expf(z[2] - zm);
        const float inv = 1.0f / ((e0 + e1) + e2);
        float *dst = a.a + (size_t)agent * 3 * C + c;
        dst[0] = e0 * inv; dst[C] = e1 * inv; dst[2 * C] = e2 * inv;
    }
}

// ---- launch 4: out = x + sum_b a_b * (Wout_b o_b + bout_b) for one map's 32 pixels -------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void window_output_kernel(const WinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int G = C / 8, steps = C / 16, xrow_b = x_row_bytes(C), MAXI = TP * G / 256, TILES = C / 32, TW = (TILES + 3) / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char *xt = lds;
    const int HW = a.H * a.W;
    const int tiles_px = HW / TP;
    const int agent = blockIdx.x / tiles_px;
    const int pix0 = (blockIdx.x - agent * tiles_px) * TP;
    const int col = lane & 31, half = lane >> 5;
    const char *xrow = xt + col * xrow_b;
    const float *bout = reinterpret_cast<const float *>(a.params + off_floats(C)) + 9 * C;
    floatx16 acc[TW];
#pragma unroll
    for (int ti = 0; ti < TW; ++ti)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[ti][k] = 0.f;
#pragma unroll 1
    for (int b = 0; b < 3; ++b) {
        if (b) __syncthreads();
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const int idx = it * 256 + tid;
            const int ip = idx / G, ig = idx - ip * G;
            const float4 *src = reinterpret_cast<const float4 *>(a.o + ((size_t)agent * HW + pix0 + ip) * (3 * C) + b * C + ig * 8);
            const float4 v0 = src[0], v1 = src[1];
            const float X[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            store_split8(xt + ip * xrow_b + ig * 32, X);
        }
        __syncthreads();
        const unsigned char *img = a.params + off_wout(C) + (size_t)b * image_bytes(C, C);
#pragma unroll
        for (int ti = 0; ti < TW; ++ti) {
            const int t = wave + 4 * ti;
            if (t < TILES) {
                const floatx16 r = row_tile(img, TILES, t, bout + b * C, lane, xrow, steps);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float4 w = make_float4(1.0f / 3.0f, 1.0f / 3.0f, 1.0f / 3.0f, 1.0f / 3.0f);
                    if (a.fuse) w = *reinterpret_cast<const float4 *>(a.a + ((size_t)agent * 3 + b) * C + 32 * t + 8 * i + 4 * half);
                    acc[ti][4 * i] = fmaf(w.x, r[4 * i], acc[ti][4 * i]); acc[ti][4 * i + 1] = fmaf(w.y, r[4 * i + 1], acc[ti][4 * i + 1]);
                    acc[ti][4 * i + 2] = fmaf(w.z, r[4 * i + 2], acc[ti][4 * i + 2]); acc[ti][4 * i + 3] = fmaf(w.w, r[4 * i + 3], acc[ti][4 * i + 3]);
                }
            }
        }
    }
    const size_t pixel = (size_t)agent * HW + pix0 + col;
#pragma unroll
    for (int ti = 0; ti < TW; ++ti) {
        const int t = wave + 4 * ti;
        if (t < TILES) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c0 = 32 * t + 8 * i + 4 * half;
                const float4 xv = *reinterpret_cast<const float4 *>(a.x + pixel * C + c0);
                coalign::store_stream(reinterpret_cast<float4 *>(a.out + pixel * C + c0),
                                      make_float4(xv.x + acc[ti][4 * i], xv.y + acc[ti][4 * i + 1], xv.z + acc[ti][4 * i + 2], xv.w + acc[ti][4 * i + 3]));
            }
        }
    }
}

template <int C>
int launch(const WinArgs &a, hipStream_t stream) {
    // the C = 256 tile (33 KB) stays below the 64 KB of dynamic LDS a kernel gets without asking
    const int HW = a.H * a.W, tiles = HW / TP;
    hipLaunchKernelGGL(window_project_kernel<TP * (C / 8) / 256>, dim3((unsigned)(a.n * tiles)), dim3(256), lds_bytes(C), stream, a);
    int rc = coalign::check_launch();
    if (rc != COALIGN_OK) return rc;
    const int per = a.n * HW / 256;
    hipLaunchKernelGGL(window_attend_kernel, dim3((unsigned)(per * (C / 64 + C / 32 + C / 16))), dim3(256), 0, stream, a);
    rc = coalign::check_launch();
    if (rc != COALIGN_OK) return rc;
    if (a.fuse) {
        hipLaunchKernelGGL(window_split_kernel, dim3((unsigned)a.n), dim3(4 * C), 0, stream, a);
        rc = coalign::check_launch();
        if (rc != COALIGN_OK) return rc;
    }
    hipLaunchKernelGGL(window_output_kernel<C>, dim3((unsigned)(a.n * tiles)), dim3(256), lds_bytes(C), stream, a);
    return coalign::check_launch();
}

bool shape_ok(int C, int fuse) { return (fuse == 0 || fuse == 1) && (C == 256 || (C == 64 && fuse == 0)); }

// floats of the four parts of the workspace, each a multiple of four
struct Parts { size_t qkv, o, part, a; };
Parts parts(int n, int C, int H, int W) {
    const size_t HW = (size_t)H * W;
    return Parts{(size_t)n * HW * 9 * C, (size_t)n * HW * 3 * C, (size_t)n * 3 * (HW / 16) * C, (size_t)n * 3 * C};
}

}  // namespace

extern "C" size_t coalign_v2x_window_param_bytes(int C, int fuse) {
    if (!shape_ok(C, fuse)) return 0;
    return param_bytes(C, fuse);
}

extern "C" size_t coalign_v2x_window_workspace_bytes(int n, int C, int H, int W) {
    if (!shape_ok(C, 0) || n < 1 || n > 8 || H < 1 || W < 1 || H % 16 || W % 16 || (size_t)C * H * W > (size_t)INT32_MAX) return 0;
    const Parts p = parts(n, C, H, W);
    return (p.qkv + p.o + p.part + p.a) * sizeof(float);
}

extern "C" int coalign_v2x_window_attention(const float *x, int n, int C, int H, int W, int fuse, const void *params, size_t params_bytes, float *out,
                                            void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || C < 1 || H < 1 || W < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > 8 || !shape_ok(C, fuse) || H % 16 || W % 16) return COALIGN_ERR_UNSUPPORTED;
    if (n == 0) return COALIGN_OK;
    if (!x || !params || !out || !workspace) return COALIGN_ERR_NULL_POINTER;
    if ((size_t)C * H * W > (size_t)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (params_bytes != param_bytes(C, fuse) || workspace_bytes < coalign_v2x_window_workspace_bytes(n, C, H, W)) return COALIGN_ERR_BAD_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(workspace)) & 15)
        return COALIGN_ERR_UNSUPPORTED;
    const Parts p = parts(n, C, H, W);
    WinArgs a;
    a.x = x; a.params = static_cast<const unsigned char *>(params); a.out = out;
    a.qkv = static_cast<float *>(workspace); a.o = a.qkv + p.qkv; a.part = a.o + p.o; a.a = a.part + p.part;
    a.n = n; a.C = C; a.H = H; a.W = W; a.fuse = fuse;
    return C == 256 ? launch<256>(a, stream) : launch<64>(a, stream);
}
