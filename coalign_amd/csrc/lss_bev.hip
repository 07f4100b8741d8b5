// The two operations of the camera model's BEV encoder that the SplitMap convolutions do not cover, gfx950 (include/coalign_amd_lss_bev.h):
//   conv7x7_s2_sp    the 7 x 7 / stride 2 / pad 3 stem, channels-last float32 in, 64 channels out as a SplitMap
//                    (opencood/models/sub_modules/lss_submodule.py:369-372, 402-404);
//   up2x_concat_sp   bilinear x 2 up-sampling (align_corners = True) of the low map, concatenated behind the skip map, as a SplitMap in one pass
//                    (`Up.forward`, lss_submodule.py:19-38).
//
// ---- conv7x7_s2_sp ---------------------------------------------------------------------------------------------------------------------------------------
// Same arithmetic as conv3x3_sp.hip / conv3x3_narrow.hip: sp16 pairs (common.h) on v_mfma_f32_32x32x16_f16, w_h x_h into one fp32 accumulator, w_h x_l' +
// w_l' x_h into a second one that enters with 2^-10, the per-channel power-of-two weight scale undone in the epilogue.  The input is float32 and is split by
// the loader (the "consumer split" of conv3x3_emu.hip): sp16_split2, i.e. the pairs coalign_sp_pack would have stored, bit for bit.
//
// Implicit GEMM, K = 49 Cin: one matrix instruction = the 16 channels of one tap (lanes 0-31 channels 0-7, lanes 32-63 channels 8-15).  A workgroup of 8
// wavefronts owns 8 rows x 32 columns of output pixels and all 64 output channels (two 32 x 32 accumulator tiles x two accumulators per wavefront, one output
// row each).  Per 16-channel interval its input patch is 21 rows x 69 columns.
//
// The LDS layout of the patch.  Output column px under tap kx reads patch column 2 px + kx: at the natural layout the 32 lanes of an operand read would be 32
// bytes apart -- two lanes per bank group, a 2-way conflict on every ds_read_b128.  The loader therefore DE-INTERLEAVES the columns by parity: a patch row is
// [35 even columns | 35 odd columns] of 16-byte groups (8 channels x fp16), and column 2 px + kx is group (kx & 1) 35 + (kx >> 1) + px -- 32 CONSECUTIVE groups
// for the 32 lanes, whatever kx.  ds_read_b128 serves lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and the same of the upper half) per cycle, bank =
// (address / 4) mod 64: consecutive groups i .. i + 31 put each of those sets on 16 different residues mod 16, whatever the base -- conflict-free.  Four planes
// (2 * channel half + term) of 21 x 70 groups: 94 080 bytes, ONE buffer.
// The loader: 4 lanes per pixel, a float4 (4 channels) each, fetched one interval ahead into registers (12 per thread), split and stored as 8-byte halves of a
// group after the interval's last matrix step, behind a barrier of its own (the patch has one buffer).  The padding is zeros made in registers.
//
// Weights: 49 taps x 16 channels x 64 outputs x 2 terms = 200 704 bytes per interval do not fit beside the patch, so a barrier interval is ONE ROW OF TAPS
// (interval, ky): 7 taps, 28 672 contiguous bytes of the image, by LDS-DMA into one of two buffers while the previous row's matrix steps run.
// LDS: 2 x 28 672 (weights) + 94 080 (patch) + 512 (bias, 2^-k_c) = 151 936 bytes, one workgroup per CU, two wavefronts per SIMD.
//
// ---- up2x_concat_sp ----------------------------------------------------------------------------------------------------------------------------------------
// Bound by bytes.  A wavefront covers 8 output pixels x 8 groups of 8 channels: its loads are 8 runs of 256 contiguous bytes (16 bytes per lane along the
// channels), its stores 8 + 8 runs of 128 contiguous bytes (16 bytes per lane along the pixels of a plane).  A group lies wholly in the skip part (a copy
// through sp16_split2) or in the up-sampled part (four taps, weights from the exact integer division, summed in float64 and rounded to float32 once).
#include "common.h"
#include "coalign_amd_lss_bev.h"

namespace {

using namespace coalign;
typedef __attribute__((address_space(3))) void *lptr_t;

constexpr int kWaves = 8, kThreads = 64 * kWaves;
constexpr int kTH = kWaves, kTW = 32;                                 // output tile: a row per wavefront
constexpr int kPH = 2 * kTH + 5, kPWU = 2 * kTW + 5;                  // patch rows, patch columns in use (21 x 69)
constexpr int kPWH = (kPWU + 1) / 2;                                  // groups per column parity (35; the odd half uses 34)
constexpr int kPW = 2 * kPWH;                                         // groups per patch row: [even | odd]
constexpr int kPix = kPH * kPW;                                       // groups per plane (1470)
constexpr int kPatchBytes = 4 * kPix * 16;
constexpr int kWQ = 7 * 2 * 2 * 64, kWBytes = kWQ * 16, kWIns = kWQ / 64;      // one row of taps: 16-byte groups, bytes, DMA instructions (28)
constexpr int kWJ = (kWIns + kWaves - 1) / kWaves;
constexpr int kItems = (4 * kPix + kThreads - 1) / kThreads;          // (pixel, channel quad) items per thread and interval (12)
constexpr size_t kLdsBytes = 2 * (size_t)kWBytes + kPatchBytes + 2 * 64 * sizeof(float);
static_assert(kThreads % 4 == 0, "a thread keeps its channel quad in every item");
static_assert(kLdsBytes <= 160 * 1024, "does not fit the 160 KB LDS");

struct StemArgs {
    const float *__restrict__ x;        // [N, H, W, Cin]
    const uint4 *__restrict__ wt;       // weight image
    const float *__restrict__ bias, *__restrict__ wscale;      // wscale: [64] 2^-k_c
    uint4 *__restrict__ y;              // SplitMap [N, 64, Ho, Wo]
    int *range_flag;                    // may be NULL
    int N, Cin, H, W, Ho, Wo, relu, tiles_x, tiles_y;
};

__global__ __launch_bounds__(kThreads) void conv7x7_s2_sp(const StemArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, half = lane >> 5, p = lane & 31;
    const int chunks = a.Cin / 16, HWo = a.Ho * a.Wo;
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)lds;
    constexpr unsigned kPatch0 = 2 * kWBytes;
    float *lds_par = reinterpret_cast<float *>(lds + kPatch0 + kPatchBytes);      // bias | 2^-k_c (the first interval's wait + barrier orders these stores before the epilogue)
    if (tid < 64) {
        lds_par[tid] = a.bias[tid];
        lds_par[64 + tid] = a.wscale[tid];
    }
    int t = blockIdx.x;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y, n = t / a.tiles_y;
    const int y0 = ty * kTH, x0 = tx * kTW;                             // output pixel of the tile's corner; patch group (row, column) <-> input pixel (2 y0 - 3 + row, 2 x0 - 3 + column)

    auto issue_weights = [&](int it, int slot) {                        // row of taps `it` = interval * 7 + ky: 28 672 contiguous bytes
#pragma unroll
        for (int k = 0; k < kWJ; ++k) {
            const int ins = wave + kWaves * k;
            if (ins < kWIns) lds_dma16(a.wt + (size_t)it * kWQ + ins * 64 + lane, lds0 + slot * kWBytes + ins * 1024);
        }
    };
    // item j of this thread: patch group i = (tid >> 2) + (kThreads / 4) j, channel quad tid & 3 of the interval's 16 channels
    const int quad = tid & 3;
    float4 pv[kItems];
    auto stage_load = [&](int c) {
        const float *src = a.x + (size_t)n * a.H * a.W * a.Cin + 16 * c + 4 * quad;
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int i = (tid >> 2) + (kThreads / 4) * j;
            const int row = i / kPW, r = i - row * kPW, par = r >= kPWH ? 1 : 0, col = 2 * (r - par * kPWH) + par;
            const int gy = 2 * y0 - 3 + row, gx = 2 * x0 - 3 + col;
            const bool ok = i < kPix && col < kPWU && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            pv[j] = float4{0.f, 0.f, 0.f, 0.f};
            if (ok) pv[j] = *reinterpret_cast<const float4 *>(src + ((size_t)gy * a.W + gx) * a.Cin);
        }
    };
    auto stage_store = [&]() {                                          // four channels -> 8 bytes of h and 8 bytes of l', each into its half of the group [channel half][term][pixel]
        uint2 *pb = reinterpret_cast<uint2 *>(lds + kPatch0);
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int i = (tid >> 2) + (kThreads / 4) * j;
            unsigned h01, l01, h23, l23;
            coalign::sp16_split2(pv[j].x, pv[j].y, h01, l01);
            coalign::sp16_split2(pv[j].z, pv[j].w, h23, l23);
            if (i < kPix) {
                const int grp = (2 * (quad >> 1)) * kPix + i;
                pb[(size_t)grp * 2 + (quad & 1)] = uint2{h01, h23};
                pb[(size_t)(grp + kPix) * 2 + (quad & 1)] = uint2{l01, l23};
            }
        }
    };

    issue_weights(0, 0);
    stage_load(0);
    stage_store();
    const int gy = y0 + wave, gx = x0 + p;
    const bool wave_live = gy < a.Ho;                                   // (wave-uniform)
    const bool live = wave_live && gx < a.Wo;
    floatx16 acc[2] = {floatx16{0}, floatx16{0}}, accl[2] = {floatx16{0}, floatx16{0}};
    const int wlane = half * 64 + p;                                    // this lane's group inside one (tap, term) weight block, first accumulator tile
    const int total = chunks * 7;
    for (int it = 0, chunk = 0, ky = 0; it < total; ++it) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        const bool next_patch = ky == 0 && chunk + 1 < chunks, store_patch = ky == 6 && chunk + 1 < chunks;
        if (it + 1 < total) issue_weights(it + 1, (it + 1) & 1);
        if (next_patch) stage_load(chunk + 1);
        if (wave_live) {
            const uint4 *bq = reinterpret_cast<const uint4 *>(lds + kPatch0) + 2 * half * kPix + (2 * wave + ky) * kPW + p;
            const uint4 *wq = reinterpret_cast<const uint4 *>(lds + (it & 1) * kWBytes) + wlane;
            halfx8 bc[2], wc[2][2];
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
                bc[tm] = __builtin_bit_cast(halfx8, bq[tm * kPix]);
#pragma unroll
                for (int q = 0; q < 2; ++q) wc[q][tm] = __builtin_bit_cast(halfx8, wq[(tm * 2) * 64 + q * 32]);
            }
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                halfx8 bn[2], wn[2][2];
                if (kx + 1 < 7) {                                      // operands of the next tap are in flight while this tap's matrix instructions issue
                    const int boff = ((kx + 1) & 1) * kPWH + ((kx + 1) >> 1);
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm) {
                        bn[tm] = __builtin_bit_cast(halfx8, bq[tm * kPix + boff]);
#pragma unroll
                        for (int q = 0; q < 2; ++q) wn[q][tm] = __builtin_bit_cast(halfx8, wq[(((kx + 1) * 2 + tm) * 2) * 64 + q * 32]);
                    }
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) accl[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wc[q][0], bc[1], accl[q], 0, 0, 0);      // w_h x_l'
#pragma unroll
                for (int q = 0; q < 2; ++q) accl[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wc[q][1], bc[0], accl[q], 0, 0, 0);      // w_l' x_h
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wc[q][0], bc[0], acc[q], 0, 0, 0);        // w_h x_h
                if (kx + 1 < 7) {
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm) {
                        bc[tm] = bn[tm];
#pragma unroll
                        for (int q = 0; q < 2; ++q) wc[q][tm] = wn[q][tm];
                    }
                }
            }
        }
        if (store_patch) {
            __syncthreads();                                           // every wavefront is done reading the one patch buffer
            stage_store();
        }
        if (++ky == 7) {
            ky = 0;
            ++chunk;
        }
    }
    // ---- epilogue, as conv3x3_narrow.hip's: y = (acc + 2^-10 accl) * 2^-k_c + bias, ReLU, stored as SplitMap pairs
    const float floor_v = a.relu ? 0.f : -__builtin_inff();
    float vmax = 0.f;
    uint4 *ysp = a.y + ((size_t)n * 4 * 4 + half) * HWo + (live ? (size_t)gy * a.Wo + gx : 0);
    const size_t sp_step = 2 * (size_t)HWo;
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) {                                   // groups of 4 consecutive channels per lane: channel = 8 g8 + 4 half + j
        const float4 b4 = reinterpret_cast<const float4 *>(lds_par + 4 * half)[2 * g8], i4 = reinterpret_cast<const float4 *>(lds_par + 64 + 4 * half)[2 * g8];
        const float bb[4] = {b4.x, b4.y, b4.z, b4.w}, ii[4] = {i4.x, i4.y, i4.z, i4.w};
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * (g8 & 3) + j;
            const float s = fmaf(accl[g8 >> 2][e], coalign::kSp16LowInv, acc[g8 >> 2][e]);
            v[j] = fmaxf(s * ii[j] + (0.f + bb[j]), floor_v);         // (the operations of conv3x3_sp.hip without a residual, in its order)
        }
        vmax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fmaxf(fabsf(v[2]), fabsf(v[3])), vmax));
        unsigned h01, l01, h23, l23;
        coalign::sp16_split2(v[0], v[1], h01, l01);
        coalign::sp16_split2(v[2], v[3], h23, l23);
        swap32(h01, l01);          // lanes 0-31: h of channels 0,1 | 4,5 of the 8-channel group; lanes 32-63: l' of the same channels
        swap32(h23, l23);
        if (live) *ysp = uint4{h01, h23, l01, l23};                    // plane = 2 * channel half + term: lanes 32-63 hold term 1 (the `half` in ysp)
        ysp += sp_step;
    }
    if (a.range_flag && live && vmax > 65504.f) atomicOr(a.range_flag, 1);
}

// ---- up2x_concat_sp ---------------------------------------------------------------------------------------------------------------------------------------
struct UpArgs {
    const float *__restrict__ skip, *__restrict__ low;
    uint4 *__restrict__ y;
    int *range_flag;
    int N, Cs, Cl, h, w, cblocks;
    long long pixels;                                                  // N * 2h * 2w
};

__device__ __forceinline__ void store_pairs(uint4 *dst, size_t plane, const float (&v)[8], float &vmax) {
    unsigned h[4], l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        coalign::sp16_split2(v[2 * k], v[2 * k + 1], h[k], l[k]);
        vmax = fmaxf(vmax, fmaxf(fabsf(v[2 * k]), fabsf(v[2 * k + 1])));
    }
    dst[0] = uint4{h[0], h[1], h[2], h[3]};
    dst[plane] = uint4{l[0], l[1], l[2], l[3]};
}

__global__ __launch_bounds__(256) void up2x_concat_sp(const UpArgs a) {
    const long long wv = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;      // wavefront: 8 pixels x 8 groups of 8 channels
    const int lane = threadIdx.x & 63;
    const int C8 = (a.Cs + a.Cl) / 8, c8 = (int)(wv % a.cblocks) * 8 + (lane & 7);
    const long long pix = (wv / a.cblocks) * 8 + (lane >> 3);
    if (c8 >= C8 || pix >= a.pixels) return;
    const int H2 = 2 * a.h, W2 = 2 * a.w;
    const size_t plane = (size_t)H2 * W2;
    const int n = (int)(pix / (long long)plane), r = (int)(pix - (long long)n * plane), Y = r / W2, X = r - Y * W2;
    uint4 *dst = a.y + ((size_t)n * (C8 / 2) * 4 + (size_t)(c8 >> 1) * 4 + 2 * (c8 & 1)) * plane + r;
    float v[8], vmax = 0.f;
    if (8 * c8 < a.Cs) {
        const float4 *s = reinterpret_cast<const float4 *>(a.skip + (size_t)pix * a.Cs + 8 * c8);
        const float4 s0 = s[0], s1 = s[1];
        v[0] = s0.x; v[1] = s0.y; v[2] = s0.z; v[3] = s0.w; v[4] = s1.x; v[5] = s1.y; v[6] = s1.z; v[7] = s1.w;
    } else {
        // source row Y (h - 1) / (2h - 1): integer part and remainder exactly, the fraction = remainder / (2h - 1) in float64
        const long long ny = (long long)Y * (a.h - 1), nx = (long long)X * (a.w - 1);
        const int dy = H2 - 1, dx = W2 - 1, iy0 = (int)(ny / dy), ix0 = (int)(nx / dx);
        const int iy1 = iy0 + 1 < a.h ? iy0 + 1 : a.h - 1, ix1 = ix0 + 1 < a.w ? ix0 + 1 : a.w - 1;
        const double ly = (double)(ny - (long long)iy0 * dy) / (double)dy, lx = (double)(nx - (long long)ix0 * dx) / (double)dx;
        const double w00 = (1.0 - ly) * (1.0 - lx), w01 = (1.0 - ly) * lx, w10 = ly * (1.0 - lx), w11 = ly * lx;
        const float *base = a.low + (size_t)n * a.h * a.w * a.Cl + (8 * c8 - a.Cs);
        const float4 *q00 = reinterpret_cast<const float4 *>(base + ((size_t)iy0 * a.w + ix0) * a.Cl), *q01 = reinterpret_cast<const float4 *>(base + ((size_t)iy0 * a.w + ix1) * a.Cl);
        const float4 *q10 = reinterpret_cast<const float4 *>(base + ((size_t)iy1 * a.w + ix0) * a.Cl), *q11 = reinterpret_cast<const float4 *>(base + ((size_t)iy1 * a.w + ix1) * a.Cl);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float4 t00 = q00[k], t01 = q01[k], t10 = q10[k], t11 = q11[k];
            v[4 * k + 0] = (float)(w00 * t00.x + w01 * t01.x + w10 * t10.x + w11 * t11.x);
            v[4 * k + 1] = (float)(w00 * t00.y + w01 * t01.y + w10 * t10.y + w11 * t11.y);
            v[4 * k + 2] = (float)(w00 * t00.z + w01 * t01.z + w10 * t10.z + w11 * t11.z);
            v[4 * k + 3] = (float)(w00 * t00.w + w01 * t01.w + w10 * t10.w + w11 * t11.w);
        }
    }
    store_pairs(dst, plane, v, vmax);
    if (a.range_flag && vmax > 65504.f) atomicOr(a.range_flag, 1);
}

}  // namespace

extern "C" size_t coalign_conv7x7_s2_weight_bytes(int Cin) {
    if (Cin < 16 || Cin % 16 || Cin > COALIGN_CONV7X7_MAX_CIN) return 0;
    return (size_t)Cin * 49 * COALIGN_CONV7X7_COUT * 2 * 2 + 16 + (size_t)COALIGN_CONV7X7_COUT * 8;
}

extern "C" int coalign_conv7x7_s2_sp(const float *x, const void *w_image, const float *bias, void *y_sp, int N, int Cin, int H, int W, int relu, int32_t *range_flag,
                                     void *stream) {
    if (!x || !w_image || !bias || !y_sp) return COALIGN_ERR_NULL_POINTER;
    if (N < 0 || H < 1 || W < 1 || (int64_t)N * H * W >= (int64_t)1 << 31) return COALIGN_ERR_BAD_SHAPE;
    if (Cin < 16 || Cin % 16 || Cin > COALIGN_CONV7X7_MAX_CIN || (relu != 0 && relu != 1)) return COALIGN_ERR_UNSUPPORTED;
    if (misaligned(x, 15) || misaligned(w_image, 15) || misaligned(y_sp, 15) || misaligned(bias, 3) || misaligned(range_flag, 3)) return COALIGN_ERR_NULL_POINTER;
    if (N == 0) return COALIGN_OK;
    static PerDevice lds_set;
    if (const int rc = allow_dynamic_lds(lds_set, kLdsBytes, conv7x7_s2_sp)) return rc;
    const size_t wbytes = coalign_conv7x7_s2_weight_bytes(Cin), tail = (size_t)COALIGN_CONV7X7_COUT * 8;
    StemArgs a{};
    a.x = x;
    a.wt = static_cast<const uint4 *>(w_image);
    a.bias = bias;
    a.wscale = reinterpret_cast<const float *>(static_cast<const char *>(w_image) + wbytes - tail);
    a.y = static_cast<uint4 *>(y_sp);
    a.range_flag = range_flag;
    a.N = N; a.Cin = Cin; a.H = H; a.W = W; a.relu = relu;
    a.Ho = (H - 1) / 2 + 1;
    a.Wo = (W - 1) / 2 + 1;
    a.tiles_x = (a.Wo + kTW - 1) / kTW;
    a.tiles_y = (a.Ho + kTH - 1) / kTH;
    const int64_t tiles = (int64_t)N * a.tiles_y * a.tiles_x;         // (< 2^31: N H W is)
    hipLaunchKernelGGL(conv7x7_s2_sp, dim3((unsigned)tiles), dim3(kThreads), kLdsBytes, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}

extern "C" int coalign_up2x_concat_sp(const float *skip, const float *low, void *y_sp, int N, int Cs, int Cl, int h, int w, int32_t *range_flag, void *stream) {
    if (!skip || !low || !y_sp) return COALIGN_ERR_NULL_POINTER;
    if (N < 0 || h < 1 || w < 1 || (int64_t)N * (2 * (int64_t)h) * (2 * (int64_t)w) >= (int64_t)1 << 31) return COALIGN_ERR_BAD_SHAPE;
    if (Cs < 16 || Cs % 16 || Cl < 16 || Cl % 16) return COALIGN_ERR_UNSUPPORTED;
    if (misaligned(skip, 15) || misaligned(low, 15) || misaligned(y_sp, 15) || misaligned(range_flag, 3)) return COALIGN_ERR_NULL_POINTER;
    if (N == 0) return COALIGN_OK;
    UpArgs a{};
    a.skip = skip;
    a.low = low;
    a.y = static_cast<uint4 *>(y_sp);
    a.range_flag = range_flag;
    a.N = N; a.Cs = Cs; a.Cl = Cl; a.h = h; a.w = w;
    a.cblocks = ((Cs + Cl) / 8 + 7) / 8;
    a.pixels = (long long)N * (2 * h) * (2 * w);
    const long long waves = ((a.pixels + 7) / 8) * a.cblocks;
    if ((waves + 3) / 4 >= (long long)1 << 31) return COALIGN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(up2x_concat_sp, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}
