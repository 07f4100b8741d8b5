// The two operations of the SECOND detectors' SSFA neck (opencood/models/sub_modules/cia_ssd_utils.py:6-55) that had no kernel, gfx950
// (include_open/coalign_amd_ssfa.h):
//   deconv3x3_s2_sp   ConvTranspose2d 3 x 3 / stride 2 / padding 1 / output_padding 1 + folded BatchNorm + ReLU (+ residual AFTER the activation), SplitMap in,
//                     SplitMap out.  An implicit GEMM at the LOW resolution: the four output parities are four small convolutions (1, 2, 2 and 4 taps) over the
//                     same input patch -- 2.25 taps per output pixel where the zero-stuffed restatement on conv3x3_sp costs 9.  Arithmetic, operand staging
//                     (LDS-DMA of SplitMap planes and of the tap-major weight image, double buffered, one barrier per interval) and epilogue are conv3x3_sp.hip's.
//   ssfa_blend        the two 1-channel 1 x 1 convolutions, the softmax over the two and the weighted sum, one pass over both maps.
// Accumulators: a wavefront owns 32 input pixels x 32 output channels and keeps all four classes in registers, 4 x 2 x 16 = 128 accumulator registers.  With 64
// output channels per wavefront (conv3x3_sp's tile) the four classes would take 256: the operands' prefetch registers no longer fit beside them without
// scratch at two wavefronts per SIMD.  Running the classes one after another over the same patch would read every weight operand from LDS again per class for
// no matrix work saved, so the channel tile was halved instead: a workgroup's eight wavefronts are 4 pixel blocks x 2 channel halves of one 64-channel group.
#include "common.h"
#include "coalign_amd_ssfa.h"

namespace {

using namespace coalign;
typedef __attribute__((address_space(3))) void *lptr_t;

constexpr int kTH = COALIGN_DECONV3X3_TILE_H, kTW = COALIGN_DECONV3X3_TILE_W;      // input pixels of a workgroup: four 2 x 16 blocks, one above the other
constexpr int kWaves = 8, kThreads = 64 * kWaves;
constexpr int kPH = kTH + 1, kPW = kTW + 1;                 // + the row below, the column to the right
constexpr int kPix = kPH * kPW, kPixP = (kPix + 63) / 64 * 64, kPIns = kPixP / 64;      // groups per plane, whole DMA instructions
constexpr int kWQ = 9 * 2 * 2 * 64, kWIns = kWQ / 64;       // 16-byte groups of one interval's weights ([9 taps][2 terms][2 channel halves][64 cout])
constexpr int kWBytes = kWQ * 16, kBBytes = 4 * kPixP * 16;
constexpr int kOps = kWIns + 4 * kPIns, kOpsPerWave = (kOps + kWaves - 1) / kWaves;
constexpr size_t kLdsBytes = 2 * (size_t)kWBytes + 2 * (size_t)kBBytes;      // 98 304
static_assert(kLdsBytes <= 160 * 1024, "does not fit the 160 KB LDS");

struct DeconvArgs {
    const uint4 *__restrict__ x;        // SplitMap [N, Cin, h, w]
    const uint4 *__restrict__ wt;       // tap-major fp16 weight image
    const uint4 *__restrict__ zero;     // its 16 zero bytes
    const float *__restrict__ bias, *__restrict__ winv;      // winv: [Cout] 2^-k_c
    const float *__restrict__ residual; // NULL or channels-last float32 [N, 2h, 2w, Cout]
    uint4 *__restrict__ y;              // SplitMap [N, Cout, 2h, 2w]
    int *range_flag;
    int N, Cin, Cout, h, w, relu, tiles_x, tiles_y, groups;
};

__global__ __launch_bounds__(kThreads, 2) void deconv3x3_s2_sp(const DeconvArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, half = lane >> 5, p = lane & 31;
    const int hw = a.h * a.w, CI16 = a.Cin / 16, CO16 = a.Cout / 16;
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)lds;
    // tile: output-channel group fastest (the groups of one spatial tile are neighbours: they read the same patch), then columns, rows, images
    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int cg = t % a.groups;
    t /= a.groups;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y, n = t / a.tiles_y, y0 = ty * kTH, x0 = tx * kTW;
    const int pb = wave & 3, q = wave >> 2;                    // pixel block, 32-channel half of the group
    const int py = pb * 2 + (p >> 4), px = p & 15;
    const int wlane = half * 64 + q * 32 + p;                  // this lane's group inside one (tap, term) weight block
    const int b00 = 2 * half * kPixP + py * kPW + px;          // group of this lane's pixel inside plane (2 * half + term 0)

    // DMA operation k of the workgroup for interval c: k < kWIns a 1 KB piece of the weights, then piece j of patch plane pl
    const uint4 *wsrc = a.wt + (size_t)cg * CI16 * kWQ + lane;
    const size_t xbase = (size_t)n * CI16 * 4 * hw;
    auto issue = [&](int c, int slot) {
#pragma unroll
        for (int j = 0; j < kOpsPerWave; ++j) {
            const int k = wave + kWaves * j;
            if (k < kWIns) {
                lds_dma16(wsrc + (size_t)c * kWQ + k * 64, lds0 + slot * kWBytes + k * 1024);
            } else if (k < kOps) {
                const int pl = (k - kWIns) / kPIns, ins = (k - kWIns) % kPIns, i = ins * 64 + lane;
                const int yy = i / kPW, gy = y0 + yy, gx = x0 + (i - yy * kPW);
                const bool ok = i < kPix && gy < a.h && gx < a.w;
                lds_dma16(ok ? a.x + xbase + ((size_t)c * 4 + pl) * hw + (size_t)gy * a.w + gx : a.zero, lds0 + 2 * kWBytes + slot * kBBytes + (pl * kPixP + ins * 64) * 16);
            }
        }
    };
    issue(0, 0);
    floatx16 acc[4], accl[4];                                  // class = 2 * (Y mod 2) + (X mod 2)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc[k] = floatx16{0};
        accl[k] = floatx16{0};
    }
    for (int c = 0; c < CI16; ++c) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();                                       // interval c has landed; every wavefront has left interval c - 1, whose buffers the next DMA overwrites
        const int slot = c & 1;
        if (c + 1 < CI16) issue(c + 1, slot ^ 1);
        const uint4 *bq = reinterpret_cast<const uint4 *>(lds + 2 * kWBytes + slot * kBBytes) + b00, *wq = reinterpret_cast<const uint4 *>(lds + slot * kWBytes) + wlane;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            // descending 3 ky + kx: the order in which a 3 x 3 convolution with the flipped kernel meets the non-zero pixels of the zero-stuffed map
            const int s = 8 - r, ky = s / 3, kx = s % 3;
            const int dy = ky == 0, dx = kx == 0, cls = 2 * (ky != 1) + (kx != 1);      // output (2y - 1 + ky, 2x - 1 + kx): ky = 0 belongs to the row pair above
            const halfx8 bh = __builtin_bit_cast(halfx8, bq[dy * kPW + dx]), bl = __builtin_bit_cast(halfx8, bq[kPixP + dy * kPW + dx]);
            const halfx8 wh = __builtin_bit_cast(halfx8, wq[(s * 2 + 0) * 128]), wl = __builtin_bit_cast(halfx8, wq[(s * 2 + 1) * 128]);
            accl[cls] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bl, accl[cls], 0, 0, 0);      // w_h x_l'
            accl[cls] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, bh, accl[cls], 0, 0, 0);      // w_l' x_h
            acc[cls] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bh, acc[cls], 0, 0, 0);        // w_h x_h
        }
    }
    // ---- epilogue (conv3x3_sp.hip's): v = max((acc + 2^-10 accl) 2^-k_c + bias, floor), y = v + residual, stored as pairs
    const int gy = y0 + py, gx = x0 + px, W2 = 2 * a.w;
    const bool live = gy < a.h && gx < a.w;
    const size_t HW2 = 4 * (size_t)hw;
    const int co0 = cg * 64 + q * 32 + 4 * half;               // this lane's channels: co0 + 8 g8 + j
    const float floor_v = a.relu ? 0.f : -__builtin_inff();
    float4 b4[4], i4[4];
#pragma unroll
    for (int g8 = 0; g8 < 4; ++g8) {
        b4[g8] = float4{a.bias[co0 + 8 * g8], a.bias[co0 + 8 * g8 + 1], a.bias[co0 + 8 * g8 + 2], a.bias[co0 + 8 * g8 + 3]};      // (bias is 4-byte aligned only)
        i4[g8] = *reinterpret_cast<const float4 *>(a.winv + co0 + 8 * g8);
    }
    float vmax = 0.f;
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
        const size_t pix = live ? (size_t)(2 * gy + (cls >> 1)) * W2 + 2 * gx + (cls & 1) : 0;
        uint4 *ysp = a.y + ((size_t)(n * CO16 + cg * 4 + q * 2) * 4 + half) * HW2 + pix;
        const float4 *rp = reinterpret_cast<const float4 *>(a.residual + ((size_t)n * HW2 + pix) * a.Cout + co0);
#pragma unroll
        for (int g8 = 0; g8 < 4; ++g8) {
            const float bb[4] = {b4[g8].x, b4[g8].y, b4[g8].z, b4[g8].w}, ii[4] = {i4[g8].x, i4[g8].y, i4[g8].z, i4[g8].w};
            float4 r4 = float4{0.f, 0.f, 0.f, 0.f};
            if (a.residual && live) r4 = rp[2 * g8];
            const float rr[4] = {r4.x, r4.y, r4.z, r4.w};
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * g8 + j;
                const float tsum = fmaf(accl[cls][e], kSp16LowInv, acc[cls][e]);
                v[j] = fmaxf(tsum * ii[j] + (0.f + bb[j]), floor_v);
                if (a.residual) v[j] = v[j] + rr[j];
            }
            vmax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fmaxf(fabsf(v[2]), fabsf(v[3])), vmax));
            unsigned h01, l01, h23, l23;
            sp16_split2(v[0], v[1], h01, l01);
            sp16_split2(v[2], v[3], h23, l23);
            swap32(h01, l01);          // lanes 0-31: h of channels 0,1 | 4,5 of the 8-channel group; lanes 32-63: l of the same channels
            swap32(h23, l23);
            if (live) *ysp = uint4{h01, h23, l01, l23};      // plane = 2 * channel half + term: lanes 32-63 hold term 1 (the `half` in ysp)
            ysp += 2 * HW2;
        }
    }
    if (a.range_flag && live && vmax > 65504.f) atomicOr(a.range_flag, 1);
}

struct BlendArgs {
    const float *__restrict__ a, *__restrict__ b, *__restrict__ wa, *__restrict__ wb;
    float *__restrict__ y;              // may be NULL
    uint4 *__restrict__ ysp;            // may be NULL
    int *range_flag;
    float bias_a, bias_b;
    int C, HW;
    long long pixels;
};

constexpr int kBlendGroups = COALIGN_SSFA_BLEND_MAX_C / 8 / 16;      // 8-channel groups a lane holds at most

// 16 lanes (one DPP row) share a pixel, a wavefront takes four: lane k of the row holds the 8-channel groups k, k + 16, ... of BOTH maps in registers between the
// logit sums and the blend -- one pass over a and b.
__global__ __launch_bounds__(256) void ssfa_blend(const BlendArgs g) {
    const long long pix = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int k = threadIdx.x & 15, C8 = g.C / 8;
    const bool live = pix < g.pixels;
    const long long pq = live ? pix : 0;                      // (dead lanes of the last wavefront read pixel 0 and store nothing: the row sums need all 16 lanes)
    float va[kBlendGroups][8], vb[kBlendGroups][8], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < kBlendGroups; ++i) {
        const int c8 = k + 16 * i;
        if (c8 < C8) {
            const float4 *pa = reinterpret_cast<const float4 *>(g.a + (size_t)pq * g.C + 8 * c8), *pb = reinterpret_cast<const float4 *>(g.b + (size_t)pq * g.C + 8 * c8);
            const float4 *pwa = reinterpret_cast<const float4 *>(g.wa + 8 * c8), *pwb = reinterpret_cast<const float4 *>(g.wb + 8 * c8);
            const float4 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1], wa0 = pwa[0], wa1 = pwa[1], wb0 = pwb[0], wb1 = pwb[1];
            const float ta[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, tb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            const float twa[8] = {wa0.x, wa0.y, wa0.z, wa0.w, wa1.x, wa1.y, wa1.z, wa1.w}, twb[8] = {wb0.x, wb0.y, wb0.z, wb0.w, wb1.x, wb1.y, wb1.z, wb1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                va[i][j] = ta[j];
                vb[i][j] = tb[j];
                sa = fmaf(twa[j], ta[j], sa);
                sb = fmaf(twb[j], tb[j], sb);
            }
        }
    }
    sa += dppf<0xB1>(sa); sb += dppf<0xB1>(sb);               // quad_perm [1, 0, 3, 2]
    sa += dppf<0x4E>(sa); sb += dppf<0x4E>(sb);               // quad_perm [2, 3, 0, 1]
    sa += dppf<0x141>(sa); sb += dppf<0x141>(sb);             // row_half_mirror
    sa += dppf<0x140>(sa); sb += dppf<0x140>(sb);             // row_mirror: every lane of the row holds the pixel's sum
    const float la = sa + g.bias_a, lb = sb + g.bias_b;
    const float pr = 1.f / (1.f + expf(lb - la)), qr = 1.f - pr;
    if (!live) return;
    const int n = (int)(pix / g.HW), r = (int)(pix - (long long)n * g.HW);
    float vmax = 0.f;
#pragma unroll
    for (int i = 0; i < kBlendGroups; ++i) {
        const int c8 = k + 16 * i;
        if (c8 < C8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = va[i][j] * pr + vb[i][j] * qr;
            if (g.y) {
                float4 *py = reinterpret_cast<float4 *>(g.y + (size_t)pix * g.C + 8 * c8);
                py[0] = float4{v[0], v[1], v[2], v[3]};
                py[1] = float4{v[4], v[5], v[6], v[7]};
            }
            if (g.ysp) {
#pragma unroll
                for (int j = 0; j < 8; ++j) vmax = fmaxf(vmax, fabsf(v[j]));
                uint4 h, l;
                sp16_split8(v, h, l);
                uint4 *dst = g.ysp + ((size_t)n * (C8 / 2) * 4 + (size_t)(c8 >> 1) * 4 + 2 * (c8 & 1)) * g.HW + r;
                dst[0] = h;
                dst[g.HW] = l;
            }
        }
    }
    if (g.ysp && g.range_flag && vmax > 65504.f) atomicOr(g.range_flag, 1);
}

bool deconv_shape_ok(int Cin, int Cout) { return Cin >= 16 && Cin % 16 == 0 && Cout >= 64 && Cout % 64 == 0 && Cout <= COALIGN_DECONV3X3_MAX_COUT; }

}  // namespace

extern "C" size_t coalign_deconv3x3_s2_weight_bytes(int Cin, int Cout) { return deconv_shape_ok(Cin, Cout) ? coalign_conv3x3_emu_weight_bytes_ex(Cin, Cout, 16, 1) : 0; }

extern "C" int coalign_deconv3x3_s2_sp(const void *x_sp, const void *w_image, const float *bias, const float *residual, void *y_sp, int N, int Cin, int Cout, int h,
                                       int w, int relu, int32_t *range_flag, void *stream) {
    if (!x_sp || !w_image || !bias || !y_sp) return COALIGN_ERR_NULL_POINTER;
    if (N < 0 || h < 1 || w < 1 || (int64_t)N * (2 * (int64_t)h) * (2 * (int64_t)w) >= (int64_t)1 << 31) return COALIGN_ERR_BAD_SHAPE;
    if (!deconv_shape_ok(Cin, Cout) || (relu != 0 && relu != 1)) return COALIGN_ERR_UNSUPPORTED;
    if (misaligned(x_sp, 15) || misaligned(w_image, 15) || misaligned(y_sp, 15) || misaligned(residual, 15) || misaligned(bias, 3) || misaligned(range_flag, 3))
        return COALIGN_ERR_NULL_POINTER;
    const int tiles_x = (w + kTW - 1) / kTW, tiles_y = (h + kTH - 1) / kTH;
    const int64_t tiles = (int64_t)N * tiles_y * tiles_x * (Cout / 64);
    if (tiles >= (int64_t)1 << 31) return COALIGN_ERR_UNSUPPORTED;
    if (N == 0) return COALIGN_OK;
    static PerDevice lds_set;
    if (const int rc = allow_dynamic_lds(lds_set, kLdsBytes, deconv3x3_s2_sp)) return rc;
    const size_t wbytes = coalign_deconv3x3_s2_weight_bytes(Cin, Cout), tail = (size_t)Cout * 8;
    const char *wb = static_cast<const char *>(w_image);
    DeconvArgs a{};
    a.x = static_cast<const uint4 *>(x_sp);
    a.wt = static_cast<const uint4 *>(w_image);
    a.zero = reinterpret_cast<const uint4 *>(wb + wbytes - tail - 16);
    a.bias = bias;
    a.winv = reinterpret_cast<const float *>(wb + wbytes - tail);
    a.residual = residual;
    a.y = static_cast<uint4 *>(y_sp);
    a.range_flag = range_flag;
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.h = h; a.w = w; a.relu = relu;
    a.tiles_x = tiles_x;
    a.tiles_y = tiles_y;
    a.groups = Cout / 64;
    hipLaunchKernelGGL(deconv3x3_s2_sp, dim3((unsigned)tiles), dim3(kThreads), kLdsBytes, static_cast<hipStream_t>(stream), a);
    return check_launch();
}

extern "C" int coalign_ssfa_blend(const float *a, const float *b, const float *wa, const float *wb, float bias_a, float bias_b, float *y_nhwc, void *y_sp, int N, int C,
                                  int H, int W, int32_t *range_flag, void *stream) {
    if (!a || !b || !wa || !wb || (!y_nhwc && !y_sp)) return COALIGN_ERR_NULL_POINTER;
    if (N < 0 || H < 1 || W < 1 || (int64_t)N * H * W >= (int64_t)1 << 31) return COALIGN_ERR_BAD_SHAPE;
    if (C < 16 || C % 16 || C > COALIGN_SSFA_BLEND_MAX_C) return COALIGN_ERR_UNSUPPORTED;
    if (misaligned(a, 15) || misaligned(b, 15) || misaligned(wa, 15) || misaligned(wb, 15) || misaligned(y_nhwc, 15) || misaligned(y_sp, 15) || misaligned(range_flag, 3))
        return COALIGN_ERR_NULL_POINTER;
    if (N == 0) return COALIGN_OK;
    BlendArgs g{};
    g.a = a; g.b = b; g.wa = wa; g.wb = wb;
    g.y = y_nhwc;
    g.ysp = static_cast<uint4 *>(y_sp);
    g.range_flag = range_flag;
    g.bias_a = bias_a; g.bias_b = bias_b;
    g.C = C; g.HW = H * W;
    g.pixels = (long long)N * H * W;
    hipLaunchKernelGGL(ssfa_blend, dim3((unsigned)((g.pixels + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), g);
    return check_launch();
}
