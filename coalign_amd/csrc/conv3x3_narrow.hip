// 3x3 / stride 1 / pad 1 convolution with a NARROW output (16 or 32 channels) that writes a SplitMap, gfx950: the encoder of NaiveCompressor
// (opencood/models/sub_modules/naive_compress.py:5-31, 64 -> 64 / r channels at canvas resolution).  Same arithmetic as conv3x3_sp.hip -- sp16 pairs
// (common.h) on v_mfma_f32_32x32x16_f16, w_h x_h into one fp32 accumulator, w_h x_l' + w_l' x_h into a second one that enters with 2^-10, the per-channel
// power-of-two weight scale undone in the epilogue -- with the SAME products in the SAME order per output value (interval by interval, tap by tap), so the two
// kernels agree bit for bit on the same weights (tests/test_compressor_gpu.py).
//
// What is different is the balance: 9 * Cin * Cout products per pixel against (Cin + Cout) * 4 bytes -- at Cout = 16 the layer is bound by bytes, not by the
// matrix pipe.  Hence ONE workgroup produces ALL output channels of its pixels (no second channel group re-reads the patch), and the weight image, 74 KB at
// most for the compressor's 64 input channels, is WEIGHT-STATIONARY: a persistent workgroup fetches it into LDS once and then streams patches.  (An image
// that does not fit -- Cin * Cout > 64 * 32 -- travels interval by interval beside the patch, double buffered, as in conv3x3_sp.hip.)
//
// Tile: 16 wavefronts, each one row of 32 pixels (16 x 32 output pixels, an 18 x 34 patch of 16-byte groups x 4 planes per 16-channel interval, double
// buffered: 74 + 2 x 40 KB of LDS, one workgroup per CU, four wavefronts per SIMD).  Measured against 8 wavefronts / 8 x 32 tiles on 5 x 64 x 200 x 704 -> 16:
// channels-last input 10-12 % faster box for box, SplitMap input equal (more bytes in flight per CU, 12 % instead of 25 % halo rows).
// A wavefront owns ONE 32 x 32 accumulator tile x two accumulators; Cout = 16 fills rows 0-15 of the matrix instruction and lets rows 16-31
// repeat them (never stored): half the pipe is spent on nothing, which a byte-bound layer can afford, and the 32x32x16 instruction keeps the summation order
// of the other SplitMap kernels.
//
// Input kinds: 0 = SplitMap (the patch travels global -> LDS by LDS-DMA, no VALU work in the K loop); 1 = channels-last float32 [N, H, W, Cin] (the dense
// canvas): the loader fetches 8 channels of a pixel per lane into registers one interval ahead and splits them (sp16_split2: the pairs coalign_sp_pack would
// have stored, bit for bit) into the other patch buffer behind the interval's matrix steps -- the 360 MB pack pass over the canvas never runs;
// 2 = the SPARSE CANVAS of pillar_sparse.hip (coalign_conv3x3_sp_narrow_sparse, include/coalign_amd_narrow_sparse.h): sp16 feature ROWS [M][Cin / 16][4 planes]
// [8 x fp16] (coalign_sp_pack_rows) + the 8-byte cell stamps: pixel (n, y, x) = row (stamp & 0xffffffff) if stamp >> 32 == *tag, tag != 0 and row < M_rows,
// else the zero group -- conv3x3_sp_s2.hip's rule.  The loader is kind 0's with another source address per lane (one 32-bit row offset or -1): the K loop,
// the LDS layout and the products are the same.  A tile's stamps (one per lane of the ten loading wavefronts) are fetched one interval before the tile's first
// DMA instruction is issued, which takes two intervals per tile: the entry point refuses Cin < 32 (COALIGN_ERR_UNSUPPORTED), as _s2_sparse does.
//
// Weight image (coalign_conv3x3_narrow_weight_bytes): [Cin / 16][9 taps][2 terms][2 channel halves][Cout][8 cin] fp16 + 16 zero bytes + [Cout] float32 2^-k_c
// + [Cout] float32 2^k_c: the (9b) order with a Cout-wide block in place of 64, i.e. exactly its LDS order -- the weight DMA is a linear copy.
#include "common.h"
#include "coalign_amd_narrow.h"
#include "coalign_amd_narrow_sparse.h"

namespace {

using namespace coalign;
typedef __attribute__((address_space(3))) void *lptr_t;

constexpr int kWaves = 16, kThreads = 64 * kWaves;
constexpr int kTH = kWaves, kTW = 32;                                // output tile: a row per wavefront
constexpr int kPH = kTH + 2, kPW = kTW + 2;                          // patch
constexpr int kPix = kPH * kPW, kPixP = (kPix + 63) / 64 * 64;       // groups per plane, padded to whole DMA instructions (612 -> 640)
constexpr int kPIns = kPixP / 64;                                    // DMA instructions per plane
constexpr int kBBytes = 4 * kPixP * 16;                              // one patch buffer: 4 planes
constexpr int kWAreaBytes = 4 * 9 * 2 * 2 * 32 * 16;                 // weight area: the whole image of Cin * Cout <= 64 * 32 (73728 bytes)
constexpr int kItems = (2 * kPix + kThreads - 1) / kThreads;         // input kind 1: (pixel, channel half) items per thread and interval
constexpr size_t kLdsBytes = (size_t)kWAreaBytes + 2 * kBBytes + 2 * 32 * sizeof(float);
static_assert(kPIns <= kWaves, "one patch piece per wavefront");
static_assert(kLdsBytes <= 160 * 1024, "does not fit the 160 KB LDS");

struct NarrowArgs {
    const void *__restrict__ x;         // SplitMap, channels-last float32, or sp16 rows
    const unsigned long long *__restrict__ stamps;      // kind 2 only
    const int *__restrict__ tag_ptr;
    unsigned sparse_rows;
    const uint4 *__restrict__ wt;       // weight image
    const uint4 *__restrict__ zero;     // its 16 zero bytes
    const float *__restrict__ bias, *__restrict__ wscale;      // wscale: [Cout] 2^-k_c
    uint4 *__restrict__ y;              // SplitMap [N, Cout, H, W]
    int *range_flag;                    // may be NULL
    int N, Cin, H, W, relu, tiles_x, tiles_y, total_tiles, stationary;
};

struct Tile {
    int n, y0, x0;
};

template <int CT, int KIND>
__global__ __launch_bounds__(kThreads, kWaves / 4) void conv3x3_narrow_kernel(const NarrowArgs a) {
    static_assert(CT == 16 || CT == 32, "output channels");
    constexpr int NG8 = CT / 8;                                        // 8-channel groups
    constexpr int WQ = 9 * 2 * 2 * CT, W_BYTES = WQ * 16, WINS = WQ / 64;      // one interval's weights: 16-byte groups, bytes, DMA instructions
    constexpr int WJ = (WINS + kWaves - 1) / kWaves;
    static_assert(WQ % 64 == 0 && 2 * W_BYTES <= kWAreaBytes, "weight pieces");
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, half = lane >> 5, p = lane & 31;
    const int HW = a.H * a.W, chunks = a.Cin / 16;
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)lds;
    constexpr unsigned kPatch0 = kWAreaBytes;
    float *lds_par = reinterpret_cast<float *>(lds + kWAreaBytes + 2 * kBBytes);      // bias | 2^-k_c (the first interval's wait + barrier orders these stores before any epilogue)
    if (tid < CT) {
        lds_par[tid] = a.bias[tid];
        lds_par[CT + tid] = a.wscale[tid];
    }
    int boff[9];                                                       // group of this lane's pixel under tap s, inside plane (2 * half + term 0)
#pragma unroll
    for (int s = 0; s < 9; ++s) boff[s] = 2 * half * kPixP + (wave + s / 3) * kPW + p + s % 3;
    const int wlane = half * CT + (p & (CT - 1));                      // this lane's group inside one (tap, term) weight block (CT = 16: rows 16-31 repeat rows 0-15)

    auto decode = [&](int t) {
        Tile c;
        const int tx = t % a.tiles_x, r = t / a.tiles_x, ty = r % a.tiles_y;
        c.n = r / a.tiles_y;
        c.y0 = ty * kTH;
        c.x0 = tx * kTW;
        return c;
    };
    // patch group i = row * kPW + column <-> image pixel (y0 - 1 + row, x0 - 1 + column); outside the image: zero
    auto pixel_of = [&](const Tile &t, int i, int &gy, int &gx) {
        const int y = i / kPW, xq = i - y * kPW;
        gy = t.y0 - 1 + y;
        gx = t.x0 - 1 + xq;
        return i < kPix && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    };
    // ---- input kind 0: the wavefront's DMA piece of every plane (wavefronts 0 .. kPIns - 1), as an offset in 16-byte groups inside plane 0 of interval 0
    auto make_plan = [&](const Tile &t) {
        int gy, gx;
        const bool ok = pixel_of(t, wave * 64 + lane, gy, gx);
        return ok ? t.n * chunks * 4 * HW + gy * a.W + gx : -1;
    };
    // ---- input kind 2: the lane's stamp of a tile (cells outside the image read stamp 0: tag 0 is never current) -> the offset of its row, in 16-byte groups
    const unsigned tag = KIND == 2 ? (unsigned)*a.tag_ptr : 0u;
    auto load_stamp = [&](const Tile &t) {
        int gy, gx;
        unsigned long long s = 0ull;
        if (wave < kPIns && pixel_of(t, wave * 64 + lane, gy, gx)) s = a.stamps[((size_t)t.n * a.H + gy) * a.W + gx];
        return s;
    };
    auto make_plan_sparse = [&](unsigned long long s) {
        const unsigned row = (unsigned)s;
        const bool ok = (unsigned)(s >> 32) == tag && tag != 0u && row < a.sparse_rows;
        return ok ? (int)(row * (unsigned)(chunks * 4)) : -1;
    };
    auto issue_patch = [&](int off, int c, int slot) {
        if (wave < kPIns) {
            const uint4 *xs = static_cast<const uint4 *>(a.x);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 *src = off < 0 ? a.zero : KIND == 2 ? xs + (size_t)off + (c * 4 + q) : xs + (size_t)off + ((size_t)c * 4 + q) * HW;
                lds_dma16(src, lds0 + kPatch0 + slot * kBBytes + (q * kPixP + wave * 64) * 16);
            }
        }
    };
    auto issue_weights = [&](int c, int slot) {
#pragma unroll
        for (int k = 0; k < WJ; ++k) {
            const int ins = (kWaves - 1 - wave) + kWaves * k;          // (the wavefronts without a patch piece first)
            if (ins < WINS) lds_dma16(a.wt + (size_t)c * WQ + ins * 64 + lane, lds0 + slot * W_BYTES + ins * 1024);
        }
    };
    // ---- input kind 1: (pixel, channel half) items of this thread: 8 floats each, fetched one interval ahead, split into the other patch buffer
    struct Stage {
        long long off[kItems];                                         // float offset of the item's first channel in interval 0, or -1
        float4 v[kItems][2];
    };
    auto make_stage_plan = [&](const Tile &t, Stage &st) {
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int it = tid + kThreads * j, i = it >> 1, hh = it & 1;
            int gy, gx;
            const bool ok = pixel_of(t, i, gy, gx);
            st.off[j] = ok ? ((long long)t.n * HW + (long long)gy * a.W + gx) * a.Cin + 8 * hh : -1;
        }
    };
    auto stage_load = [&](Stage &st, int c) {
        const float *xf = static_cast<const float *>(a.x);
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            if (st.off[j] >= 0) {
                const float4 *q = reinterpret_cast<const float4 *>(xf + st.off[j] + 16 * c);
                st.v[j][0] = q[0];
                st.v[j][1] = q[1];
            } else {
                st.v[j][0] = st.v[j][1] = float4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    auto stage_store = [&](const Stage &st, int slot) {
        uint4 *pb = reinterpret_cast<uint4 *>(lds + kPatch0 + slot * kBBytes);
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int it = tid + kThreads * j, i = it >> 1, hh = it & 1;
            if (it < 2 * kPix) {
                unsigned h[4], l[4];
                coalign::sp16_split2(st.v[j][0].x, st.v[j][0].y, h[0], l[0]);
                coalign::sp16_split2(st.v[j][0].z, st.v[j][0].w, h[1], l[1]);
                coalign::sp16_split2(st.v[j][1].x, st.v[j][1].y, h[2], l[2]);
                coalign::sp16_split2(st.v[j][1].z, st.v[j][1].w, h[3], l[3]);
                pb[(2 * hh) * kPixP + i] = uint4{h[0], h[1], h[2], h[3]};
                pb[(2 * hh + 1) * kPixP + i] = uint4{l[0], l[1], l[2], l[3]};
            }
        }
    };

    // persistent workgroups over whole tiles g, g + n, ...; XCD k takes the k-th eighth of the logical ids (neighbouring tiles share halo rows in its L2)
    const int n_wg = gridDim.x;
    int g = blockIdx.x;
    {
        const int q = n_wg >> 3, r = n_wg & 7, k = g & 7, j = g >> 3;
        g = k * q + (k < r ? k : r) + j;
    }
    int tile = g;
    if (tile >= a.total_tiles) return;
    const int n_local = ((a.total_tiles - g + n_wg - 1) / n_wg) * chunks;
    Tile cur = decode(tile);
    int plan = 0;
    Stage st;
    if (a.stationary) {
        for (int c = 0; c < chunks; ++c) issue_weights(c, c);
    } else {
        issue_weights(0, 0);
    }
    if constexpr (KIND == 0) {
        plan = make_plan(cur);
        issue_patch(plan, 0, 0);
    } else if constexpr (KIND == 2) {
        plan = make_plan_sparse(load_stamp(cur));
        issue_patch(plan, 0, 0);
    } else {
        make_stage_plan(cur, st);
        stage_load(st, 0);
        stage_store(st, 0);
    }
    if (wave >= kWaves / 2) __builtin_amdgcn_s_setprio(1);             // (as conv3x3_sp.hip: the later-dispatched half of the wavefronts loses every arbitration otherwise)
    int L = 0;
    while (L < n_local) {
        const int gy = cur.y0 + wave, gx = cur.x0 + p;
        const bool live = gy < a.H && gx < a.W;
        const bool wave_live = gy < a.H;                               // (wave-uniform: gy depends on the wavefront only)
        const size_t pix = live ? (size_t)gy * a.W + gx : 0;
        floatx16 acc = floatx16{0}, accl = floatx16{0};
        Tile next = cur;
        int ntile = tile;
        unsigned long long nstamp = 0ull;
        for (int chunk = 0; chunk < chunks; ++chunk, ++L) {
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            const bool more = L + 1 < n_local;
            int nc = chunk + 1;
            if constexpr (KIND == 2) {                                 // the next tile's stamps: one interval ahead of its first DMA (chunks >= 2)
                if (chunk == chunks - 2 && L + 2 < n_local) {
                    ntile = tile + n_wg;
                    next = decode(ntile);
                    nstamp = load_stamp(next);
                }
            }
            if (more && nc == chunks) {                                // the next interval opens this workgroup's next tile
                nc = 0;
                if constexpr (KIND == 2) {
                    plan = make_plan_sparse(nstamp);
                } else {
                    ntile = tile + n_wg;
                    next = decode(ntile);
                    if constexpr (KIND == 0) plan = make_plan(next);
                    else make_stage_plan(next, st);
                }
            }
            const int slot_cur = L & 1, slot_next = (L + 1) & 1;
            if (more) {
                if (!a.stationary) issue_weights(nc, slot_next);
                if constexpr (KIND != 1) issue_patch(plan, nc, slot_next);
                else stage_load(st, nc);
            }
            if (wave_live) {
                const uint4 *bq = reinterpret_cast<const uint4 *>(lds + kPatch0 + slot_cur * kBBytes);
                const uint4 *wq = reinterpret_cast<const uint4 *>(lds + (a.stationary ? chunk : slot_cur) * W_BYTES) + wlane;
                halfx8 bc[2], wc[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    bc[t] = __builtin_bit_cast(halfx8, bq[t * kPixP + boff[0]]);
                    wc[t] = __builtin_bit_cast(halfx8, wq[t * 2 * CT]);
                }
#pragma unroll
                for (int s = 0; s < 9; ++s) {
                    halfx8 bn[2], wn[2];
                    if (s + 1 < 9) {                                   // operands of the next tap are in flight while this tap's matrix instructions issue
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            bn[t] = __builtin_bit_cast(halfx8, bq[t * kPixP + boff[s + 1]]);
                            wn[t] = __builtin_bit_cast(halfx8, wq[(((s + 1) * 2 + t) * 2) * CT]);
                        }
                    }
                    accl = __builtin_amdgcn_mfma_f32_32x32x16_f16(wc[0], bc[1], accl, 0, 0, 0);      // w_h x_l'
                    accl = __builtin_amdgcn_mfma_f32_32x32x16_f16(wc[1], bc[0], accl, 0, 0, 0);      // w_l' x_h
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wc[0], bc[0], acc, 0, 0, 0);        // w_h x_h
                    if (s + 1 < 9) {
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            bc[t] = bn[t];
                            wc[t] = wn[t];
                        }
                    }
                }
            }
            if constexpr (KIND == 1) {
                if (more) stage_store(st, slot_next);                  // (that buffer was last read in the previous interval: every wavefront has passed this interval's barrier)
            }
        }
        // ---- epilogue, as conv3x3_sp.hip's: y = (acc + 2^-10 accl) * 2^-k_c + bias, ReLU, stored as SplitMap pairs
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = fmaf(accl[e], coalign::kSp16LowInv, acc[e]);
        const float floor_v = a.relu ? 0.f : -__builtin_inff();
        float vmax = 0.f;
        uint4 *ysp = a.y + ((size_t)(cur.n * (CT / 16)) * 4 + half) * HW + pix;
        const size_t sp_step = 2 * (size_t)HW;
#pragma unroll
        for (int g8 = 0; g8 < NG8; ++g8) {                             // groups of 4 consecutive channels per lane: channel = 8 g8 + 4 half + j
            const float4 b4 = reinterpret_cast<const float4 *>(lds_par + 4 * half)[2 * g8], i4 = reinterpret_cast<const float4 *>(lds_par + CT + 4 * half)[2 * g8];
            const float bb[4] = {b4.x, b4.y, b4.z, b4.w}, ii[4] = {i4.x, i4.y, i4.z, i4.w};
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(acc[4 * g8 + j] * ii[j] + (0.f + bb[j]), floor_v);      // (the operations of conv3x3_sp.hip without a residual, in its order)
            vmax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fmaxf(fabsf(v[2]), fabsf(v[3])), vmax));
            unsigned h01, l01, h23, l23;
            coalign::sp16_split2(v[0], v[1], h01, l01);
            coalign::sp16_split2(v[2], v[3], h23, l23);
            swap32(h01, l01);          // lanes 0-31: h of channels 0,1 | 4,5 of the 8-channel group; lanes 32-63: l of the same channels
            swap32(h23, l23);
            if (live && wave_live) *ysp = uint4{h01, h23, l01, l23};   // plane = 2 * channel half + term: lanes 32-63 hold term 1 (the `half` in ysp)
            ysp += sp_step;
        }
        if (a.range_flag && live && wave_live && vmax > 65504.f) atomicOr(a.range_flag, 1);
        cur = next;
        tile = ntile;
    }
}

int narrow_check(int N, int Cin, int Cout, int H, int W) {
    if (N < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return COALIGN_ERR_BAD_SHAPE;
    if (Cin % 16 || (Cout != 16 && Cout != 32)) return COALIGN_ERR_UNSUPPORTED;
    if ((int64_t)N * (Cin > Cout ? Cin : Cout) * H * W > (int64_t)1 << 32) return COALIGN_ERR_UNSUPPORTED;      // group offsets are 32-bit
    return COALIGN_OK;
}

template <int CT, int KIND>
int launch_narrow(NarrowArgs a, hipStream_t s) {
    auto k = conv3x3_narrow_kernel<CT, KIND>;
    static PerDevice lds_set;
    if (const int rc = allow_dynamic_lds(lds_set, kLdsBytes, k)) return rc;
    const int cus = cu_count();
    a.tiles_x = (a.W + kTW - 1) / kTW;
    a.tiles_y = (a.H + kTH - 1) / kTH;
    a.total_tiles = a.N * a.tiles_y * a.tiles_x;
    a.stationary = (size_t)(a.Cin / 16) * (9 * 2 * 2 * CT * 16) <= (size_t)kWAreaBytes ? 1 : 0;
    const int grid = a.total_tiles < cus ? a.total_tiles : cus;      // 152 KB of LDS: one workgroup per CU
    hipLaunchKernelGGL(k, dim3(grid), dim3(kThreads), kLdsBytes, s, a);
    return coalign::check_launch();
}

}  // namespace

extern "C" size_t coalign_conv3x3_narrow_weight_bytes(int Cin, int Cout) {
    if (Cin < 1 || Cin % 16 || (Cout != 16 && Cout != 32)) return 0;
    return (size_t)Cin * Cout * 9 * 2 * 2 + 16 + (size_t)Cout * 8;
}

extern "C" int coalign_conv3x3_sp_narrow(const void *x, int in_kind, const void *w_narrow, const float *bias, void *y_sp, int N, int Cin, int Cout, int H, int W,
                                         int relu, int32_t *range_flag, void *stream) {
    if (!x || !w_narrow || !bias || !y_sp) return COALIGN_ERR_NULL_POINTER;
    int rc = narrow_check(N, Cin, Cout, H, W);
    if (rc != COALIGN_OK) return rc;
    if (in_kind != COALIGN_NARROW_IN_SP && in_kind != COALIGN_NARROW_IN_NHWC) return COALIGN_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_narrow) | reinterpret_cast<uintptr_t>(y_sp)) & 15) return COALIGN_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(bias) & 3) return COALIGN_ERR_UNSUPPORTED;
    if (N == 0) return COALIGN_OK;
    const size_t wbytes = coalign_conv3x3_narrow_weight_bytes(Cin, Cout), tail = (size_t)Cout * 8;
    const char *wb = static_cast<const char *>(w_narrow);
    NarrowArgs a{};
    a.x = x;
    a.wt = static_cast<const uint4 *>(w_narrow);
    a.zero = reinterpret_cast<const uint4 *>(wb + wbytes - tail - 16);
    a.bias = bias;
    a.wscale = reinterpret_cast<const float *>(wb + wbytes - tail);
    a.y = static_cast<uint4 *>(y_sp);
    a.range_flag = range_flag;
    a.N = N; a.Cin = Cin; a.H = H; a.W = W; a.relu = relu;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Cout == 16) return in_kind == COALIGN_NARROW_IN_SP ? launch_narrow<16, 0>(a, s) : launch_narrow<16, 1>(a, s);
    return in_kind == COALIGN_NARROW_IN_SP ? launch_narrow<32, 0>(a, s) : launch_narrow<32, 1>(a, s);
}

extern "C" int coalign_conv3x3_sp_narrow_sparse(const void *rows_sp, int M_rows, const void *stamps, const int32_t *state, const void *w_narrow, const float *bias, void *y_sp,
                                                int N, int Cin, int Cout, int H, int W, int relu, int32_t *range_flag, void *stream) {
    if (!rows_sp || !stamps || !state || !w_narrow || !bias || !y_sp) return COALIGN_ERR_NULL_POINTER;
    if (M_rows < 0) return COALIGN_ERR_BAD_SHAPE;
    int rc = narrow_check(N, Cin, Cout, H, W);
    if (rc != COALIGN_OK) return rc;
    if (Cin < 32) return COALIGN_ERR_UNSUPPORTED;                     // (a tile's stamps are fetched one interval ahead: at least two intervals per tile)
    if ((reinterpret_cast<uintptr_t>(rows_sp) | reinterpret_cast<uintptr_t>(w_narrow) | reinterpret_cast<uintptr_t>(y_sp)) & 15) return COALIGN_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(bias) & 3) return COALIGN_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(stamps) & 7) || (reinterpret_cast<uintptr_t>(state) & 3)) return COALIGN_ERR_UNSUPPORTED;
    if ((int64_t)M_rows * Cin / 4 >= (int64_t)1 << 31) return COALIGN_ERR_UNSUPPORTED;      // row offsets are 32-bit
    if (N == 0) return COALIGN_OK;
    const size_t wbytes = coalign_conv3x3_narrow_weight_bytes(Cin, Cout), tail = (size_t)Cout * 8;
    const char *wb = static_cast<const char *>(w_narrow);
    NarrowArgs a{};
    a.x = rows_sp;
    a.stamps = static_cast<const unsigned long long *>(stamps);
    a.tag_ptr = state;
    a.sparse_rows = (unsigned)M_rows;
    a.wt = static_cast<const uint4 *>(w_narrow);
    a.zero = reinterpret_cast<const uint4 *>(wb + wbytes - tail - 16);
    a.bias = bias;
    a.wscale = reinterpret_cast<const float *>(wb + wbytes - tail);
    a.y = static_cast<uint4 *>(y_sp);
    a.range_flag = range_flag;
    a.N = N; a.Cin = Cin; a.H = H; a.W = W; a.relu = relu;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return Cout == 16 ? launch_narrow<16, 2>(a, s) : launch_narrow<32, 2>(a, s);
}
