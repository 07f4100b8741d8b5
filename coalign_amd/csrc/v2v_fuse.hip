// The glue of V2VNet's message passing between its 3 x 3 convolutions, on CHANNELS-LAST maps and SplitMaps, gfx950.
//
// Reference semantics: V2VNetFusion.forward, fuse_modules/fusion_in_one.py:197-293, with ConvGRUCell.forward, sub_modules/convgru.py:48-70.  Per iteration and
// receiver i the reference warps every sender's map (warp_affine_simple), concatenates it with the receiver's, convolves (msg_cnn), multiplies by the warp of a map
// of ones, takes the max / mean over the senders, concatenates with the receiver's map and runs a ConvGRU with a zero hidden state.  The convolutions run on
// coalign_conv3x3_sp (csrc/conv3x3_sp.hip); what lies between them is three memory-bound kernels here, each one pass over its operands:
//   v2v_warp_split   x -> the SplitMap of every (receiver, sender) warp: the taps and the blend of warp_taps.h (the warp of warp_fuse_nhwc.hip bit for bit) and the
//                    sp16 split of coalign_sp_pack in registers; the float32 warped maps never reach memory
//   v2v_aggregate    (a_ij + e_i) * mask_ij, max / mean over j, and the GRU's input [x_i | agg_i] as a SplitMap (or x_i + agg_i as float32 without the GRU).  The
//                    mask is the sum of the four masked tap weights, computed per lane from theta: it is read from nowhere
//   v2v_gate         sigmoid(y[:Ch]) * tanh(y[Ch:]) -> float32 (the next node features) or a SplitMap (a second GRU layer's input)
// One lane mapping for all three: a wavefront owns 16 consecutive pixels of one map; lane = (pixel = lane & 15, channel group = lane >> 4) and walks the 8-channel
// groups g, g + 4, ...  The 4 lanes of a pixel read 4 x 32 B = one 128-byte line of a channels-last row (2 x 16 B per lane), the 16 lanes of a group write
// 16 x 16 B = 256 contiguous bytes of a SplitMap plane.  No LDS, no barriers, no workspace, the caller's stream: capturable.
#include "common.h"
#include "warp_taps.h"
#include "v2v_lanes.h"

#include "coalign_amd_v2v.h"

namespace {

using coalign::misaligned;

struct WarpArgs {
    const float *x;          // [n, H, W, C]
    const double *theta;     // [R, n, 2, 3]
    uint4 *y;                // SplitMap [R n, C, H, W]
    int *range_flag;
    int n, R, C, H, W;
};

struct AggArgs {
    const float *a, *e, *x;  // [R n, H, W, C], [R, H, W, C], [>= R, H, W, C]
    const double *theta;
    void *out;               // SplitMap [R, 2C, H, W] or float [R, H, W, C]
    int *range_flag;
    int n, R, C, H, W, agg, out_kind;
};

struct GateArgs {
    const float *y;          // [R, H, W, 2 Ch]
    void *out;               // float [R, H, W, Ch] or SplitMap [R, Ch, H, W]
    int *range_flag;
    int R, Ch, H, W, out_kind;
};

__global__ __launch_bounds__(256) void v2v_warp_split_kernel(const WarpArgs a) {
    const int HW = a.H * a.W, G = a.C / 8;
    Place p;
    if (!place(a.R * a.n, HW, p)) return;
    const int oy = p.pix / a.W;
    const Geom geo{a.C, a.H, a.W, a.H, a.W};
    const Taps t = make_taps(geo, a.theta, p.map, p.pix - oy * a.W, oy);      // theta row (i, j) = map i n + j
    const float *xa = a.x + (size_t)(p.map % a.n) * HW * a.C;
    bool big = false;
    for (int g = p.g0; g < G; g += GL) {
        float4 v[8];
        float X[8];
        issue(t, xa + g * 8, 1, v);
        blend(t, v, X);
        big = store_split8(a.y, p.map, a.C / 16, g, HW, p.pix, X, p.live) || big;
    }
    if (a.range_flag && big) atomicOr(a.range_flag, 1);
}

__global__ __launch_bounds__(256) void v2v_aggregate_kernel(const AggArgs a) {
    const int HW = a.H * a.W, C = a.C, G = C / 8;
    Place p;
    if (!place(a.R, HW, p)) return;
    const int i = p.map, oy = p.pix / a.W, ox = p.pix - oy * a.W;
    const Geom geo{C, a.H, a.W, a.H, a.W};
    float mask[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mask[j] = 0.f;
        if (j < a.n) {
            const Taps t = make_taps(geo, a.theta, i * a.n + j, ox, oy);
            mask[j] = t.w00 + t.w01 + t.w10 + t.w11;      // the blend of a map of ones, left to right
        }
    }
    const float fn = (float)a.n;
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
                    m[k] = (m[k] + e[k]) * mask[j];
                    acc[k] = j == 0 ? m[k] : a.agg == COALIGN_V2V_AGG_MAX ? fmaxf(acc[k], m[k]) : acc[k] + m[k];
                }
            }
        if (a.agg == COALIGN_V2V_AGG_AVG) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = acc[k] / fn;
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

__global__ __launch_bounds__(256) void v2v_gate_kernel(const GateArgs a) {
    const int HW = a.H * a.W, Ch = a.Ch, G = Ch / 8;
    Place p;
    if (!place(a.R, HW, p)) return;
    const float *yp = a.y + ((size_t)p.map * HW + p.pix) * 2 * Ch;
    bool big = false;
    for (int g = p.g0; g < G; g += GL) {
        float b[8], c[8], o[8];
        load8(yp + g * 8, b);
        load8(yp + Ch + g * 8, c);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (1.0f / (1.0f + expf(-b[k]))) * tanhf(c[k]);
        if (a.out_kind == COALIGN_V2V_OUT_SP) big = store_split8(static_cast<uint4 *>(a.out), p.map, Ch / 16, g, HW, p.pix, o, p.live) || big;
        else if (p.live) store8(static_cast<float *>(a.out) + ((size_t)p.map * HW + p.pix) * Ch + g * 8, o);
    }
    if (a.range_flag && big) atomicOr(a.range_flag, 1);
}

// the checks the three entry points share; COALIGN_OK + *empty when there is nothing to do
int check_counts(int n, int R, int C, int H, int W, long long maps, bool *empty) {
    *empty = false;
    if (n < 0 || R < 0 || C < 1 || H < 1 || W < 1) return COALIGN_ERR_BAD_SHAPE;
    if (n > 8 || C % 16) return COALIGN_ERR_UNSUPPORTED;
    if (R > n) return COALIGN_ERR_BAD_SHAPE;
    if (n == 0 || R == 0) {
        *empty = true;
        return COALIGN_OK;
    }
    if ((long long)C * H * W * maps > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    return COALIGN_OK;
}

}  // namespace

extern "C" int coalign_v2v_warp_split(const float *x, int n, int R, int C, int H, int W, const double *theta, void *y_sp, int32_t *range_flag, void *stream) {
    bool empty;
    const int rc = check_counts(n, R, C, H, W, (long long)R * n, &empty);
    if (rc != COALIGN_OK || empty) return rc;
    if (!x || !theta || !y_sp) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(x, 15) || misaligned(y_sp, 15) || (reinterpret_cast<uintptr_t>(theta) & 7) || (reinterpret_cast<uintptr_t>(range_flag) & 3)) return COALIGN_ERR_UNSUPPORTED;
    WarpArgs a;
    a.x = x; a.theta = theta; a.y = static_cast<uint4 *>(y_sp); a.range_flag = range_flag;
    a.n = n; a.R = R; a.C = C; a.H = H; a.W = W;
    hipLaunchKernelGGL(v2v_warp_split_kernel, dim3(blocks_of(R * n, H, W)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}

extern "C" int coalign_v2v_aggregate(const float *a_, const float *e, const float *x, int n, int R, int C, int H, int W, const double *theta, int agg, int out_kind,
                                     void *out, int32_t *range_flag, void *stream) {
    bool empty;
    const int rc = check_counts(n, R, C, H, W, (long long)R * n, &empty);
    if (rc != COALIGN_OK) return rc;
    if ((agg != COALIGN_V2V_AGG_MAX && agg != COALIGN_V2V_AGG_AVG) || (out_kind != COALIGN_V2V_OUT_NHWC && out_kind != COALIGN_V2V_OUT_SP)) return COALIGN_ERR_UNSUPPORTED;
    if (empty) return COALIGN_OK;
    if (!a_ || !e || !x || !theta || !out) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(a_, 15) || misaligned(e, 15) || misaligned(x, 15) || misaligned(out, 15) || (reinterpret_cast<uintptr_t>(theta) & 7) || (reinterpret_cast<uintptr_t>(range_flag) & 3))
        return COALIGN_ERR_UNSUPPORTED;
    AggArgs a;
    a.a = a_; a.e = e; a.x = x; a.theta = theta; a.out = out; a.range_flag = out_kind == COALIGN_V2V_OUT_SP ? range_flag : nullptr;
    a.n = n; a.R = R; a.C = C; a.H = H; a.W = W; a.agg = agg; a.out_kind = out_kind;
    hipLaunchKernelGGL(v2v_aggregate_kernel, dim3(blocks_of(R, H, W)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}

extern "C" int coalign_v2v_gate(const float *y, int R, int Ch, int H, int W, int out_kind, void *out, int32_t *range_flag, void *stream) {
    if (R < 0 || Ch < 1 || H < 1 || W < 1) return COALIGN_ERR_BAD_SHAPE;
    if (Ch % 16 || (out_kind != COALIGN_V2V_OUT_NHWC && out_kind != COALIGN_V2V_OUT_SP)) return COALIGN_ERR_UNSUPPORTED;
    if (R == 0) return COALIGN_OK;
    if ((long long)2 * Ch * H * W * R > (long long)INT32_MAX) return COALIGN_ERR_BAD_SHAPE;
    if (!y || !out) return COALIGN_ERR_NULL_POINTER;
    if (misaligned(y, 15) || misaligned(out, 15) || (reinterpret_cast<uintptr_t>(range_flag) & 3)) return COALIGN_ERR_UNSUPPORTED;
    GateArgs a;
    a.y = y; a.out = out; a.range_flag = out_kind == COALIGN_V2V_OUT_SP ? range_flag : nullptr;
    a.R = R; a.Ch = Ch; a.H = H; a.W = W; a.out_kind = out_kind;
    hipLaunchKernelGGL(v2v_gate_kernel, dim3(blocks_of(R, H, W)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return coalign::check_launch();
}
