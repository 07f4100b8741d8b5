// Online pose correction (include/coalign_amd_align.h), gfx950: the three small kernels around coalign_pose_graph_optimize that keep CoAlign's box
// alignment on the device -- stage-1 gather, pose-graph construction, corrected pairwise / affine matrices.
//
// Reference semantics: box_alignment_relative_sample_np (opencood/models/sub_modules/box_align_v2.py:150-372) as coalign_amd/box_align.py:build_pose_graph
// restates it line by line; the comments below name the lines of that restatement.  Everything is float32 / float64 scalar arithmetic on four wavefronts per
// sample.  The clustering is serial by nature (a seed takes its still unassigned neighbours, in index order), so ONE workgroup per sample walks the seeds and
// recomputes a seed's row of the distance test when it needs it: K is a few hundred, K x K never exists.  Per seed that is taken: one row pass, one block
// scan that orders the members, the yaw variance; a member's edge only gets its SLOT there (seed rank + position, no scan unless drop_unsure_edge has to look
// at certainties first).  What an edge holds -- float64 atan2 / exp on corners read from memory -- is computed for all boxes in parallel after the walk, so
// the serial part touches LDS only.
//
// FLOAT32 ORDER.  The all-pair test sqrt(sq_i + sq_j - 2 dot_ij) < thres cancels ~1e3-sized squares in float32: two detections of one object a centimetre
// apart land within rounding of zero, and whether the radicand is a tiny positive or a tiny negative number (NaN: "not near") depends on the summation order
// (coalign_amd/box_align.py:108-111).  The order is FIXED here in the source, (x*x + y*y) + z*z for the squares and the dots, and the file relies on the
// -ffp-contract=off that build.FLAGS carries: this is the one place of the chain where a fused multiply-add changes WHICH boxes cluster, not a last bit.
#include "common.h"
#include "coalign_amd_align.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxAgents = COALIGN_ALIGN_MAX_AGENTS;
constexpr int kMaxLandmarks = COALIGN_ALIGN_MAX_LANDMARKS;
constexpr int kStoreBoxes = COALIGN_ALIGN_STORE_BOXES;
constexpr int kMaxBoxes = kMaxAgents * kStoreBoxes;           // 2048
constexpr int kPerThread = kMaxBoxes / kThreads;              // 8 consecutive boxes per thread in the member pass
constexpr int kMaxVertices = COALIGN_ALIGN_MAX_VERTICES;
constexpr int kMaxEdges = COALIGN_ALIGN_MAX_EDGES;
constexpr int kMaxCav = 16;
constexpr double kPi = 3.14159265358979323846;
constexpr double kAnchorDiagSq = 1.6 * 1.6 + 3.9 * 3.9;       // box_align_v2.py:187-189, hard-coded anchor width / length
static_assert(kPerThread == 8, "the member pass packs one thread's flags into a byte");

// ------------------------------------------------------------------------------------------------------------------------------ (11a) stage-1 gather
struct GatherArgs {
    const int32_t *keep, *keep_count, *cand_index;
    const float *cand_corners, *unc;
    int capacity, A, udim, HW, slot;
    float *corners, *unc_out;
    int32_t *count, *status;
};

__global__ __launch_bounds__(kThreads) void stage1_gather_kernel(const GatherArgs g) {
    const int e = blockIdx.x * kThreads + threadIdx.x;         // grid: kStoreBoxes * 24 elements
    const int kept = g.keep_count[0];
    const int n = kept < 0 ? 0 : (kept > kStoreBoxes ? kStoreBoxes : kept);
    float *corners = g.corners + (size_t)g.slot * kStoreBoxes * 24;
    const int k = e / 24;
    if (k < n) {
        const int src = g.keep[k];
        corners[e] = (src >= 0 && src < g.capacity) ? g.cand_corners[(size_t)src * 24 + e % 24] : 0.f;
    }
    if (g.udim > 0 && e < n * g.udim) {                       // unc_preds.permute(0, 2, 3, 1).view(-1, udim)[mask], postprocess.py:273-275
        const int ku = e / g.udim, d = e % g.udim;
        const int src = g.keep[ku];
        float v = 0.f;
        if (src >= 0 && src < g.capacity) {
            const int flat = g.cand_index[src];                // (h, w, anchor) order
            if (flat >= 0 && flat < g.A * g.HW) v = g.unc[(size_t)((flat % g.A) * g.udim + d) * g.HW + flat / g.A];
        }
        g.unc_out[(size_t)g.slot * kStoreBoxes * g.udim + e] = v;
    }
    if (e == 0) {
        g.count[g.slot] = n;
        const int over = kept > kStoreBoxes ? COALIGN_ALIGN_STORE_OVERFLOW : 0;
        g.status[0] = g.slot == 0 ? over : (g.status[0] | over);      // launches of one frame are ordered by the stream
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ (11b) construction
struct BuildArgs {
    int n_agents, wide, udim, flags;
    float thres, yaw_var_thres;
    const void *corners, *unc;
    const int32_t *count;
    const double *noisy;
    int32_t *vertex_off, *edge_off, *graph_agents, *kinds, *edge_agent, *edge_landmark, *status;
    double *vertices, *edge_meas, *edge_info;
};

// exclusive prefix of `v` over the workgroup in thread order, and the total
__device__ __forceinline__ int block_excl_scan(int v, int *wave_tot, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < kThreads / 64; ++i) {
        const int x = wave_tot[i];
        if (i < w) base += x;
        total += x;
    }
    __syncthreads();
    return base + inc - v;
}

__device__ __forceinline__ double corner_at(const void *corners, int wide, size_t i) {
    return wide ? static_cast<const double *>(corners)[i] : (double)static_cast<const float *>(corners)[i];
}

// certainty of one box (box_align.py:115-119, 139-140): exp(-log variance), x / y over the squared anchor diagonal, sqrt under normalize_uncertainty, doubled for
// a point landmark of an adaptive cluster; returns certainty.sum()
__device__ __forceinline__ double box_certainty(const BuildArgs &g, size_t ub, bool normalize, bool doubled, double *c) {
    double total = 0;
    for (int d = 0; d < 3; ++d) c[d] = 0;
    for (int d = 0; d < g.udim; ++d) {
        const double u = g.wide ? static_cast<const double *>(g.unc)[ub + d] : (double)static_cast<const float *>(g.unc)[ub + d];
        c[d] = exp(-u);
        if (d < 2) c[d] /= kAnchorDiagSq;      // var(x) = d_a^2 var(x_t) for the anchor-normalised regression target
        if (normalize) c[d] = sqrt(c[d]);
        if (doubled) c[d] *= 2;
        total += c[d];
    }
    return total;
}

__global__ __launch_bounds__(kThreads) void pose_graph_build_kernel(const BuildArgs g) {
    __shared__ float cx[kMaxBoxes], cy[kMaxBoxes], cz[kMaxBoxes], sq[kMaxBoxes], yw[kMaxBoxes];      // float32 world frame: centre, |centre|^2, yaw
    __shared__ unsigned short members[kMaxBoxes], edge_slot[kMaxBoxes], edge_vertex[kMaxBoxes];      // a box's edge: its row of the edge arrays, its landmark
    __shared__ unsigned char owner[kMaxBoxes], is_free[kMaxBoxes], any_near[kMaxBoxes], edge_kind[kMaxBoxes];      // bit 0 SE(2) landmark, bit 1 certainty doubled
    constexpr unsigned short kNoEdge = 0xffff;
    __shared__ float tfm[kMaxAgents][12];
    __shared__ int start[kMaxAgents + 1], wave_tot[kThreads / 64];
    const int s = blockIdx.x, t = threadIdx.x, NA = g.n_agents;
    const size_t box0 = (size_t)s * kMaxBoxes;
    const double *noisy = g.noisy + (size_t)s * NA * 6;
    double *vertices = g.vertices + (size_t)s * kMaxVertices * 3;
    int32_t *kinds = g.kinds + (size_t)s * kMaxVertices;
    int32_t *edge_agent = g.edge_agent + (size_t)s * kMaxEdges, *edge_landmark = g.edge_landmark + (size_t)s * kMaxEdges;
    double *edge_meas = g.edge_meas + (size_t)s * kMaxEdges * 3, *edge_info = g.edge_info + (size_t)s * kMaxEdges * 3;
    const bool use_unc = (g.flags & COALIGN_ALIGN_USE_UNCERTAINTY) && g.unc != nullptr && g.udim > 0;
    const bool landmark_se2 = g.flags & COALIGN_ALIGN_LANDMARK_SE2, adaptive = g.flags & COALIGN_ALIGN_ADAPTIVE_LANDMARK;
    const bool normalize = g.flags & COALIGN_ALIGN_NORMALIZE_UNCERTAINTY, abandon_hard = g.flags & COALIGN_ALIGN_ABANDON_HARD_CASES;
    const bool drop_hard = g.flags & COALIGN_ALIGN_DROP_HARD_BOXES, drop_unsure = g.flags & COALIGN_ALIGN_DROP_UNSURE_EDGE;

    int word = g.status[s] & COALIGN_ALIGN_STORE_OVERFLOW;
    if (t == 0) {
        int acc = 0;
        for (int a = 0; a < NA; ++a) {
            const int c = g.count[s * kMaxAgents + a];
            start[a] = acc;
            acc += c < 0 ? 0 : (c > kStoreBoxes ? kStoreBoxes : c);
        }
        start[NA] = acc;
    }
    if (t < NA) {                                     // pose_to_tfm (box_align.py:29-50): float32, torch's operation order
        float p[6];
        for (int q = 0; q < 6; ++q) p[q] = (float)noisy[t * 6 + q];
        const float rad = (float)(kPi / 180.0);
        const float yaw = p[4] * rad, roll = p[3] * rad, pitch = p[5] * rad;
        const float cyw = cosf(yaw), syw = sinf(yaw), cr = cosf(roll), sr = sinf(roll), cp = cosf(pitch), sp = sinf(pitch);
        float *m = tfm[t];
        m[0] = cp * cyw; m[1] = cyw * sp * sr - syw * cr; m[2] = -cyw * sp * cr - syw * sr; m[3] = p[0];
        m[4] = syw * cp; m[5] = syw * sp * sr + cyw * cr; m[6] = -syw * sp * cr + cyw * sr; m[7] = p[1];
        m[8] = sp;       m[9] = -cp * sr;                 m[10] = cp * cr;                  m[11] = p[2];
    }
    __syncthreads();
    const int K = start[NA];

    // ---- world frame (box_align.py:107, 112): _project_f32 with the translation as the fourth product of each dot product, corner_to_center in float32
    for (int b = t; b < K; b += kThreads) {
        int a = 0;
        while (a + 1 < NA && b >= start[a + 1]) ++a;
        const size_t base = (box0 + (size_t)a * kStoreBoxes + (b - start[a])) * 24;
        const float *m = tfm[a];
        float wx[8], wy[8], wz[8];
        for (int c = 0; c < 8; ++c) {
            const float x = (float)corner_at(g.corners, g.wide, base + c * 3), y = (float)corner_at(g.corners, g.wide, base + c * 3 + 1),
                        z = (float)corner_at(g.corners, g.wide, base + c * 3 + 2);
            wx[c] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            wy[c] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            wz[c] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        }
        const float x = (((wx[0] + wx[3]) + wx[5]) + wx[6]) * 0.25f, y = (((wy[0] + wy[3]) + wy[5]) + wy[6]) * 0.25f,
                    z = (((wz[0] + wz[3]) + wz[5]) + wz[6]) * 0.25f;
        const float h = ((atan2f(wy[1] - wy[2], wx[1] - wx[2]) + atan2f(wy[0] - wy[3], wx[0] - wx[3])) + atan2f(wy[5] - wy[6], wx[5] - wx[6])) +
                        atan2f(wy[4] - wy[7], wx[4] - wx[7]);
        cx[b] = x; cy[b] = y; cz[b] = z;
        sq[b] = (x * x + y * y) + z * z;              // fixed order, no contraction: see the head of the file
        yw[b] = h * 0.25f;
        owner[b] = (unsigned char)a;
        is_free[b] = 1;
        edge_slot[b] = kNoEdge;
    }
    __syncthreads();
    // all_pair_l2 (box_align.py:120-123): dist = sqrt(sq_i + sq_j - 2 * dot_ij) in float32; NaN compares false; boxes of one agent never pair
    auto near = [&](int i, int j) {
        const float dot = (cx[i] * cx[j] + cy[i] * cy[j]) + cz[i] * cz[j];
        return owner[i] != owner[j] && sqrtf((sq[i] + sq[j]) - 2.f * dot) < g.thres;
    };
    for (int i = t; i < K; i += kThreads) {           // `near[seed].any()` of every box, in parallel: the serial loop below skips the others at once
        unsigned char any = 0;
        for (int j = 0; j < K && !any; ++j) any = near(i, j) ? 1 : 0;
        any_near[i] = any;
    }
    __syncthreads();

    // ---- the greedy pass over seeds in index order (box_align.py:127-144).  Every decision below is taken from LDS by all threads alike (uniform).
    int n_lm = 0, n_edges = 0, n_varies = 0;
    bool too_many = false;
    for (int seed = 0; seed < K; ++seed) {
        if (!is_free[seed] || !any_near[seed]) continue;
        unsigned mask = 0;
        for (int q = 0; q < kPerThread; ++q) {
            const int j = t * kPerThread + q;
            if (j < K && is_free[j] && near(seed, j)) mask |= 1u << q;
        }
        int others;
        int at = 1 + block_excl_scan(__popc(mask), wave_tot, others);
        if (others == 0) {                             // all neighbours already belong to earlier clusters
            if (t == 0) is_free[seed] = 0;
            __syncthreads();
            continue;
        }
        if (n_lm >= kMaxLandmarks) { too_many = true; break; }
        const int n = others + 1;
        if (t == 0) members[0] = (unsigned short)seed;
        for (int q = 0; q < kPerThread; ++q)
            if (mask >> q & 1) members[at++] = (unsigned short)(t * kPerThread + q);      // [seed, ascending j]
        __syncthreads();
        float sum = 0.f, dev = 0.f;                    // np.var(yaw[members]), float32
        for (int r = 0; r < n; ++r) sum += yw[members[r]];
        const float mean = sum / (float)n;
        for (int r = 0; r < n; ++r) { const float d = yw[members[r]] - mean; dev += d * d; }
        const bool varies = dev / (float)n > g.yaw_var_thres;
        const bool se2 = landmark_se2 && !(adaptive && varies);
        const bool doubled = !se2 && landmark_se2;     // adaptive landmark: the point constraint counts double (box_align.py:139-140)
        const int vertex = NA + n_lm;
        if (t == 0) {
            vertices[vertex * 3] = cx[seed];
            vertices[vertex * 3 + 1] = cy[seed];
            vertices[vertex * 3 + 2] = se2 ? yw[seed] : 0.f;
            kinds[vertex] = se2 ? 1 : 2;
        }
        if (!(drop_hard && varies)) {                  // edges of this landmark (box_align.py:154-169): members in order, unsure ones dropped
            const unsigned char kind = (se2 ? 1 : 0) | (doubled ? 2 : 0);
            if (drop_unsure && use_unc) {              // which members keep their edge depends on their certainties: look, then rank
                for (int r0 = 0; r0 < n; r0 += kThreads) {
                    const int r = r0 + t;
                    bool emit = r < n;
                    int j = 0;
                    if (emit) {
                        j = members[r];
                        const int a = owner[j];
                        double c[3];
                        emit = !(box_certainty(g, (box0 + (size_t)a * kStoreBoxes + (j - start[a])) * g.udim, normalize, doubled, c) < 100);
                    }
                    int emitted;
                    const int e = n_edges + block_excl_scan(emit ? 1 : 0, wave_tot, emitted);
                    if (emit) { edge_slot[j] = (unsigned short)e; edge_vertex[j] = (unsigned short)vertex; edge_kind[j] = kind; }
                    n_edges += emitted;
                }
            } else {
                for (int r = t; r < n; r += kThreads) {
                    const int j = members[r];
                    edge_slot[j] = (unsigned short)(n_edges + r);
                    edge_vertex[j] = (unsigned short)vertex;
                    edge_kind[j] = kind;
                }
                n_edges += n;
            }
        }
        for (int r = t; r < n; r += kThreads) is_free[members[r]] = 0;
        ++n_lm;
        n_varies += varies ? 1 : 0;
        __syncthreads();
    }

    // ---- what the edges hold (box_align.py:160-169), all boxes in parallel: the measurement is corner_to_center in float64 in the agent's own frame
    __syncthreads();
    for (int j = t; j < K; j += kThreads) {
        const int e = edge_slot[j];
        if (e == kNoEdge || e >= kMaxEdges) continue;
        const int a = owner[j];
        const bool se2 = edge_kind[j] & 1, doubled = edge_kind[j] & 2;
        const size_t box = box0 + (size_t)a * kStoreBoxes + (j - start[a]);
        double x[8], y[8], info[3] = {1, 1, 1};
        for (int c = 0; c < 8; ++c) { x[c] = corner_at(g.corners, g.wide, box * 24 + c * 3); y[c] = corner_at(g.corners, g.wide, box * 24 + c * 3 + 1); }
        double yaw = (((atan2(y[1] - y[2], x[1] - x[2]) + atan2(y[0] - y[3], x[0] - x[3])) + atan2(y[5] - y[6], x[5] - x[6])) + atan2(y[4] - y[7], x[4] - x[7])) / 4;
        if (use_unc) {
            double c[3];
            box_certainty(g, box * g.udim, normalize, doubled, c);
            for (int d = 0; d < (se2 ? 3 : 2) && d < g.udim; ++d) info[d] = c[d];
        }
        if (!se2) yaw = info[2] = 0.0;
        edge_agent[e] = a;
        edge_landmark[e] = edge_vertex[j];
        edge_meas[e * 3] = (((x[0] + x[3]) + x[5]) + x[6]) / 4;
        edge_meas[e * 3 + 1] = (((y[0] + y[3]) + y[5]) + y[6]) / 4;
        edge_meas[e * 3 + 2] = yaw;
        for (int d = 0; d < 3; ++d) edge_info[e * 3 + d] = info[d];
    }

    // ---- the sample's word, the agents' vertices, the offsets the solver reads
    if (too_many) word |= COALIGN_ALIGN_TOO_MANY_LANDMARKS;
    if (word) word |= COALIGN_ALIGN_OUTSIDE_LIMITS;
    else if (K == 0) word = COALIGN_ALIGN_NO_BOXES;
    else if (abandon_hard && (n_lm <= 3 || 2 * n_varies >= n_lm)) word = COALIGN_ALIGN_KEPT_NOISY;      // box_align.py:146
    if (t < NA) {
        vertices[t * 3] = noisy[t * 6];
        vertices[t * 3 + 1] = noisy[t * 6 + 1];
        vertices[t * 3 + 2] = noisy[t * 6 + 4] * (kPi / 180.0);
        kinds[t] = t == 0 ? 0 : 1;                     // the ego pose is the gauge
    }
    if (t == 0) {
        const bool solve = word == COALIGN_ALIGN_SOLVED;
        g.vertex_off[s * 2] = 0;
        g.vertex_off[s * 2 + 1] = solve ? NA + n_lm : NA;
        g.edge_off[s * 2] = 0;
        g.edge_off[s * 2 + 1] = solve ? n_edges : 0;
        g.graph_agents[s] = NA;
        g.status[s] = word;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ (11c) matrices
struct MatrixArgs {
    int n_agents, L, proj_first;
    double H, W, den_x, den_y;
    const double *noisy, *vertices;
    const int32_t *status;
    double *poses_out, *pairwise, *affine;
};

__global__ __launch_bounds__(kThreads) void pose_matrices_kernel(const MatrixArgs g) {
    __shared__ double T[kMaxAgents][12];              // x_to_world (pose.py:19-34): rows of Rz(yaw) Ry'(pitch) Rx'(roll) | translation
    const int s = blockIdx.x, t = threadIdx.x, NA = g.n_agents, L = g.L;
    if (t < NA) {
        const double *in = g.noisy + ((size_t)s * NA + t) * 6, *v = g.vertices + ((size_t)s * kMaxVertices + t) * 3;
        double p[6];
        for (int q = 0; q < 6; ++q) p[q] = in[q];
        if (g.status[s] == COALIGN_ALIGN_SOLVED) {    // refined (x, y, yaw): radians -> degrees, like the input poses (box_align.py:196-201)
            p[0] = v[0];
            p[1] = v[1];
            p[4] = v[2] * (180.0 / kPi);
        }
        double *out = g.poses_out + ((size_t)s * NA + t) * 6;
        for (int q = 0; q < 6; ++q) out[q] = p[q];
        const double yaw = p[4] * (kPi / 180.0), roll = p[3] * (kPi / 180.0), pitch = p[5] * (kPi / 180.0);
        const double cyw = cos(yaw), syw = sin(yaw), cr = cos(roll), sr = sin(roll), cp = cos(pitch), sp = sin(pitch);
        double *m = T[t];
        m[0] = cyw * cp; m[1] = cyw * sp * sr - syw * cr; m[2] = -cyw * sp * cr - syw * sr; m[3] = p[0];
        m[4] = syw * cp; m[5] = syw * sp * sr + cyw * cr; m[6] = -syw * sp * cr + cyw * sr; m[7] = p[1];
        m[8] = sp;       m[9] = -cp * sr;                 m[10] = cp * cr;                  m[11] = p[2];
    }
    __syncthreads();
    for (int pr = t; pr < L * L; pr += kThreads) {
        const int i = pr / L, j = pr % L;
        double M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (!g.proj_first && i < NA && j < NA && i != j) {          // T_j^-1 T_i of two rigid transforms: R_j^T R_i | R_j^T (t_i - t_j)
            const double *a = T[i], *b = T[j];
            const double d[3] = {a[3] - b[3], a[7] - b[7], a[11] - b[11]};
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) M[r * 4 + c] = b[r] * a[c] + b[4 + r] * a[4 + c] + b[8 + r] * a[8 + c];
                M[r * 4 + 3] = b[r] * d[0] + b[4 + r] * d[1] + b[8 + r] * d[2];
            }
        }
        double *pw = g.pairwise + ((size_t)s * L * L + pr) * 16, *af = g.affine + ((size_t)s * L * L + pr) * 6;
        for (int q = 0; q < 16; ++q) pw[q] = M[q];
        af[0] = M[0];                                 // normalize_pairwise_tfm (pose.py:70-83), the same operations in the same order
        af[1] = M[1] * g.H / g.W;
        af[2] = M[3] / g.den_x * 2;
        af[3] = M[4] * g.W / g.H;
        af[4] = M[5];
        af[5] = M[7] / g.den_y * 2;
    }
}

}  // namespace

extern "C" int coalign_align_store_boxes(void) { return kStoreBoxes; }

extern "C" int coalign_stage1_gather(const int32_t *keep, const int32_t *keep_count, const int32_t *cand_index, const float *cand_corners, int capacity,
                                     const float *unc, int A, int udim, int H, int W, int slot, float *store_corners, float *store_unc, int32_t *store_count,
                                     int32_t *status, void *stream) {
    using namespace coalign;
    if (capacity <= 0 || A <= 0 || H <= 0 || W <= 0 || udim < 0 || slot < 0) return COALIGN_ERR_BAD_SHAPE;
    if (slot >= kMaxAgents || udim > 3 || (long long)A * H * W > 0x7fffffffLL) return COALIGN_ERR_UNSUPPORTED;
    if (!keep || !keep_count || !cand_index || !cand_corners || !store_corners || !store_count || !status) return COALIGN_ERR_NULL_POINTER;
    if (udim > 0 && (!unc || !store_unc)) return COALIGN_ERR_NULL_POINTER;
    GatherArgs g{keep, keep_count, cand_index, cand_corners, unc, capacity, A, udim, H * W, slot, store_corners, store_unc, store_count, status};
    hipLaunchKernelGGL(stage1_gather_kernel, dim3(kStoreBoxes * 24 / kThreads), dim3(kThreads), 0, static_cast<hipStream_t>(stream), g);
    return check_launch();
}

extern "C" int coalign_pose_graph_build(int n_samples, int n_agents, const void *corners, const void *unc, int wide, int udim, const int32_t *count,
                                        const double *noisy_poses, int flags, double thres, double yaw_var_thres, int32_t *vertex_off, int32_t *edge_off,
                                        int32_t *graph_agents, double *vertices, int32_t *kinds, int32_t *edge_agent, int32_t *edge_landmark, double *edge_meas,
                                        double *edge_info, int32_t *status, void *stream) {
    using namespace coalign;
    if (n_samples < 0 || n_agents < 1 || udim < 0 || flags < 0) return COALIGN_ERR_BAD_SHAPE;
    if (n_agents > kMaxAgents || udim > 3 || (wide != 0 && wide != 1) || flags > 127) return COALIGN_ERR_UNSUPPORTED;
    if (n_samples == 0) return COALIGN_OK;
    if (!corners || !count || !noisy_poses || !vertex_off || !edge_off || !graph_agents || !vertices || !kinds || !edge_agent || !edge_landmark || !edge_meas ||
        !edge_info || !status)
        return COALIGN_ERR_NULL_POINTER;
    BuildArgs g{n_agents, wide, unc ? udim : 0, flags, (float)thres, (float)yaw_var_thres, corners, unc, count, noisy_poses, vertex_off, edge_off, graph_agents,
                kinds, edge_agent, edge_landmark, status, vertices, edge_meas, edge_info};
    hipLaunchKernelGGL(pose_graph_build_kernel, dim3(n_samples), dim3(kThreads), 0, static_cast<hipStream_t>(stream), g);
    return check_launch();
}

extern "C" int coalign_pose_correct_matrices(int n_samples, int n_agents, const double *noisy_poses, const double *vertices, const int32_t *status, int max_cav,
                                             int proj_first, int H, int W, double den_x, double den_y, double *poses_out, double *pairwise, double *affine,
                                             void *stream) {
    using namespace coalign;
    if (n_samples < 0 || n_agents < 1 || max_cav < 1 || H <= 0 || W <= 0 || !(den_x > 0) || !(den_y > 0)) return COALIGN_ERR_BAD_SHAPE;
    if (n_agents > kMaxAgents || max_cav > kMaxCav) return COALIGN_ERR_UNSUPPORTED;
    if (n_agents > max_cav) return COALIGN_ERR_BAD_SHAPE;
    if (n_samples == 0) return COALIGN_OK;
    if (!noisy_poses || !vertices || !status || !poses_out || !pairwise || !affine) return COALIGN_ERR_NULL_POINTER;
    MatrixArgs g{n_agents, max_cav, proj_first ? 1 : 0, (double)H, (double)W, den_x, den_y, noisy_poses, vertices, status, poses_out, pairwise, affine};
    hipLaunchKernelGGL(pose_matrices_kernel, dim3(n_samples), dim3(kThreads), 0, static_cast<hipStream_t>(stream), g);
    return check_launch();
}
