// Host-side memory safety of the message entry points' argument checks (csrc/w2comm_msg.hip): a stand-alone program, built with the host half under
// AddressSanitizer and UndefinedBehaviorSanitizer by tools/w2comm_msg_args_check.sh and run on a machine WITHOUT a GPU.  Every call below is refused by a check,
// so none reaches a launch; the host arrays are heap blocks of exactly the size the header states, so a check that read past one would be reported.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "coalign_amd_where2comm_msg.h"

static int failures = 0;
#define EXPECT(call, want)                                                                   \
    do {                                                                                     \
        const int got = (call);                                                              \
        if (got != (want)) { std::printf("%s:%d: %s = %d, expected %d\n", __FILE__, __LINE__, #call, got, (want)); ++failures; } \
    } while (0)

template <class T>
struct Exact {          // a heap array of exactly n entries
    std::vector<T> v;
    explicit Exact(std::initializer_list<T> init) : v(init) { v.shrink_to_fit(); }
    T *get() { return v.data(); }
};

int main() {
    void *const tok = reinterpret_cast<void *>(16), *const odd = reinterpret_cast<void *>(18);
    using U8 = const uint8_t *; using U32 = uint32_t *; using I32 = int32_t *; using F = float *; using CF = const float *; using CU32 = const uint32_t *; using CI32 = const int32_t *;
    Exact<int32_t> H{9, 4, 2}, W{33, 16, 8}, C{64, 128, 256}, Hbig{65536, 4, 2}, Wbig{65536, 16, 8}, Cbad{64, 96, 256}, Hzero{9, 0, 2};
    Exact<U8> masks{(U8)tok, (U8)tok, (U8)tok}, masks_hole{(U8)tok, nullptr, (U8)tok};
    Exact<U32> bits{(U32)tok, (U32)tok, (U32)tok}, bits_odd{(U32)tok, (U32)odd, (U32)tok}, bits_hole{(U32)tok, (U32)tok, nullptr};
    Exact<I32> rank{(I32)tok, (I32)tok, (I32)tok}, rank_odd{(I32)odd, (I32)tok, (I32)tok};
    // (15a)
    EXPECT(coalign_w2comm_msg_index(3, 3, nullptr, W.get(), masks.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_index(3, 3, H.get(), W.get(), masks.get(), nullptr, rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_index(3, 3, H.get(), W.get(), masks.get(), bits.get(), rank.get(), nullptr, nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_index(3, 3, H.get(), W.get(), masks_hole.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_index(3, 3, H.get(), W.get(), nullptr, bits_hole.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_index(0, 3, H.get(), W.get(), masks.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_BAD_SHAPE);
    EXPECT(coalign_w2comm_msg_index(3, 0, H.get(), W.get(), masks.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_BAD_SHAPE);
    EXPECT(coalign_w2comm_msg_index(3, 3, Hzero.get(), W.get(), masks.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_BAD_SHAPE);
    EXPECT(coalign_w2comm_msg_index(3, 3, Hbig.get(), Wbig.get(), masks.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_BAD_SHAPE);
    EXPECT(coalign_w2comm_msg_index(9, 3, H.get(), W.get(), masks.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_index(3, 4, H.get(), W.get(), masks.get(), bits.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_index(3, 3, H.get(), W.get(), masks.get(), bits_odd.get(), rank.get(), (int32_t *)tok, nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_index(3, 3, H.get(), W.get(), masks.get(), bits.get(), rank_odd.get(), (int32_t *)tok, nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_index(3, 3, H.get(), W.get(), masks.get(), bits.get(), rank.get(), (int32_t *)odd, nullptr), COALIGN_ERR_UNSUPPORTED);
    // (15b)
    Exact<CF> x{(CF)tok, (CF)tok, (CF)tok}, x_odd{(CF)tok, (CF)tok, (CF)reinterpret_cast<void *>(24)};
    Exact<CU32> cbits{(CU32)tok, (CU32)tok, (CU32)tok};
    Exact<CI32> crank{(CI32)tok, (CI32)tok, (CI32)tok}, crank_hole{(CI32)tok, nullptr, (CI32)tok};
    Exact<F> rows{(F)tok, (F)tok, (F)tok}, rows_odd{(F)tok, (F)reinterpret_cast<void *>(20), (F)tok};
    EXPECT(coalign_w2comm_msg_pack(3, 3, nullptr, C.get(), H.get(), W.get(), cbits.get(), crank.get(), rows.get(), nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_pack(3, 3, x.get(), C.get(), H.get(), W.get(), cbits.get(), crank_hole.get(), rows.get(), nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_pack(3, 3, x.get(), C.get(), H.get(), W.get(), cbits.get(), crank.get(), nullptr, nullptr), COALIGN_ERR_NULL_POINTER);
    EXPECT(coalign_w2comm_msg_pack(3, 3, x.get(), C.get(), Hzero.get(), W.get(), cbits.get(), crank.get(), rows.get(), nullptr), COALIGN_ERR_BAD_SHAPE);
    EXPECT(coalign_w2comm_msg_pack(3, 3, x.get(), C.get(), Hbig.get(), Wbig.get(), cbits.get(), crank.get(), rows.get(), nullptr), COALIGN_ERR_BAD_SHAPE);
    EXPECT(coalign_w2comm_msg_pack(3, 3, x.get(), Cbad.get(), H.get(), W.get(), cbits.get(), crank.get(), rows.get(), nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_pack(9, 3, x.get(), C.get(), H.get(), W.get(), cbits.get(), crank.get(), rows.get(), nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_pack(3, 4, x.get(), C.get(), H.get(), W.get(), cbits.get(), crank.get(), rows.get(), nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_pack(3, 3, x.get(), C.get(), H.get(), W.get(), cbits.get(), crank.get(), rows_odd.get(), nullptr), COALIGN_ERR_UNSUPPORTED);
    EXPECT(coalign_w2comm_msg_pack(3, 3, x_odd.get(), C.get(), H.get(), W.get(), cbits.get(), crank.get(), rows.get(), nullptr), COALIGN_ERR_UNSUPPORTED);
    // (15c): two scales of three agents, the ego dense and the others packed: arrays of exactly 2 x 3 entries
    using CV = const void *;
    Exact<int32_t> C2{64, 256}, H2{9, 4}, W2{14, 7}, kind{0, 1, 1, 0, 1, 1}, kind_bad{0, 1, 1, 0, 1, 2}, C2bad{64, 32}, H2big{9, 4096}, W2big{14, 4096};
    Exact<CF> src{(CF)tok, (CF)tok, (CF)tok, (CF)tok, (CF)tok, (CF)tok}, src_hole{(CF)tok, (CF)tok, (CF)tok, (CF)tok, (CF)tok, nullptr}, src_odd{(CF)tok, (CF)tok, (CF)tok, (CF)tok, (CF)tok, (CF)reinterpret_cast<void *>(20)};
    Exact<CV> aux{nullptr, tok, tok, tok, tok, tok}, aux_hole{nullptr, tok, tok, tok, tok, nullptr}, aux_odd{nullptr, tok, odd, tok, tok, tok};
    Exact<CI32> frank{nullptr, (CI32)tok, (CI32)tok, nullptr, (CI32)tok, (CI32)tok}, frank_hole{nullptr, (CI32)tok, (CI32)tok, nullptr, nullptr, (CI32)tok};
    Exact<F> out{(F)reinterpret_cast<void *>(32), (F)reinterpret_cast<void *>(32)}, out_odd{(F)reinterpret_cast<void *>(32), (F)reinterpret_cast<void *>(8)};
    const double *theta = reinterpret_cast<const double *>(tok);
#define FUSE(ns, c, h, w, k, s, a, r, o, n, th, mode) coalign_w2comm_fuse_packed(ns, c.get(), h.get(), w.get(), k.get(), s.get(), a.get(), r.get(), o.get(), h.get(), w.get(), n, th, mode, nullptr)
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux, frank, out, 3, nullptr, COALIGN_FUSE_ATT), COALIGN_ERR_NULL_POINTER);
    EXPECT(FUSE(2, C2, H2, W2, kind, src_hole, aux, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_NULL_POINTER);
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux_hole, frank, out, 3, theta, COALIGN_FUSE_MAX), COALIGN_ERR_NULL_POINTER);
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux, frank_hole, out, 3, theta, COALIGN_FUSE_MAX), COALIGN_ERR_NULL_POINTER);      // a packed source without rank
    EXPECT(FUSE(0, C2, H2, W2, kind, src, aux, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_BAD_SHAPE);
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux, frank, out, 0, theta, COALIGN_FUSE_ATT), COALIGN_ERR_BAD_SHAPE);
    EXPECT(FUSE(2, C2, H2big, W2big, kind, src, aux, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_BAD_SHAPE);
    EXPECT(FUSE(4, C2, H2, W2, kind, src, aux, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_UNSUPPORTED);
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux, frank, out, 9, theta, COALIGN_FUSE_ATT), COALIGN_ERR_UNSUPPORTED);
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux, frank, out, 3, theta, COALIGN_FUSE_NONE), COALIGN_ERR_UNSUPPORTED);
    EXPECT(FUSE(2, C2bad, H2, W2, kind, src, aux, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_UNSUPPORTED);
    EXPECT(FUSE(2, C2, H2, W2, kind_bad, src, aux, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_UNSUPPORTED);
    EXPECT(FUSE(2, C2, H2, W2, kind, src_odd, aux, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_UNSUPPORTED);
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux_odd, frank, out, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_UNSUPPORTED);
    EXPECT(FUSE(2, C2, H2, W2, kind, src, aux, frank, out_odd, 3, theta, COALIGN_FUSE_ATT), COALIGN_ERR_UNSUPPORTED);
    std::printf(failures ? "%d check(s) failed\n" : "all argument checks refused as stated (%d failures)\n", failures);
    return failures ? 1 : 0;
}
