// plan_probe.cpp — the record arithmetic of onc_fragment_iov
// (onc-rpc_amd/csrc/fragment_iov_plan.h) on the CPU: compiled with the host
// compiler (and -fsanitize=undefined where the toolchain has it) and run by
// tests/test_fragment_iov_host.py. The kernels call the same functions. The
// piece map is checked against a walk over the fragments as the loop in
// include/onc_rpc.h writes them, the 64-bit counts at every length (on the GPU:
// tests/test_gpu_far_offsets.py, entries of 4 GiB), both capacity tests near 2^64, and the plan's scan at every
// blocking of a record list.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fragment_iov_plan.h"

static int g_fail = 0;
#define EXPECT(expr, want)                                                                              \
    do {                                                                                                \
        const uint64_t got_ = uint64_t(expr);                                                           \
        if (got_ != uint64_t(want)) {                                                                   \
            std::printf("FAIL line %d: %s = %llu, want %llu\n", __LINE__, #expr, (unsigned long long)got_, \
                        (unsigned long long)uint64_t(want));                                            \
            ++g_fail;                                                                                   \
        }                                                                                               \
    } while (0)

using namespace onc;

// The pieces of one record as the header's loop lists them (relative to the
// record: marks from its first, header and payload offsets from its own).
static std::vector<FivPiece> walk_pieces(uint32_t hl, uint32_t pl, uint32_t F, std::vector<uint32_t>* marks) {
    std::vector<FivPiece> out;
    const uint64_t Hb = hl - 4u, B = uint64_t(hl) + pl - 4;
    uint64_t k = B / F + (B % F ? 1 : 0);
    if (!k) k = 1;
    for (uint64_t j = 0; j < k; ++j) {
        const uint64_t a = j * F, b = (j + 1) * F < B ? (j + 1) * F : B;
        marks->push_back((j == k - 1 ? 0x80000000u : 0u) | uint32_t(b - a));
        out.push_back(FivPiece{4 * j, 4, ONC_PIECE_MARK});
        if (a < Hb && b > a) out.push_back(FivPiece{4 + a, uint32_t((b < Hb ? b : Hb) - a), ONC_PIECE_HDR});
        if (b > Hb && pl > 0) {
            const uint64_t s = a > Hb ? a : Hb;
            out.push_back(FivPiece{s - Hb, uint32_t(b - s), ONC_PIECE_PAYLOAD});
        }
    }
    return out;
}

static void walk(uint32_t hl, uint32_t pl, uint32_t F) {
    std::vector<uint32_t> marks;
    const std::vector<FivPiece> want = walk_pieces(hl, pl, F, &marks);
    const FivRec r = fiv_rec(hl, pl, F);
    const FivShape sh = fiv_shape(hl, pl, F);
    EXPECT(r.status, ONC_OK);
    EXPECT(r.k, marks.size());
    EXPECT(r.e, want.size());
    EXPECT(r.len, 4 * marks.size() + sh.B);
    EXPECT(r.k, frag_count(sh.B, F));
    uint64_t bytes = 0;
    for (uint64_t t = 0; t < want.size(); ++t) {
        const FivAt at = fiv_at(sh, t);
        const FivPiece p = fiv_piece(sh, F, at);
        EXPECT(p.src, want[t].src);
        EXPECT(p.off, want[t].off);
        EXPECT(p.len, want[t].len);
        EXPECT(p.len > 0, 1);
        if (at.c == 0) {
            EXPECT(fiv_first_piece(sh, at.j), t);
            EXPECT(frag_mark(sh.B, at.j, F), marks[at.j]);
        } else {
            bytes += p.len;
        }
    }
    EXPECT(bytes, sh.B);
}

// The plan as the kernels run it: sums of blocks of `blk` records, their
// scan, then the records — any blocking must give what one serial pass gives.
struct Entry {
    uint32_t hl, pl, F;
};
struct Placed {
    FivAgg at;
    int32_t status;
};
static std::vector<Placed> plan(const std::vector<Entry>& L, uint64_t max_pieces, uint64_t marks_cap, size_t blk,
                                FivAgg* all) {
    std::vector<FivAgg> base;
    FivAgg carry = fiv_none();
    for (size_t b = 0; b < L.size(); b += blk) {
        base.push_back(carry);
        FivAgg run = fiv_none();
        for (size_t i = b; i < b + blk && i < L.size(); ++i)
            run = fiv_join(run, fiv_elem(fiv_rec(L[i].hl, L[i].pl, L[i].F)));
        carry = fiv_join(carry, run);
    }
    *all = carry;
    std::vector<Placed> out;
    for (size_t b = 0; b < L.size(); b += blk) {
        FivAgg s = base[b / blk];
        for (size_t i = b; i < b + blk && i < L.size(); ++i) {
            const FivRec r = fiv_rec(L[i].hl, L[i].pl, L[i].F);
            out.push_back(Placed{s, fiv_status(r, s.pieces, max_pieces, s.frags, marks_cap)});
            s = fiv_join(s, fiv_elem(r));
        }
    }
    return out;
}

int main() {
    const uint64_t kMax = ~uint64_t(0);
    const uint32_t kF = kFragMaxBody, k32 = 0xFFFFFFFFu;
    // the piece map against the walk
    for (uint32_t F = 1; F < 45; ++F)
        for (uint32_t Hb = 0; Hb < 40; ++Hb)
            for (uint32_t P = 0; P < 40; ++P) walk(Hb + 4, P, F);
    walk(4 + 1000, 5000, 1000);
    walk(4 + 999, 5000, 1000);
    walk(460, 4096, 1024);
    walk(28, 100000, 7);

    // entries that are no records
    EXPECT(fiv_rec(0, 0, 7).status, ONC_OK);
    EXPECT(fiv_rec(0, 0, 0).status, ONC_OK);               // nothing to send, whatever the limit
    EXPECT(fiv_rec(0, 0, 7).e, 0);
    for (uint32_t hl : {0u, 1u, 3u}) {
        const FivRec r = fiv_rec(hl, 9, 7);
        EXPECT(r.status, ONC_ENC_BAD_DESCRIPTOR);
        EXPECT(r.k + r.len + r.e, 0);
        EXPECT(fiv_status(r, 0, 0, 0, 0), ONC_ENC_BAD_DESCRIPTOR);
        EXPECT(fiv_elem(r).multi, 0);
    }
    for (uint32_t F : {0u, 0x80000000u, k32}) {
        const FivRec r = fiv_rec(28, 9, F);
        EXPECT(r.status, ONC_ENC_BAD_DESCRIPTOR);
        EXPECT(r.k + r.len + r.e, 0);
    }
    EXPECT(fiv_rec(4, 0, 7).e, 1);                          // the bare mark
    EXPECT(fiv_rec(4, 0, 7).k, 1);
    EXPECT(fiv_rec(4, 0, 7).len, 4);

    // the largest entry, at the smallest and the largest limit: nothing wraps
    {
        const uint64_t B = 2 * uint64_t(k32) - 4;           // 2^33 - 6
        const FivRec a = fiv_rec(k32, k32, 1);
        EXPECT(a.status, ONC_OK);
        EXPECT(a.k, B);
        EXPECT(a.len, 5 * B);
        EXPECT(a.e, 2 * B);                                 // x = 0: every fragment is one byte
        const FivShape sa = fiv_shape(k32, k32, 1);
        EXPECT(sa.Hb, uint64_t(k32) - 4);
        EXPECT(sa.s, uint64_t(k32) - 4);
        const FivAt last = fiv_at(sa, a.e - 1), mid = fiv_at(sa, 2 * sa.Hb + 1), midm = fiv_at(sa, 2 * sa.Hb);
        EXPECT(last.j, B - 1);
        EXPECT(last.c, 1);
        EXPECT(fiv_piece(sa, 1, last).src, ONC_PIECE_PAYLOAD);
        EXPECT(fiv_piece(sa, 1, last).off, uint64_t(k32) - 1);
        EXPECT(fiv_piece(sa, 1, last).len, 1);
        EXPECT(mid.j, sa.Hb);                               // the first payload byte
        EXPECT(fiv_piece(sa, 1, mid).src, ONC_PIECE_PAYLOAD);
        EXPECT(fiv_piece(sa, 1, mid).off, 0);
        EXPECT(fiv_piece(sa, 1, midm).off, 4 * sa.Hb);      // its mark: beyond 2^32 bytes into the record's marks
        EXPECT(fiv_piece(sa, 1, fiv_at(sa, 2 * sa.Hb - 1)).src, ONC_PIECE_HDR);
        EXPECT(fiv_piece(sa, 1, fiv_at(sa, 2 * sa.Hb - 1)).off, 4 + sa.Hb - 1);
        EXPECT(frag_mark(B, B - 1, 1), 0x80000001u);
        EXPECT(frag_mark(B, B - 2, 1), 1);

        const FivRec b = fiv_rec(k32, k32, kF);             // 2^33 - 6 = 3 (2^31 - 1) + (2^31 - 3)
        EXPECT(b.status, ONC_OK);
        EXPECT(b.k, 4);
        EXPECT(b.len, 16 + B);
        EXPECT(b.e, 9);                                     // the header ends inside fragment 1
        const FivShape sb = fiv_shape(k32, k32, kF);
        EXPECT(sb.s, 1);
        EXPECT(sb.x, 1);
        const uint32_t srcs[9] = {0, 1, 0, 1, 2, 0, 2, 0, 2};
        uint64_t sum = 0;
        for (uint64_t t = 0; t < 9; ++t) {
            const FivPiece p = fiv_piece(sb, kF, fiv_at(sb, t));
            EXPECT(p.src, srcs[t]);
            if (p.src != ONC_PIECE_MARK) sum += p.len;
        }
        EXPECT(sum, B);
        EXPECT(fiv_piece(sb, kF, fiv_at(sb, 3)).len, uint64_t(k32) - 4 - kF);   // header bytes of fragment 1
        EXPECT(fiv_piece(sb, kF, fiv_at(sb, 4)).off, 0);
        EXPECT(fiv_piece(sb, kF, fiv_at(sb, 8)).len, uint64_t(kF) - 2);
        EXPECT(frag_mark(B, 3, kF), 0x80000000u | (kF - 2));
        // a header alone of that length
        EXPECT(fiv_rec(k32, 0, 1).e, 2 * (uint64_t(k32) - 4));
        EXPECT(fiv_rec(4, k32, 1).e, 2 * uint64_t(k32));
        EXPECT(fiv_rec(4, k32, kF).k, 3);                   // 2^32 - 1 = 2 (2^31 - 1) + 1
        EXPECT(fiv_rec(4, k32, kF).e, 6);
    }

    // both capacities: no sum and no product of a position is formed
    {
        const FivRec r = fiv_rec(14, 10, 7);                // 3 fragments, 7 pieces
        EXPECT(r.k, 3);
        EXPECT(r.e, 7);
        EXPECT(fiv_status(r, 0, 7, 0, 12), ONC_OK);
        EXPECT(fiv_status(r, 0, 6, 0, 12), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(r, 0, 7, 0, 11), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(r, 0, 7, 0, 15), ONC_OK);         // a capacity that is no multiple of 4
        EXPECT(fiv_status(r, 1, 7, 0, 12), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(r, 0, 7, 1, 15), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(r, 0, 7, 1, 16), ONC_OK);
        EXPECT(fiv_status(r, 0, 0, 0, kMax), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(r, 0, kMax, 0, 0), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(fiv_rec(0, 0, 7), 5, 0, 5, 0), ONC_OK);               // nothing to send fits anywhere
        EXPECT(fiv_status(r, kMax - 7, kMax, 0, kMax), ONC_OK);
        EXPECT(fiv_status(r, kMax - 6, kMax, 0, kMax), ONC_ENC_WRITE_ZERO);     // np + e wraps to 0
        EXPECT(fiv_status(r, kMax, kMax, 0, kMax), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(r, 0, kMax, kMax / 4 - 3, kMax), ONC_OK);
        EXPECT(fiv_status(r, 0, kMax, kMax / 4 - 2, kMax), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(r, 0, kMax, kMax / 4 + 1, kMax), ONC_ENC_WRITE_ZERO); // 4 nf wraps to 0
        EXPECT(fiv_status(r, 0, kMax, kMax - 1, kMax), ONC_ENC_WRITE_ZERO);     // 4 nf wraps to kMax - 7
        const FivRec big = fiv_rec(k32, k32, 1);
        EXPECT(fiv_status(big, kMax - big.e, kMax, kMax / 4 - big.k, kMax), ONC_OK);
        EXPECT(fiv_status(big, kMax - big.e + 1, kMax, 0, kMax), ONC_ENC_WRITE_ZERO);
        EXPECT(fiv_status(big, 0, kMax, kMax / 4 - big.k + 1, kMax), ONC_ENC_WRITE_ZERO);
    }

    // the plan's scan, at every blocking; a limit per record
    const std::vector<Entry> L = {{0, 0, 8}, {4, 0, 8}, {3, 0, 8}, {14, 10, 7}, {0, 5, 8}, {0, 0, 0},
                                  {28, 80, 8}, {4, 0, 1}, {28, 9, 0}, {8, 8, 8}, {5, 4, 100}, {0, 0, 8}};
    // fragments: 0 1 0 3 0 0 13 1 0 2 1 0; pieces: 0 1 0 7 0 0 26 1 0 5 3 0; bytes: 0 4 0 32 0 0 156 4 0 20 9 0
    const uint64_t wantP[] = {0, 0, 1, 1, 8, 8, 8, 34, 35, 35, 40, 43};
    const uint64_t wantF[] = {0, 0, 1, 1, 4, 4, 4, 17, 18, 18, 20, 21};
    const uint64_t wantB[] = {0, 0, 4, 4, 36, 36, 36, 192, 196, 196, 216, 225};
    const uint64_t caps[][2] = {{kMax, kMax}, {43, 84}, {42, 84}, {43, 83}, {8, kMax}, {kMax, 16}, {kMax, 19},
                                {7, kMax}, {0, kMax}, {kMax, 0}, {0, 0}};
    for (const auto& cap : caps) {
        for (size_t blk = 1; blk <= L.size() + 1; ++blk) {
            FivAgg all;
            const std::vector<Placed> p = plan(L, cap[0], cap[1], blk, &all);
            EXPECT(all.bytes, 225);
            EXPECT(all.frags, 21);
            EXPECT(all.multi, 3);
            EXPECT(all.pieces, 43);
            bool cut = false;
            for (size_t i = 0; i < L.size(); ++i) {
                EXPECT(p[i].at.pieces, wantP[i]);
                EXPECT(p[i].at.frags, wantF[i]);
                EXPECT(p[i].at.bytes, wantB[i]);
                const FivRec r = fiv_rec(L[i].hl, L[i].pl, L[i].F);
                int32_t want = r.status;
                if (r.k) {
                    const bool fits = wantP[i] + r.e <= cap[0] && 4 * (wantF[i] + r.k) <= cap[1];
                    want = fits ? ONC_OK : ONC_ENC_WRITE_ZERO;
                    if (cut) EXPECT(fits, 0);               // nothing fits after the first record that does not
                    cut = cut || !fits;
                }
                EXPECT(p[i].status, want);
            }
        }
    }
    // sums near 2^64 wrap the same way in any grouping (unsigned arithmetic)
    const FivAgg a{kMax - 5, 1, 0, kMax}, b{4, 2, 1, 1}, c{9, 3, 1, 5};
    const FivAgg l = fiv_join(fiv_join(a, b), c), r = fiv_join(a, fiv_join(b, c));
    EXPECT(l.bytes, r.bytes);
    EXPECT(l.bytes, 7);
    EXPECT(l.frags, 6);
    EXPECT(l.multi, 2);
    EXPECT(l.pieces, r.pieces);
    EXPECT(l.pieces, 5);
    if (g_fail) return 1;
    std::printf("fragment iov plan ok\n");
    return 0;
}
