// plan_probe.cpp — the record arithmetic of onc_defragment
// (onc-rpc_amd/csrc/defrag_plan.h) up to sizes no buffer has (the GPU tests
// stop at a 4.4 GB stream, tests/test_gpu_beyond_4gib.py), on the CPU: compiled with the host compiler (and -fsanitize=undefined where the
// toolchain has it) and run by tests/test_defrag_host.py. The kernels call
// the same functions.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "defrag_plan.h"

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

struct Frag {
    uint64_t body;
    bool last;
};
struct Rec {
    uint64_t first, B;
    bool multi;
};

// The plan as the kernels run it: the state before every fragment by joining
// runs, here in blocks of `blk` fragments (block states first, then their
// scan, then the fragments) — any blocking must give what one serial pass gives.
static std::vector<Rec> plan(const std::vector<Frag>& f, size_t blk, DefragAgg* all) {
    std::vector<DefragAgg> base;
    DefragAgg carry = defrag_none();
    for (size_t b = 0; b < f.size(); b += blk) {
        base.push_back(carry);
        DefragAgg run = defrag_none();
        for (size_t j = b; j < b + blk && j < f.size(); ++j) run = defrag_join(run, defrag_elem(f[j].body, f[j].last));
        carry = defrag_join(carry, run);
    }
    *all = carry;
    std::vector<Rec> recs;
    for (size_t b = 0; b < f.size(); b += blk) {
        DefragAgg s = base[b / blk];
        for (size_t j = b; j < b + blk && j < f.size(); ++j) {
            if (f[j].last) {
                EXPECT(s.lasts, recs.size());
                recs.push_back(Rec{j - s.cnt, s.tail + f[j].body, s.cnt != 0});
            }
            s = defrag_join(s, defrag_elem(f[j].body, f[j].last));
        }
    }
    return recs;
}

int main() {
    const uint64_t kMax = ~uint64_t(0);
    const uint64_t k31 = uint64_t(1) << 31;
    // a record's status, length and mark around the 2^31 limit (rpc_message.rs:146-151)
    EXPECT(defrag_status(0), ONC_OK);
    EXPECT(defrag_len(0), 4);
    EXPECT(defrag_mark(0), 0x80000000u);
    EXPECT(defrag_status(k31 - 1), ONC_OK);
    EXPECT(defrag_len(k31 - 1), 0x80000003u);
    EXPECT(defrag_mark(k31 - 1), 0xFFFFFFFFu);
    EXPECT(defrag_status(k31), ONC_ENC_TOO_LONG);
    EXPECT(defrag_len(k31), 0);
    EXPECT(defrag_status(kMax), ONC_ENC_TOO_LONG);
    EXPECT(defrag_len(kMax), 0);
    EXPECT(defrag_body(100, 104), 0);
    EXPECT(defrag_body(kMax - 9, kMax), 5);
    // capacity: no sum is formed
    EXPECT(defrag_fits(0, 4, 0), 0);
    EXPECT(defrag_fits(0, 0, 0), 1);
    EXPECT(defrag_fits(0, 4, 4), 1);
    EXPECT(defrag_fits(0, 4, 3), 0);
    EXPECT(defrag_fits(96, 4, 100), 1);
    EXPECT(defrag_fits(97, 4, 100), 0);
    EXPECT(defrag_fits(100, 0, 100), 1);
    EXPECT(defrag_fits(101, 0, 100), 0);
    EXPECT(defrag_fits(kMax - 3, 8, kMax), 0);       // off + len wraps to 4
    EXPECT(defrag_fits(kMax - 3, 3, kMax), 1);
    EXPECT(defrag_fits(kMax, 0x80000003u, 100), 0);
    EXPECT(defrag_fits(8, kMax, kMax), 0);
    EXPECT(defrag_fits(0, kMax, kMax), 1);

    // the plan over fragments, at every blocking
    const std::vector<Frag> f = {
        {10, false}, {0, false}, {5, true},            // 3 fragments, 15 bytes
        {7, true},                                     // single
        {0, false}, {0, false}, {0, true},             // only empty fragments: the bare mark
        {0, true},                                     // an empty single
        {k31 - 1, true},                               // the largest record
        {k31 - 1, false}, {1, true},                   // 2^31: too long
        {k31 - 1, false}, {k31 - 1, false}, {k31 - 1, false}, {3, true},   // far beyond
        {9, false}, {2, false},                        // pending
    };
    const uint64_t wantB[] = {15, 7, 0, 0, k31 - 1, k31, 3 * (k31 - 1) + 3};
    const uint64_t wantFirst[] = {0, 3, 4, 7, 8, 9, 11};
    const bool wantMulti[] = {true, false, true, false, false, true, true};
    for (size_t blk = 1; blk <= f.size() + 1; ++blk) {
        DefragAgg all;
        const std::vector<Rec> recs = plan(f, blk, &all);
        EXPECT(recs.size(), 7);
        EXPECT(all.lasts, 7);
        EXPECT(all.cnt, 2);       // pending fragments
        EXPECT(all.tail, 11);     // and their body bytes
        uint64_t off = 0;
        for (size_t r = 0; r < recs.size() && r < 7; ++r) {
            EXPECT(recs[r].B, wantB[r]);
            EXPECT(recs[r].first, wantFirst[r]);
            EXPECT(recs[r].multi, wantMulti[r]);
            off += defrag_len(recs[r].B);
        }
        // placement: the two records past the limit take nothing
        EXPECT(off, 19 + 11 + 4 + 4 + (k31 + 3));
        EXPECT(defrag_status(recs[5].B), ONC_ENC_TOO_LONG);
        EXPECT(defrag_status(recs[6].B), ONC_ENC_TOO_LONG);
        EXPECT(defrag_status(recs[4].B), ONC_OK);
        EXPECT(defrag_len(recs[2].B), 4);
    }
    // the join is associative where it matters: sums near 2^64 wrap the same
    // way in any grouping (unsigned arithmetic, no undefined behaviour)
    const DefragAgg a = defrag_elem(kMax - 5, false), b = defrag_elem(4, false), c = defrag_elem(9, false);
    const DefragAgg l = defrag_join(defrag_join(a, b), c), r = defrag_join(a, defrag_join(b, c));
    EXPECT(l.tail, r.tail);
    EXPECT(l.tail, 7);
    EXPECT(l.cnt, 3);
    EXPECT(defrag_status(defrag_join(a, b).tail), ONC_ENC_TOO_LONG);
    const DefragAgg z = defrag_join(defrag_join(a, defrag_elem(1, true)), c);
    EXPECT(z.tail, 9);
    EXPECT(z.lasts, 1);
    EXPECT(z.cnt, 1);
    // placement sums near 2^64 against the capacity
    EXPECT(defrag_fits(kMax - 0x80000003ull, 0x80000003u, kMax), 1);
    EXPECT(defrag_fits(kMax - 0x80000002ull, 0x80000003u, kMax), 0);
    if (g_fail) return 1;
    std::printf("defrag plan ok\n");
    return 0;
}
