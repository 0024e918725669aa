// plan_probe.cpp — the arithmetic of onc_piece_offsets / onc_gather_pieces
// (onc-rpc_amd/csrc/gather_plan.h) on the CPU: compiled with the host compiler
// (and -fsanitize=undefined where the toolchain has it) and run by
// tests/test_gather_host.py. The kernels call the same functions. Checked:
// which pieces may be read at offsets and lengths near 2^64 (no sum wraps), at
// a source's end and at a source index past the last; what is left of a
// window whose end wraps past 2^64 or that starts at the stream's end; and the
// scan of {bytes, bad pieces, first bad piece} at every blocking of a short
// list against the loop in include/onc_rpc.h.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gather_plan.h"

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

constexpr uint64_t kMax = ~0ull;

struct Piece {
    uint64_t off;
    uint32_t len, src;
};

static void check_ok() {
    const uint64_t L0 = 48, L1 = 0, L2 = 1;
    auto ok = [&](uint64_t off, uint32_t len, uint32_t src) { return gather_ok(off, len, src, L0, L1, L2); };
    // off + len wraps to 1: inside every source, were the sum formed
    EXPECT(ok(kMax, 2, 0), false);
    EXPECT(ok(kMax, 2, 2), false);
    EXPECT(ok(kMax - 5, 0xFFFFFFFFu, 0), false);
    EXPECT(ok(kMax, 1, 0), false);
    // off = the source's length: the empty slice at its end, and nothing longer
    EXPECT(ok(L0, 0, 0), true);
    EXPECT(ok(L0, 1, 0), false);
    EXPECT(ok(L2, 0, 2), true);
    EXPECT(ok(L2, 1, 2), false);
    EXPECT(ok(L2 + 1, 1, 2), false);
    EXPECT(ok(0, 0, 1), true);
    EXPECT(ok(0, 1, 1), false);           // a source of no bytes
    // inside
    EXPECT(ok(0, 48, 0), true);
    EXPECT(ok(0, 49, 0), false);
    EXPECT(ok(47, 1, 0), true);
    EXPECT(ok(47, 2, 0), false);
    EXPECT(ok(0, 1, 2), true);
    // a source past the last: bad unless the piece is empty
    EXPECT(ok(0, 1, 3), false);
    EXPECT(ok(0, 1, 0xFFFFFFFFu), false);
    EXPECT(ok(0, 0, 3), true);
    EXPECT(ok(kMax, 0, 0xFFFFFFFFu), true);
    // a source as long as the address space
    EXPECT(gather_ok(kMax - 1, 1, 2, 0, 0, kMax), true);
    EXPECT(gather_ok(kMax - 1, 2, 2, 0, 0, kMax), false);
    EXPECT(gather_ok(kMax, 0, 2, 0, 0, kMax), true);
}

static void check_window() {
    // from + count wraps past 2^64
    EXPECT(gather_window(kMax - 9, 100, kMax), 9);
    EXPECT(gather_window(kMax - 9, kMax, kMax), 9);
    EXPECT(gather_window(10, kMax, 1000), 990);
    EXPECT(gather_window(1, kMax, kMax), kMax - 1);
    EXPECT(gather_window(kMax, kMax, kMax), 0);
    // from = the stream's end, and past it
    EXPECT(gather_window(1000, 16, 1000), 0);
    EXPECT(gather_window(1001, 16, 1000), 0);
    EXPECT(gather_window(0, 16, 0), 0);
    EXPECT(gather_window(999, 16, 1000), 1);
    // inside, and nothing asked for
    EXPECT(gather_window(0, 1000, 1000), 1000);
    EXPECT(gather_window(0, 1001, 1000), 1000);
    EXPECT(gather_window(5, 10, 1000), 10);
    EXPECT(gather_window(5, 0, 1000), 0);
    EXPECT(gather_window((1ull << 32) - 5, 10, (1ull << 33)), 10);
}

// The loop of include/onc_rpc.h.
struct Offsets {
    std::vector<uint64_t> pos;
    uint64_t total, bad, first_bad;
};
static Offsets reference(const std::vector<Piece>& p, const uint64_t len[3]) {
    Offsets r{{}, 0, 0, p.size()};
    for (size_t i = 0; i < p.size(); ++i) {
        r.pos.push_back(r.total);
        if (!gather_ok(p[i].off, p[i].len, p[i].src, len[0], len[1], len[2])) {
            ++r.bad;
            if (i < r.first_bad) r.first_bad = i;
        }
        r.total += p[i].len;
    }
    r.pos.push_back(r.total);
    return r;
}

// The kernels' scan with the list cut into blocks at the set bits of `cuts`:
// block sums, their exclusive scan, then every element from its block's base.
static void check_scan(const std::vector<Piece>& p, const uint64_t len[3]) {
    const Offsets want = reference(p, len);
    const size_t n = p.size();
    auto elem = [&](size_t i) {
        return gather_elem(i, p[i].len, gather_ok(p[i].off, p[i].len, p[i].src, len[0], len[1], len[2]));
    };
    for (uint32_t cuts = 0; cuts < (1u << (n ? n - 1 : 0)); ++cuts) {
        std::vector<size_t> start{0};
        for (size_t i = 1; i < n; ++i)
            if (cuts >> (i - 1) & 1) start.push_back(i);
        start.push_back(n);
        std::vector<GatherAgg> blk;
        for (size_t b = 0; b + 1 < start.size(); ++b) {
            GatherAgg s = gather_none();
            for (size_t i = start[b]; i < start[b + 1]; ++i) s = gather_join(s, elem(i));
            blk.push_back(s);
        }
        GatherAgg carry = gather_none();
        for (size_t b = 0; b < blk.size(); ++b) {
            GatherAgg ex = carry;
            for (size_t i = start[b]; i < start[b + 1]; ++i) {
                EXPECT(ex.bytes, want.pos[i]);
                ex = gather_join(ex, elem(i));
            }
            carry = gather_join(carry, blk[b]);
            EXPECT(ex.bytes, carry.bytes);
        }
        EXPECT(carry.bytes, want.total);
        EXPECT(carry.bad, want.bad);
        EXPECT(carry.first_bad < n ? carry.first_bad : n, want.first_bad);
    }
}

int main() {
    check_ok();
    check_window();
    const uint64_t len[3] = {48, 300, 1};
    // empty pieces, bad pieces first, last and in the middle, lengths up to 2^32 - 1
    const std::vector<Piece> a = {{0, 4, 0}, {kMax, 0, 1}, {10, 290, 1}, {5, 9, 3}, {0, 1, 2}, {2, 1, 2},
                                  {0, 0, 7}, {kMax, 2, 0}, {44, 4, 0}, {0, 0xFFFFFFFFu, 1}, {0, 0xFFFFFFFFu, 1}, {7, 7, 1}};
    const std::vector<Piece> b = {{5, 9, 3}, {0, 4, 0}, {0, 0, 0}, {0, 0, 0}, {1, 4, 0}};
    const std::vector<Piece> c = {{0, 4, 0}, {8, 30, 1}, {0, 1, 2}, {0, 0, 2}, {299, 2, 1}};
    const std::vector<Piece> d = {{0, 4, 0}, {8, 30, 1}, {0, 1, 2}};
    check_scan(a, len);
    check_scan(b, len);
    check_scan(c, len);
    check_scan(d, len);
    check_scan({}, len);
    check_scan({{0, 0, 9}}, len);
    check_scan({{0, 1, 9}}, len);
    EXPECT(reference(a, len).bad, 5);
    EXPECT(reference(a, len).first_bad, 3);
    EXPECT(reference(a, len).total, 4ull + 290 + 9 + 1 + 1 + 2 + 4 + 2 * 0xFFFFFFFFull + 7);
    EXPECT(reference(d, len).first_bad, 3);
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("gather plan ok\n");
    return 0;
}
