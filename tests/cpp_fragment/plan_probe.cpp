// plan_probe.cpp — the record arithmetic of onc_fragment
// (onc-rpc_amd/csrc/fragment_plan.h) up to sizes no buffer has (the GPU tests
// stop at a 4.4 GB stream, tests/test_gpu_beyond_4gib.py), on the CPU: compiled with the host compiler (and -fsanitize=undefined where the
// toolchain has it) and run by tests/test_fragment_host.py. The kernels call
// the same functions.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fragment_plan.h"

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

// One record: count, length, the first and last marks, the last body length.
static void rec(uint64_t B, uint32_t F, uint64_t k, uint64_t len, uint32_t mark0, uint32_t mark_last) {
    const FragRec r = frag_rec(B + 4, F);
    EXPECT(r.status, ONC_OK);
    EXPECT(r.k, k);
    EXPECT(r.len, len);
    EXPECT(frag_count(B, F), k);
    EXPECT(frag_mark(B, 0, F), mark0);
    EXPECT(frag_mark(B, k - 1, F), mark_last);
    EXPECT(frag_body_len(B, k - 1, F), mark_last & 0x7FFFFFFFu);
    if (k > 1) EXPECT(frag_body_len(B, k - 2, F), F);
    // the first and last positions of the record, and those around the last mark
    const FragAt a0 = frag_at(0, F), aN = frag_at(len - 1, F), aM = frag_at((k - 1) * frag_stride(F), F);
    EXPECT(a0.j, 0);
    EXPECT(a0.r, 0);
    EXPECT(aM.j, k - 1);
    EXPECT(aM.r, 0);
    EXPECT(aN.j, k - 1);
    EXPECT(aN.r, B ? 4 + (mark_last & 0x7FFFFFFFu) - 1 : 3);
    if (B) EXPECT(frag_src(aN, F), B - 1);
    if (len <= 0xFFFFFFFFull) {
        const FragAt b = frag_at32(uint32_t(len - 1), F);
        EXPECT(b.j, aN.j);
        EXPECT(b.r, aN.r);
    }
}

// The position map against a walk over the fragments as the header's loop
// writes them.
static void walk(uint64_t B, uint32_t F) {
    const FragRec r = frag_rec(B + 4, F);
    uint64_t q = 0;
    for (uint64_t j = 0; j < r.k; ++j) {
        const bool last = j == r.k - 1;
        const uint64_t flen = last ? B - j * F : F;
        const uint32_t mark = last ? 0x80000000u | uint32_t(flen) : F;
        for (uint32_t m = 0; m < 4; ++m, ++q) {
            const FragAt a = frag_at(q, F), b = frag_at32(uint32_t(q), F);
            EXPECT(a.j, j);
            EXPECT(a.r, m);
            EXPECT(b.j, j);
            EXPECT(b.r, m);
            EXPECT(frag_is_mark(a), 1);
            EXPECT(frag_mark_byte(frag_mark(B, a.j, F), a.r), uint8_t(mark >> (24 - 8 * m)));
        }
        for (uint64_t o = 0; o < flen; ++o, ++q) {
            const FragAt a = frag_at(q, F), b = frag_at32(uint32_t(q), F);
            EXPECT(a.j, b.j);
            EXPECT(a.r, b.r);
            EXPECT(frag_is_mark(a), 0);
            EXPECT(frag_src(a, F), j * F + o);
            EXPECT(frag_run16(a, B, F), o + 16 <= flen);
        }
    }
    EXPECT(q, r.len);
}

// The plan as the kernels run it: sums of blocks of `blk` records, their
// scan, then the records — any blocking must give what one serial pass gives.
struct Placed {
    uint64_t off;
    int32_t status;
};
static std::vector<Placed> plan(const std::vector<uint64_t>& L, uint32_t F, uint64_t cap, size_t blk, FragAgg* all) {
    std::vector<FragAgg> base;
    FragAgg carry = frag_none();
    for (size_t b = 0; b < L.size(); b += blk) {
        base.push_back(carry);
        FragAgg run = frag_none();
        for (size_t i = b; i < b + blk && i < L.size(); ++i) run = frag_join(run, frag_elem(frag_rec(L[i], F)));
        carry = frag_join(carry, run);
    }
    *all = carry;
    std::vector<Placed> out;
    for (size_t b = 0; b < L.size(); b += blk) {
        FragAgg s = base[b / blk];
        for (size_t i = b; i < b + blk && i < L.size(); ++i) {
            const FragRec r = frag_rec(L[i], F);
            out.push_back(Placed{s.bytes, frag_status(r, s.bytes, cap)});
            s = frag_join(s, frag_elem(r));
        }
    }
    return out;
}

int main() {
    const uint64_t kMax = ~uint64_t(0);
    const uint64_t k31 = uint64_t(1) << 31, k40 = uint64_t(1) << 40;
    const uint32_t kF = kFragMaxBody, kL = 0x80000000u;
    EXPECT(frag_max_ok(0), 0);
    EXPECT(frag_max_ok(1), 1);
    EXPECT(frag_max_ok(kF), 1);
    EXPECT(frag_max_ok(0x80000000u), 0);
    EXPECT(frag_max_ok(0xFFFFFFFFu), 0);
    // bodies around max_frag and its multiples
    for (uint32_t F : {1u, 2u, 5u, 16u, 1000u}) {
        rec(0, F, 1, 4, kL, kL);
        if (F > 1) rec(F - 1, F, 1, F + 3, kL | (F - 1), kL | (F - 1));
        rec(F, F, 1, F + 4, kL | F, kL | F);
        rec(F + 1, F, 2, F + 9, F, kL | 1);
        rec(2 * F, F, 2, 2 * F + 8, F, kL | F);
    }
    // the limits of the mark and beyond, at the smallest and the largest max_frag
    rec(k31 - 1, kF, 1, k31 + 3, 0xFFFFFFFFu, 0xFFFFFFFFu);
    rec(k31, kF, 2, k31 + 8, kF, kL | 1);
    rec(k40, kF, 513, k40 + 4 * 513, kF, kL | 512);          // 2^40 = 512 (2^31 - 1) + 512
    rec(k31 - 1, 1, k31 - 1, 5 * (k31 - 1), 1, kL | 1);
    rec(k31, 1, k31, 5 * k31, 1, kL | 1);                    // len > 2^32
    rec(k40, 1, k40, 5 * k40, 1, kL | 1);
    // extents that are no records
    EXPECT(frag_rec(0, 7).status, ONC_OK);
    EXPECT(frag_rec(0, 7).len, 0);
    EXPECT(frag_rec(0, 7).k, 0);
    for (uint64_t L : {1, 3}) {
        EXPECT(frag_rec(L, 7).status, ONC_ENC_BAD_DESCRIPTOR);
        EXPECT(frag_rec(L, 7).len, 0);
        EXPECT(frag_rec(L, 7).k, 0);
        EXPECT(frag_status(frag_rec(L, 7), 0, 0), ONC_ENC_BAD_DESCRIPTOR);
        EXPECT(frag_elem(frag_rec(L, 7)).multi, 0);
    }
    EXPECT(frag_rec(4, 7).status, ONC_OK);
    EXPECT(frag_rec(4, 7).len, 4);
    EXPECT(frag_rec(4, 7).k, 1);
    // capacity: no sum is formed
    EXPECT(frag_status(frag_rec(0, 7), 5, 0), ONC_OK);       // nothing to send fits nowhere and everywhere
    EXPECT(frag_status(frag_rec(4, 7), 0, 0), ONC_ENC_WRITE_ZERO);
    EXPECT(frag_status(frag_rec(4, 7), 0, 4), ONC_OK);
    EXPECT(frag_status(frag_rec(4, 7), 1, 4), ONC_ENC_WRITE_ZERO);
    EXPECT(frag_fits(0, 0, 0), 1);
    EXPECT(frag_fits(96, 4, 100), 1);
    EXPECT(frag_fits(97, 4, 100), 0);
    EXPECT(frag_fits(101, 0, 100), 0);
    EXPECT(frag_fits(kMax - 3, 8, kMax), 0);                 // off + len wraps to 4
    EXPECT(frag_fits(kMax - 3, 3, kMax), 1);
    EXPECT(frag_fits(8, kMax, kMax), 0);
    EXPECT(frag_fits(0, kMax, kMax), 1);
    EXPECT(frag_status(frag_rec(24, 8), kMax - 35, kMax), ONC_OK);           // 3 fragments: 32 bytes
    EXPECT(frag_status(frag_rec(24, 8), kMax - 30, kMax), ONC_ENC_WRITE_ZERO);
    EXPECT(frag_status(frag_rec(k31 + 4, 1), kMax - 5 * k31 + 1, kMax), ONC_ENC_WRITE_ZERO);
    EXPECT(frag_status(frag_rec(k31 + 4, 1), kMax - 5 * k31, kMax), ONC_OK);

    // the position map, byte by byte
    for (uint32_t F = 1; F <= 20; ++F)
        for (uint64_t B = 0; B <= 70; ++B) walk(B, F);
    walk(5000, 1000);
    walk(4096, 4095);
    // positions beyond 2^32 inside a record
    {
        const FragAt a = frag_at(5 * k31 - 1, 1);
        EXPECT(a.j, k31 - 1);
        EXPECT(a.r, 4);
        EXPECT(frag_src(a, 1), k31 - 1);
        const uint64_t s = frag_stride(kF);                  // 2^31 + 3
        const FragAt b = frag_at(511 * s + 3, kF), c = frag_at(512 * s + 4 + 511, kF);
        EXPECT(b.j, 511);
        EXPECT(b.r, 3);
        EXPECT(c.j, 512);
        EXPECT(frag_src(c, kF), k40 - 1);
        EXPECT(frag_run16(frag_at(512 * s + 4 + 496, kF), k40, kF), 1);
        EXPECT(frag_run16(frag_at(512 * s + 4 + 497, kF), k40, kF), 0);
    }

    // the plan's scan, at every blocking
    const std::vector<uint64_t> L = {0, 4, 3, 24, 1, 0, 104, 4, 2, 12, 5, 0};
    const uint32_t F = 8;
    // out bytes: 0 4 0 32 0 0 152 4 0 12 5 0 (24 -> 20 in 3 fragments; 104 -> 100 in 13; 12 -> 8 in 1)
    const uint64_t wantOff[] = {0, 0, 4, 4, 36, 36, 36, 188, 192, 192, 204, 209};
    for (uint64_t cap : {kMax, uint64_t(209), uint64_t(208), uint64_t(100), uint64_t(36), uint64_t(0)}) {
        for (size_t blk = 1; blk <= L.size() + 1; ++blk) {
            FragAgg all;
            const std::vector<Placed> p = plan(L, F, cap, blk, &all);
            EXPECT(all.bytes, 209);
            EXPECT(all.frags, 1 + 3 + 13 + 1 + 1 + 1);
            EXPECT(all.multi, 2);
            for (size_t i = 0; i < L.size(); ++i) {
                EXPECT(p[i].off, wantOff[i]);
                const FragRec r = frag_rec(L[i], F);
                const int32_t want = L[i] == 0 ? ONC_OK
                                     : L[i] < 4 ? ONC_ENC_BAD_DESCRIPTOR
                                     : wantOff[i] + r.len <= cap ? ONC_OK
                                                                 : ONC_ENC_WRITE_ZERO;
                EXPECT(p[i].status, want);
            }
        }
    }
    // sums near 2^64 wrap the same way in any grouping (unsigned arithmetic)
    const FragAgg a{kMax - 5, 1, 0}, b{4, 2, 1}, c{9, 3, 1};
    const FragAgg l = frag_join(frag_join(a, b), c), r = frag_join(a, frag_join(b, c));
    EXPECT(l.bytes, r.bytes);
    EXPECT(l.bytes, 7);
    EXPECT(l.frags, 6);
    EXPECT(l.multi, 2);
    if (g_fail) return 1;
    std::printf("fragment plan ok\n");
    return 0;
}
