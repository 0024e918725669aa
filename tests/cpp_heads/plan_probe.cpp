// plan_probe.cpp — the host arithmetic of onc_defragment_heads
// (onc-rpc_amd/csrc/defrag_heads_plan.h) driven by a host program up to sizes
// no buffer has (the GPU tests stop at 4.4 GB): the serial loop of include/onc_rpc.h run with that
// arithmetic over fragment lists built here — ONC_ENC_TOO_LONG at B = 2^31 - 1
// / 2^31, the capacity cut, the result words, the head_len rule — and the
// fragment search against a brute-force walk, with runs of empty fragments.
// Stand-alone (its own main): tests/test_heads_host.py builds it with the
// host compiler, with sanitizers where the toolchain links them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "defrag_heads_plan.h"

using namespace onc;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #cond);  \
            return 1;                                                            \
        }                                                                        \
    } while (0)

struct Frag {
    uint64_t body;
    bool last;
};
struct Plan {
    std::vector<uint32_t> rec_len;
    std::vector<int32_t> status;
    std::vector<uint64_t> rec_frag, frag_pre;
    uint64_t result[6];
};

// The header's loop, its arithmetic taken from defrag_heads_plan.h (bodies are
// 64 bits wide here: a probe may add up more than a real fragment can hold).
static Plan serial(const std::vector<Frag>& f, uint64_t max_records, uint32_t head_len) {
    Plan p;
    uint64_t r = 0, first = 0, B = 0, multi = 0;
    for (uint64_t j = 0; j < f.size(); ++j) {
        p.frag_pre.push_back(B);
        B += f[j].body;
        if (f[j].last) {
            p.rec_frag.push_back(first);
            p.rec_len.push_back(heads_rec_len(B));
            p.status.push_back(heads_status(B, r, max_records));
            multi += j > first;
            ++r;
            first = j + 1;
            B = 0;
        }
    }
    p.rec_frag.push_back(first);
    heads_result(p.result, r, f.size(), f.size() - first, B, multi, head_len);
    return p;
}

// The same through the scan the device runs (defrag_plan.h), at one blocking.
static Plan scanned(const std::vector<Frag>& f, uint64_t max_records, uint32_t head_len, size_t block) {
    Plan p;
    p.frag_pre.resize(f.size());
    DefragAgg carry = defrag_none();
    uint64_t multi = 0;
    std::vector<uint32_t> lens(f.size(), 0);
    std::vector<uint64_t> first_of(f.size() + 1, 0);
    for (size_t b0 = 0; b0 < f.size(); b0 += block) {
        DefragAgg run = defrag_none();
        for (size_t j = b0; j < f.size() && j < b0 + block; ++j) {
            const DefragAgg ex = defrag_join(carry, run);
            p.frag_pre[j] = ex.tail;
            if (ex.cnt == 0) first_of[ex.lasts] = j;
            if (f[j].last) {
                lens[ex.lasts] = heads_rec_len(ex.tail + f[j].body);
                multi += ex.cnt != 0;
            }
            run = defrag_join(run, defrag_elem(f[j].body, f[j].last));
        }
        carry = defrag_join(carry, run);
    }
    const uint64_t nrec = carry.lasts;
    for (uint64_t r = 0; r < nrec; ++r) {
        p.rec_len.push_back(lens[r]);
        p.status.push_back(heads_status_len(lens[r], r, max_records));
        p.rec_frag.push_back(first_of[r]);
    }
    p.rec_frag.push_back(f.size() - carry.cnt);
    heads_result(p.result, nrec, f.size(), carry.cnt, carry.tail, multi, head_len);
    return p;
}

static bool same(const Plan& a, const Plan& b) {
    for (int k = 0; k < 6; ++k)
        if (a.result[k] != b.result[k]) return false;
    return a.rec_len == b.rec_len && a.status == b.status && a.rec_frag == b.rec_frag && a.frag_pre == b.frag_pre;
}

int main() {
    // head_len: a multiple of 16 in [64, 4096]
    for (uint32_t h = 0; h <= 4200; ++h) CHECK(heads_len_ok(h) == (h >= 64 && h <= 4096 && h % 16 == 0));
    CHECK(!heads_len_ok(0xFFFFFFF0u) && !heads_len_ok(0x80000040u));

    // TOO_LONG at B = 2^31: a record of two fragments adding up to it
    const uint64_t kMax = 0x7FFFFFFFull;
    CHECK(heads_rec_len(kMax) == 0x80000003u && heads_status(kMax, 0, 1) == ONC_OK);
    CHECK(heads_rec_len(kMax + 1) == 0 && heads_status(kMax + 1, 0, 1) == ONC_ENC_TOO_LONG);
    CHECK(heads_status(kMax + 1, 5, 1) == ONC_ENC_TOO_LONG);            // too long comes before the capacity
    CHECK(heads_status(kMax, 1, 1) == ONC_ENC_WRITE_ZERO && heads_status(0, 0, 0) == ONC_ENC_WRITE_ZERO);
    CHECK(heads_status_len(0, 0, 9) == ONC_ENC_TOO_LONG && heads_status_len(4, 8, 9) == ONC_OK &&
          heads_status_len(4, 9, 9) == ONC_ENC_WRITE_ZERO);
    CHECK(defrag_mark(kMax) == 0xFFFFFFFFu && defrag_mark(0) == 0x80000000u);
    CHECK(heads_present(4, 64) == 4 && heads_present(64, 64) == 64 && heads_present(0x80000003u, 4096) == 4096 &&
          heads_present(0, 64) == 0);
    {
        // records: B = 2^31 - 1 in two fragments, B = 2^31 in three, B = 0,
        // then a pending run of two
        const std::vector<Frag> f = {{kMax - 7, false}, {7, true}, {kMax - 1, false}, {0, false}, {2, true},
                                     {0, true},         {9, false}, {3, false}};
        for (uint64_t cap = 0; cap <= 4; ++cap) {
            const Plan p = serial(f, cap, 160);
            CHECK(p.rec_len == (std::vector<uint32_t>{0x80000003u, 0u, 4u}));
            CHECK(p.status[0] == (cap > 0 ? ONC_OK : ONC_ENC_WRITE_ZERO));
            CHECK(p.status[1] == ONC_ENC_TOO_LONG);
            CHECK(p.status[2] == (cap > 2 ? ONC_OK : ONC_ENC_WRITE_ZERO));
            CHECK(p.rec_frag == (std::vector<uint64_t>{0, 2, 5, 6}));
            CHECK(p.frag_pre == (std::vector<uint64_t>{0, kMax - 7, 0, kMax - 1, kMax - 1, 0, 0, 9}));
            const uint64_t want[6] = {3, 6, 3 * 160, 2, 12, 2};
            for (int k = 0; k < 6; ++k) CHECK(p.result[k] == want[k]);
            for (size_t block = 1; block <= f.size() + 1; ++block) CHECK(same(p, scanned(f, cap, 160, block)));
        }
    }
    {
        // no fragments; pending fragments only
        const Plan e = serial({}, 3, 64);
        CHECK(e.rec_frag == std::vector<uint64_t>{0} && e.rec_len.empty());
        for (int k = 0; k < 6; ++k) CHECK(e.result[k] == 0);
        const std::vector<Frag> f = {{5, false}, {0, false}};
        const Plan p = serial(f, 3, 4096);
        const uint64_t want[6] = {0, 0, 0, 2, 5, 0};
        for (int k = 0; k < 6; ++k) CHECK(p.result[k] == want[k]);
        CHECK(p.rec_frag == std::vector<uint64_t>{0} && p.frag_pre == (std::vector<uint64_t>{0, 5}));
        CHECK(same(p, scanned(f, 3, 4096, 1)) && same(p, scanned(f, 3, 4096, 256)));
    }
    {
        // a pseudo-random list, every blocking, the heads capacity at 4096
        std::vector<Frag> f;
        uint32_t x = 12345;
        for (int i = 0; i < 700; ++i) {
            x = x * 1664525u + 1013904223u;
            const uint32_t k = (x >> 8) % 6;
            f.push_back(Frag{k == 0 ? 0u : k == 1 ? 1u : k == 2 ? 3u : k == 3 ? 40u : (x >> 20), ((x >> 4) & 3) == 0});
        }
        const Plan p = serial(f, 100, 4096);
        CHECK(p.result[2] == p.result[0] * 4096 && p.result[0] + 0 == p.rec_len.size());
        for (size_t block : {size_t(1), size_t(2), size_t(7), size_t(64), size_t(256), size_t(699), size_t(1000)})
            CHECK(same(p, scanned(f, 100, 4096, block)));
        // the fragment search against a walk: every body byte of every record
        // up to 4096, runs of empty fragments included
        for (size_t r = 0; r + 1 < p.rec_frag.size(); ++r) {
            const uint64_t lo = p.rec_frag[r], hi = p.rec_frag[r + 1];
            uint64_t xb = 0;
            for (uint64_t j = lo; j < hi; ++j)
                for (uint64_t o = 0; o < f[j].body && xb < 4096; ++o, ++xb) {
                    CHECK(heads_frag_of(p.frag_pre.data(), lo, hi, xb) == j);
                    CHECK(xb - p.frag_pre[j] == o);
                }
        }
    }
    {
        // 200 empty fragments, then 1-byte fragments, then a long one
        std::vector<Frag> f(200, Frag{0, false});
        for (int i = 0; i < 50; ++i) f.push_back(Frag{1, false});
        for (int i = 0; i < 3; ++i) f.push_back(Frag{0, false});
        f.push_back(Frag{1000, true});
        const Plan p = serial(f, 1, 160);
        CHECK(p.rec_len[0] == 4 + 50 + 1000 && p.result[5] == 1);
        for (uint64_t xb = 0; xb < 50; ++xb) CHECK(heads_frag_of(p.frag_pre.data(), 0, f.size(), xb) == 200 + xb);
        for (uint64_t xb = 50; xb < 1050; xb += 37) CHECK(heads_frag_of(p.frag_pre.data(), 0, f.size(), xb) == 253);
        // a record of one fragment: nothing to search
        const uint64_t pre1[1] = {0};
        CHECK(heads_frag_of(pre1, 0, 1, 0) == 0 && heads_frag_of(pre1, 0, 1, 4000) == 0);
    }
    std::printf("defrag heads plan ok\n");
    return 0;
}
