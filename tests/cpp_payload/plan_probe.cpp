// plan_probe.cpp — the arithmetic of onc_payload_slots / onc_place_payloads
// (onc-rpc_amd/csrc/payload_plan.h) on the CPU: compiled with the host compiler
// (and -fsanitize=undefined where the toolchain has it) and run by
// tests/test_payload_host.py. The kernels call the same functions. Checked:
// which slices may be copied at the mark, at the record's end and where
// pay_pos + pay_len wraps 2^32; which slots fit at the destination's end and
// where slot_off + pay_len wraps 2^64; round_up at every power of two up to
// 2^20; which descriptors have a payload; the scan of {slot bytes, records,
// payload bytes} at every blocking of a short list against the loop in
// include/onc_rpc.h; and heads_frag_of over empty fragments.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "defrag_heads_plan.h"
#include "payload_plan.h"

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
constexpr uint32_t kMax32 = 0xFFFFFFFFu;

static void check_ok() {
    // behind the mark
    EXPECT(payload_ok(3, 1, 100, 0, 1000), false);
    EXPECT(payload_ok(0, 1, 100, 0, 1000), false);
    EXPECT(payload_ok(4, 1, 100, 0, 1000), true);
    EXPECT(payload_ok(4, 96, 100, 0, 1000), true);
    EXPECT(payload_ok(4, 97, 100, 0, 1000), false);
    // pay_pos = rec_len: the empty slice at the record's end, and nothing longer
    EXPECT(payload_ok(100, 0, 100, 0, 1000), true);
    EXPECT(payload_ok(100, 1, 100, 0, 1000), false);
    EXPECT(payload_ok(101, 0, 100, 0, 1000), false);
    EXPECT(payload_ok(99, 1, 100, 0, 1000), true);
    EXPECT(payload_ok(99, 2, 100, 0, 1000), false);
    // pay_pos + pay_len wraps 2^32 to a position inside the record, were the sum formed
    EXPECT(payload_ok(kMax32, 2, kMax32, 0, kMax), false);
    EXPECT(payload_ok(kMax32 - 5, 10, kMax32, 0, kMax), false);
    EXPECT(payload_ok(0x80000000u, 0x80000004u, 0x90000000u, 0, kMax), false);
    EXPECT(payload_ok(kMax32 - 5, 5, kMax32, 0, kMax), true);
    EXPECT(payload_ok(4, kMax32 - 4, kMax32, 0, kMax), true);
    // a record of length 0 (ONC_ENC_TOO_LONG)
    EXPECT(payload_ok(4, 1, 0, 0, 1000), false);
    EXPECT(payload_ok(4, 0, 0, 0, 1000), false);
    // slot_off = dst_cap: the empty slot at the destination's end
    EXPECT(payload_ok(4, 0, 100, 1000, 1000), true);
    EXPECT(payload_ok(4, 1, 100, 1000, 1000), false);
    EXPECT(payload_ok(4, 0, 100, 1001, 1000), false);
    EXPECT(payload_ok(4, 10, 100, 990, 1000), true);
    EXPECT(payload_ok(4, 11, 100, 990, 1000), false);
    EXPECT(payload_ok(4, 1, 100, 0, 0), false);
    // slot_off + pay_len wraps 2^64
    EXPECT(payload_ok(4, 2, 100, kMax, kMax), false);
    EXPECT(payload_ok(4, 2, 100, kMax - 1, kMax), false);
    EXPECT(payload_ok(4, 1, 100, kMax - 1, kMax), true);
    EXPECT(payload_ok(4, 96, 100, kMax - 50, kMax - 1), false);
    EXPECT(payload_ok(4, 96, 100, (1ull << 32) - 48, 1ull << 33), true);
}

static void check_round_up() {
    for (uint32_t s = 0; s <= 20; ++s) {
        const uint32_t a = 1u << s;
        EXPECT(payload_align_ok(a), true);
        EXPECT(payload_round_up(0, a), 0);
        EXPECT(payload_round_up(1, a), a);
        EXPECT(payload_round_up(a, a), a);
        EXPECT(payload_round_up(a + 1, a), a == 1 ? 2ull : 2ull * a);
        EXPECT(payload_round_up(a - 1, a), a == 1 ? 0ull : a);
        EXPECT(payload_round_up(kMax32, a), a == 1 ? uint64_t(kMax32) : 1ull << 32);   // not wrapped to 0
        EXPECT(payload_round_up(kMax32 - a + 1, a), uint64_t(kMax32) - a + 1);
        if (s) EXPECT(payload_align_ok(a + 1), false);
        if (s > 1) EXPECT(payload_align_ok(a - 1), false);
    }
    EXPECT(payload_align_ok(0), false);
    EXPECT(payload_align_ok(3), false);
    EXPECT(payload_align_ok(1u << 21), false);
    EXPECT(payload_align_ok(0x80000000u), false);
    EXPECT(payload_align_ok((1u << 20) + (1u << 19)), false);
}

static void check_has() {
    EXPECT(payload_has(ONC_OK, ONC_MSG_CALL, 0, 0, 5), true);
    EXPECT(payload_has(ONC_OK, ONC_MSG_CALL, 1, 3, 5), true);                 // (a Call's reply words are not read)
    EXPECT(payload_has(ONC_OK, ONC_MSG_CALL, 0, 0, 0), false);
    EXPECT(payload_has(ONC_ERR_INVALID_LENGTH, ONC_MSG_CALL, 0, 0, 5), false);
    EXPECT(payload_has(ONC_DEC_BAD_EXTENT, ONC_MSG_REPLY, ONC_REPLY_ACCEPTED, ONC_ACCEPT_SUCCESS, 5), false);
    EXPECT(payload_has(ONC_OK, ONC_MSG_REPLY, ONC_REPLY_ACCEPTED, ONC_ACCEPT_SUCCESS, 5), true);
    EXPECT(payload_has(ONC_OK, ONC_MSG_REPLY, ONC_REPLY_ACCEPTED, ONC_ACCEPT_PROG_MISMATCH, 5), false);
    EXPECT(payload_has(ONC_OK, ONC_MSG_REPLY, ONC_REPLY_ACCEPTED, ONC_ACCEPT_SYSTEM_ERR, 5), false);
    EXPECT(payload_has(ONC_OK, ONC_MSG_REPLY, ONC_REPLY_DENIED, 0, 5), false);
    EXPECT(payload_has(ONC_OK, 2, 0, 0, 5), false);
}

static void check_extent() {
    EXPECT(payload_extent(100, 20, 1000), 120);
    EXPECT(payload_extent(990, 10, 1000), 1000);
    EXPECT(payload_extent(990, 11, 1000), 1000);
    EXPECT(payload_extent(1000, 5, 1000), 1000);
    EXPECT(payload_extent(kMax, kMax32, 1000), 1000);
    EXPECT(payload_extent(kMax - 1, kMax32, kMax), kMax);
    EXPECT(payload_extent(0, 0, 1000), 0);
}

// heads_frag_of: the last fragment starting at or before a byte holds it.
static void check_frag_of() {
    // bodies 3, 0, 0, 2, 0, 4 from fragment 10 on
    std::vector<uint64_t> pre(16, 99);
    const uint64_t p[6] = {0, 3, 3, 3, 5, 5};
    for (int i = 0; i < 6; ++i) pre[10 + i] = p[i];
    const uint64_t want[9] = {10, 10, 10, 13, 13, 15, 15, 15, 15};
    for (uint64_t x = 0; x < 9; ++x) EXPECT(heads_frag_of(pre.data(), 10, 16, x), want[x]);
    EXPECT(heads_frag_of(pre.data(), 10, 11, 2), 10);
}

// The loop of include/onc_rpc.h over {has, payload_len}.
struct Rec {
    bool has;
    uint32_t len;
};
static void check_scan(const std::vector<Rec>& p, uint32_t align) {
    const size_t n = p.size();
    std::vector<uint64_t> want;
    uint64_t off = 0, k = 0, bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        want.push_back(off);
        const uint32_t len = p[i].has ? p[i].len : 0;
        off += (uint64_t(len) + align - 1) / align * align;
        k += p[i].has;
        bytes += len;
    }
    auto elem = [&](size_t i) { return payload_elem(p[i].has, p[i].len, align); };
    for (uint32_t cuts = 0; cuts < (1u << (n ? n - 1 : 0)); ++cuts) {
        std::vector<size_t> start{0};
        for (size_t i = 1; i < n; ++i)
            if (cuts >> (i - 1) & 1) start.push_back(i);
        start.push_back(n);
        std::vector<PayAgg> blk;
        for (size_t b = 0; b + 1 < start.size(); ++b) {
            PayAgg s = payload_none();
            for (size_t i = start[b]; i < start[b + 1]; ++i) s = payload_join(s, elem(i));
            blk.push_back(s);
        }
        PayAgg carry = payload_none();
        for (size_t b = 0; b < blk.size(); ++b) {
            PayAgg ex = carry;
            for (size_t i = start[b]; i < start[b + 1]; ++i) {
                EXPECT(ex.off, want[i]);
                ex = payload_join(ex, elem(i));
            }
            carry = payload_join(carry, blk[b]);
            EXPECT(ex.off, carry.off);
        }
        uint64_t res[3];
        payload_result(res, carry);
        EXPECT(res[0], k);
        EXPECT(res[1], bytes);
        EXPECT(res[2], off);
    }
}

int main() {
    check_ok();
    check_round_up();
    check_has();
    check_extent();
    check_frag_of();
    const std::vector<Rec> a = {{true, 1}, {false, 77}, {true, 16}, {true, 17}, {true, kMax32}, {false, 0},
                                {true, 4095}, {true, 4096}, {true, 4097}, {true, kMax32}, {true, 15}};
    for (uint32_t align : {1u, 16u, 4096u, 1u << 20}) {
        check_scan(a, align);
        check_scan({}, align);
        check_scan({{false, 9}}, align);
        check_scan({{true, 9}}, align);
    }
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("payload plan ok\n");
    return 0;
}
