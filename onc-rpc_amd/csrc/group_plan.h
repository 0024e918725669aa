// group_plan.h — the arithmetic of onc_group_by_conn (group.hip): the bits and
// the radix passes a connection count needs (group_bits, group_passes), an
// item's key (group_clamp) and its digit in a pass (group_digit), and the
// scratch layout (group_layout). A pass is a stable partition (partition.h) by
// one 8-bit digit, the least significant first, so `passes` of them sort the
// keys stably. Plain C++ without HIP headers, as route_plan.h:
// tests/cpp_group/plan_probe.cpp drives it on the host.
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "partition_plan.h"

namespace onc {

constexpr uint32_t kGroupTile = 1024;         // items per tile (= threads per workgroup)
constexpr uint32_t kGroupDigitBits = 8;
constexpr uint32_t kGroupDigits = 1u << kGroupDigitBits;
constexpr uint32_t kGroupBoundsGroups = 1024; // workgroups of the bounds kernel at most (a partial count each)

// Bits of the greatest key, nconn itself ("no connection"); bits(0) = 0.
ONC_HD inline uint32_t group_bits(uint32_t nconn) {
    uint32_t b = 0;
    while (b < 32 && (uint64_t(nconn) >> b) != 0) ++b;
    return b;
}
ONC_HD inline uint32_t group_passes(uint32_t nconn) {
    return (group_bits(nconn) + kGroupDigitBits - 1) / kGroupDigitBits;
}
// Connection ids of nconn or more are one group, the last.
ONC_HD inline uint32_t group_clamp(uint32_t conn, uint32_t nconn) { return conn < nconn ? conn : nconn; }
ONC_HD inline uint32_t group_digit(uint32_t key, uint32_t pass) {
    return (key >> (kGroupDigitBits * pass)) & (kGroupDigits - 1);
}

// The scratch, in u32 words from its 16-byte aligned start: the counts (at
// bin_count_at, a digit the bin), a total and a first position per digit, the
// bounds kernel's partial counts, then two (key, index) buffers that the passes
// write in turn — 16 bytes per item and a byte per item of counts.
struct GroupLayout {
    uint64_t counts;        // kGroupDigits * tiles
    uint64_t totals;        // kGroupDigits
    uint64_t first;         // kGroupDigits
    uint64_t partial;       // kGroupBoundsGroups
    uint64_t key[2];        // n each
    uint64_t idx[2];        // n each
    uint64_t words;         // all of it
};
ONC_HD inline GroupLayout group_layout(uint64_t n, uint32_t tile) {
    GroupLayout l{};
    const uint64_t tiles = tile_count(n, tile);
    const uint64_t per = (n + 3) & ~uint64_t(3);     // the buffers stay 16-byte aligned
    l.counts = 0;
    l.totals = l.counts + uint64_t(kGroupDigits) * tiles;
    l.first = l.totals + kGroupDigits;
    l.partial = l.first + kGroupDigits;
    l.key[0] = (l.partial + kGroupBoundsGroups + 3) & ~uint64_t(3);
    l.idx[0] = l.key[0] + per;
    l.key[1] = l.idx[0] + per;
    l.idx[1] = l.key[1] + per;
    l.words = l.idx[1] + per;
    return l;
}
ONC_HD inline uint64_t group_scratch_bytes(uint64_t n, uint32_t tile) { return 4 * group_layout(n, tile).words; }

// Which buffer a pass writes; the pass after it reads that one. The last pass
// writes its keys there too (the bounds kernel searches them) and its indices
// into the caller's order.
ONC_HD inline uint32_t group_pass_dst(uint32_t pass) { return pass & 1u; }

// conn_first[c] in sorted keys: how many are below c. At most 32 steps for
// n < 2^32, whatever the keys are.
template <class Keys>
ONC_HD inline uint64_t group_lower_bound(const Keys& keys, uint64_t n, uint32_t c) {
    uint64_t lo = 0, hi = n;
    for (int step = 0; step < 32; ++step) {
        if (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < c) lo = mid + 1;
            else hi = mid;
        }
    }
    return lo;
}

}  // namespace onc
