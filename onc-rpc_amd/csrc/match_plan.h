// match_plan.h — the arithmetic of onc_match_replies (match.hip): the slot
// count of the hash table over a pending list (match_slots), the hash of a
// (conn, xid) key and the slot a probe tries next (match_hash, match_next),
// where the table, first_rec and the tiles' counts lie in the scratch
// (MatchLayout, match_layout) and how many u32 words that is
// (match_scratch_words), and a record's class (match_class). The slot count
// reaches 2^33 and every word offset is formed in 64 bits. Plain C++ without
// HIP headers, as route_plan.h: tests/cpp_match/plan_probe.cpp drives it on
// the host.
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "partition_plan.h"

namespace onc {

constexpr uint32_t kMatchTile = 1024;          // records / entries per tile (= threads per workgroup)
constexpr uint32_t kMatchEmpty = 0xFFFFFFFFu;  // an empty slot; a first_rec nobody has lowered (= ONC_MATCH_NONE)
constexpr uint64_t kMatchSlotsMin = 16;        // so that S - 2 is a slot, and the clear's 16-byte stores cover whole slots
constexpr uint32_t kMatchClasses = 5;          // matched, unknown, duplicate, not_reply, failed: result's order

// Slots: the least power of two >= 2 np (at most half of them are ever
// taken, so every probe chain ends at an empty slot), and >= the floor.
ONC_HD inline uint64_t match_slots(uint64_t np) {
    uint64_t s = kMatchSlotsMin;
    while (s < 2 * np) s <<= 1;                 // np < 2^32: no wrap
    return s;
}

// The slot a key's chain starts at. Both words go through the 64-bit
// finaliser of MurmurHash3 (two multiply / xor-shift rounds: every input bit
// reaches every output bit), so that xids counting up on connections counting
// up — the keys a client really has — spread like random ones; the low bits
// index the table. ONC_VARIANT_MATCH_ONE_CHAIN: every key starts at S - 2.
ONC_HD inline uint64_t match_hash(uint32_t conn, uint32_t xid, uint64_t slots, uint32_t variant) {
    if (variant & ONC_VARIANT_MATCH_ONE_CHAIN) return slots - 2;
    uint64_t k = (uint64_t(conn) << 32) | uint64_t(xid);
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    k ^= k >> 33;
    return k & (slots - 1);
}
ONC_HD inline uint64_t match_next(uint64_t slot, uint64_t slots) { return (slot + 1) & (slots - 1); }

ONC_HD inline uint64_t match_tiles(uint64_t n) { return tile_count(n, kMatchTile); }

// The scratch in u32 words: the slots, first_rec (np rounded up to four words:
// the clear stores 16 bytes), the record tiles' class counts class-major (at
// bin_count_at from rec_counts), the pending tiles' unanswered counts (scanned
// in place by match_scan).
struct MatchLayout {
    uint64_t slots;         // S
    uint64_t first_rec;     // word offsets
    uint64_t clear_words;   // slots + first_rec: what match_clear fills (a multiple of 4)
    uint64_t rec_counts;
    uint64_t pend_counts;
    uint64_t words;
    uint64_t rtiles, ptiles;
};
ONC_HD inline MatchLayout match_layout(uint64_t n, uint64_t np) {
    MatchLayout l;
    l.slots = match_slots(np);
    l.rtiles = match_tiles(n);
    l.ptiles = match_tiles(np);
    l.first_rec = l.slots;
    l.clear_words = l.slots + ((np + 3) & ~uint64_t(3));
    l.rec_counts = l.clear_words;
    l.pend_counts = l.rec_counts + uint64_t(kMatchClasses) * l.rtiles;
    l.words = l.pend_counts + l.ptiles;
    return l;
}
ONC_HD inline uint64_t match_scratch_words(uint64_t n, uint64_t np) { return match_layout(n, np).words; }

// A record's class before the duplicates are told apart: 0 = an OK Reply (to
// be probed), else its sentinel.
ONC_HD inline uint32_t match_class(int32_t status, uint32_t msg_type) {
    if (status != ONC_OK) return ONC_MATCH_FAILED;
    if (msg_type != ONC_MSG_REPLY) return ONC_MATCH_NOT_REPLY;
    return 0;
}
// The index of a final match[] value in result: 0 matched, 1 unknown, 2
// duplicate, 3 not_reply, 4 failed.
ONC_HD inline uint32_t match_result_class(uint32_t m) { return m < ONC_MATCH_FAILED ? 0u : ONC_MATCH_UNKNOWN - m + 1u; }

}  // namespace onc
