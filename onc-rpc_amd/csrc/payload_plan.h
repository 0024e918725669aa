// payload_plan.h — the arithmetic of onc_payload_slots / onc_place_payloads
// (payload.hip): which decoded records carry a payload (payload_has), how a
// payload's slot is rounded (payload_round_up), which slices may be copied
// (payload_ok), the sum the slots are scanned with (PayAgg) and the result
// words. A slice (pay_pos, pay_len) is pay_len bytes from record byte pay_pos
// on, the mark counted (so pay_pos >= 4); its slot is dst[slot_off, slot_off +
// pay_len). No sum of a position and a length is formed anywhere: pay_pos +
// pay_len may wrap near 2^32 and slot_off + pay_len near 2^64. Plain C++
// without HIP headers, as gather_plan.h: tests/cpp_payload/plan_probe.cpp
// drives it on the host. Which fragment holds a body byte is
// defrag_heads_plan.h's heads_frag_of.
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "extent.h"

namespace onc {

constexpr uint32_t kPayAlignMax = 1u << 20;

// align: a power of two in [1, 2^20].
ONC_HD inline bool payload_align_ok(uint32_t align) {
    return align != 0 && align <= kPayAlignMax && (align & (align - 1)) == 0;
}

// len rounded up to a multiple of align (a power of two): up to 2^32.
ONC_HD inline uint64_t payload_round_up(uint32_t len, uint32_t align) {
    const uint64_t a = align;
    return (uint64_t(len) + a - 1) & ~(a - 1);
}

// A decoded record has a payload to place: it decoded OK, the payload is not
// empty, and the message is one of the two kinds that carry one (a Call, a
// Success reply). Any other descriptor's payload words are ignored.
ONC_HD inline bool payload_has(int32_t status, uint32_t msg_type, uint32_t reply_stat, uint32_t stat,
                               uint32_t payload_len) {
    if (status != ONC_OK || payload_len == 0) return false;
    return msg_type == ONC_MSG_CALL ||
           (msg_type == ONC_MSG_REPLY && reply_stat == ONC_REPLY_ACCEPTED && stat == ONC_ACCEPT_SUCCESS);
}

// The slice lies inside its record of rec_len bytes, behind the mark, and its
// slot inside a destination of dst_cap bytes. pay_pos == rec_len is the empty
// slice at the record's end and holds no byte; so does slot_off == dst_cap. (A
// slice of no bytes is skipped before the rule is asked: nothing is copied
// for it wherever it points.)
ONC_HD inline bool payload_ok(uint32_t pay_pos, uint32_t pay_len, uint32_t rec_len, uint64_t slot_off,
                              uint64_t dst_cap) {
    if (pay_pos < 4 || pay_pos > rec_len || pay_len > rec_len - pay_pos) return false;
    return slot_off <= dst_cap && pay_len <= dst_cap - slot_off;
}

// The slots are one scan over records of {slot bytes (rounded), records with a
// payload, payload bytes}.
struct PayAgg {
    uint64_t off;
    uint64_t k;
    uint64_t bytes;
};
ONC_HD inline PayAgg payload_none() { return PayAgg{0, 0, 0}; }
ONC_HD inline PayAgg payload_elem(bool has, uint32_t payload_len, uint32_t align) {
    return has ? PayAgg{payload_round_up(payload_len, align), 1, payload_len} : payload_none();
}
ONC_HD inline PayAgg payload_join(const PayAgg& a, const PayAgg& b) {
    return PayAgg{a.off + b.off, a.k + b.k, a.bytes + b.bytes};
}

// result of a batch: {records with a payload, payload bytes, the capacity the
// destination needs (= slot_off[n])}.
ONC_HD inline void payload_result(uint64_t result[3], const PayAgg& all) {
    result[0] = all.k;
    result[1] = all.bytes;
    result[2] = all.off;
}

// How far the destination is written at most: the end of the last record's
// slice, cut to dst_cap (the slots are non-decreasing). Only the partition of
// the copy depends on it; every slice is checked by payload_ok.
ONC_HD inline uint64_t payload_extent(uint64_t last_slot, uint32_t last_len, uint64_t dst_cap) {
    if (last_slot >= dst_cap) return dst_cap;
    return last_len < dst_cap - last_slot ? last_slot + last_len : dst_cap;
}

}  // namespace onc
