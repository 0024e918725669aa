// defrag_heads_plan.h — the host arithmetic of onc_defragment_heads
// (defrag_heads.hip) and of the heads form of the decode (onc_decode_heads):
// the argument rule for head_len, a record's length and status, the slot
// bytes that exist, the result words, and which fragment of a record holds a
// body byte. The record arithmetic itself (B_r, the mark, the scan state) is
// defrag_plan.h's. Plain C++ without HIP headers, as defrag_plan.h: a host
// program drives it up to sizes no buffer has; on the device
// tests/test_gpu_beyond_4gib.py runs it over 4.4 GB of fragments.
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "defrag_plan.h"

namespace onc {

// head_len: a multiple of 16 in [64, 4096] (a slot is whole 16-byte chunks,
// and at least the decode's first round).
ONC_HD inline bool heads_len_ok(uint32_t head_len) {
    return head_len >= 64u && head_len <= 4096u && (head_len & 15u) == 0;
}

// Record r of B body bytes: a body of 2^31 bytes or more is ONC_ENC_TOO_LONG
// (length 0, as onc_defragment); any other record has its true length and is
// OK when a slot is left for it. Slots have a fixed stride, so the capacity
// cut is by record index alone.
ONC_HD inline uint32_t heads_rec_len(uint64_t B) { return defrag_len(B); }
ONC_HD inline int32_t heads_status(uint64_t B, uint64_t r, uint64_t max_records) {
    if (defrag_status(B) != ONC_OK) return ONC_ENC_TOO_LONG;
    return r < max_records ? ONC_OK : ONC_ENC_WRITE_ZERO;
}
// ... from the record's length (0: TOO_LONG), which is what the device keeps
ONC_HD inline int32_t heads_status_len(uint32_t rec_len, uint64_t r, uint64_t max_records) {
    if (rec_len == 0) return ONC_ENC_TOO_LONG;
    return r < max_records ? ONC_OK : ONC_ENC_WRITE_ZERO;
}

// The bytes of record r that exist in its slot: P_r = min(rec_len, head_len).
ONC_HD inline uint32_t heads_present(uint32_t rec_len, uint32_t head_len) {
    return rec_len < head_len ? rec_len : head_len;
}

// result of a batch that closed nrec records with `multi` of them of more
// than one fragment, and left `pending` fragments of `tail` body bytes open.
ONC_HD inline void heads_result(uint64_t result[6], uint64_t nrec, uint64_t nfrag, uint64_t pending, uint64_t tail,
                                uint64_t multi, uint32_t head_len) {
    result[0] = nrec;
    result[1] = nfrag - pending;
    result[2] = nrec * uint64_t(head_len);
    result[3] = pending;
    result[4] = tail;
    result[5] = multi;
}

// The fragment holding body byte x of a record whose fragments are
// [lo, hi) (lo < hi, frag_pre[lo] == 0 <= x): the last j in [lo, hi) with
// frag_pre[j] <= x. An empty fragment starts where the next one does, so for
// x below the record's body length the fragment found is never empty.
ONC_HD inline uint64_t heads_frag_of(const uint64_t* frag_pre, uint64_t lo, uint64_t hi, uint64_t x) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (frag_pre[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace onc
