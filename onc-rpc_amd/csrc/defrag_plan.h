// defrag_plan.h — the record arithmetic of onc_defragment (defrag.hip):
// which record a fragment belongs to, a record's body bytes B_r, its length,
// status and mark, and the capacity test. RFC 5531 §11: a record is a run of
// fragments, the last one marked by bit 31 of its mark; the reassembled
// record is what RpcMessage::serialise_into writes (rpc_message.rs:146-156:
// one mark with the last-fragment bit and the body length, a body of 2^31
// bytes or more refused). Plain C++ without HIP headers, as extent.h: a host
// program drives it up to sizes no buffer has; on the device
// tests/test_gpu_beyond_4gib.py runs it over 4.4 GB of fragments and on one
// record of more than 2^32 bytes.
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "extent.h"   // ONC_HD

namespace onc {

// Body bytes of the fragment [lo, hi) of a trusted offsets array (hi - lo >= 4).
ONC_HD inline uint64_t defrag_body(uint64_t lo, uint64_t hi) { return hi - lo - 4; }

// A record of B body bytes: the mark holds 31 bits of length
// (rpc_message.rs:146-151), so B >= 2^31 is ONC_ENC_TOO_LONG and takes no
// output bytes; any other record takes its mark and its body.
ONC_HD inline int32_t defrag_status(uint64_t B) { return B > 0x7FFFFFFFull ? ONC_ENC_TOO_LONG : ONC_OK; }
ONC_HD inline uint32_t defrag_len(uint64_t B) { return B > 0x7FFFFFFFull ? 0u : uint32_t(B) + 4u; }
ONC_HD inline uint32_t defrag_mark(uint64_t B) { return 0x80000000u | uint32_t(B); }   // B < 2^31

// A record of len bytes placed at off ends within cap. No sum is formed:
// off + len may wrap.
ONC_HD inline bool defrag_fits(uint64_t off, uint64_t len, uint64_t cap) { return off <= cap && len <= cap - off; }

// The plan is one scan over fragments with this state: `lasts` records are
// complete, the open record has `cnt` fragments and `tail` body bytes so
// far. As a value it stands for a run of fragments (has = the run holds a
// last fragment: what came before it no longer shows in tail / cnt), and
// defrag_join is associative, so blocks of fragments scan in parallel.
struct DefragAgg {
    uint64_t tail;
    uint64_t lasts;
    uint64_t cnt;
    uint64_t has;
};

ONC_HD inline DefragAgg defrag_none() { return DefragAgg{0, 0, 0, 0}; }

// One fragment: a last fragment closes its record (its own body is added by
// whoever closes the record: B_r = the state before it . tail + its body).
ONC_HD inline DefragAgg defrag_elem(uint64_t body, bool last) {
    return last ? DefragAgg{0, 1, 0, 1} : DefragAgg{body, 0, 1, 0};
}

// The run a followed by the run b.
ONC_HD inline DefragAgg defrag_join(const DefragAgg& a, const DefragAgg& b) {
    if (b.has) return DefragAgg{b.tail, a.lasts + b.lasts, b.cnt, 1};
    return DefragAgg{a.tail + b.tail, a.lasts + b.lasts, a.cnt + b.cnt, a.has};
}

}  // namespace onc
