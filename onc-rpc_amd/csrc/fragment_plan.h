// fragment_plan.h — the record arithmetic of onc_fragment (fragment.hip):
// how many fragments a record of L bytes becomes under a fixed largest
// fragment body F (max_frag), how many bytes they take, its status, the mark
// of fragment j, and the closed-form map from a position inside the
// fragmented record back to a mark byte or a byte of the record's body.
// RFC 5531 §11: a record is a run of fragments, each under a 4-byte mark
// whose low 31 bits are the fragment body's length and whose bit 31 says
// "last". The input record is one fragment as RpcMessage::serialise_into
// writes it (rpc_message.rs:146-156); its own mark is never read: B = L - 4.
// Plain C++ without HIP headers, as defrag_plan.h: a host program
// (tests/cpp_fragment/plan_probe.cpp) drives it up to sizes no buffer has; on
// the device tests/test_gpu_beyond_4gib.py runs it over a 4.4 GB stream and
// over one extent of that length (frag_at's 64-bit branch). Exact for L < 2^61 (the output length, at most 5 B, fits 64 bits).
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "extent.h"   // ONC_HD

namespace onc {

constexpr uint32_t kFragMaxBody = 0x7FFFFFFFu;   // the 31 length bits of a mark

ONC_HD inline bool frag_max_ok(uint32_t F) { return F >= 1 && F <= kFragMaxBody; }

// Fragments of a body of B bytes: ceil(B / F), and one (the bare last mark)
// for an empty body. B + F - 1 is never formed: it may wrap.
ONC_HD inline uint64_t frag_count(uint64_t B, uint32_t F) {
    const uint64_t k = B / F + (B % F != 0 ? 1 : 0);
    return k ? k : 1;
}

// What an extent of L bytes becomes: k fragments in len bytes. An empty
// extent (a failing record's) is nothing to send; one of 1..3 bytes has no
// room for a mark (ONC_ENC_BAD_DESCRIPTOR); neither takes output bytes.
struct FragRec {
    uint64_t k;
    uint64_t len;
    int32_t status;   // before the capacity test
};
ONC_HD inline FragRec frag_rec(uint64_t L, uint32_t F) {
    if (L == 0) return FragRec{0, 0, ONC_OK};
    if (L < 4) return FragRec{0, 0, ONC_ENC_BAD_DESCRIPTOR};
    const uint64_t B = L - 4, k = frag_count(B, F);
    return FragRec{k, 4 * k + B, ONC_OK};
}

// len bytes placed at off end within cap. No sum is formed: off + len may
// wrap (defrag_plan.h defrag_fits).
ONC_HD inline bool frag_fits(uint64_t off, uint64_t len, uint64_t cap) { return off <= cap && len <= cap - off; }

// Status of a record after the capacity test.
ONC_HD inline int32_t frag_status(const FragRec& r, uint64_t off, uint64_t cap) {
    if (r.k == 0) return r.status;
    return frag_fits(off, r.len, cap) ? ONC_OK : ONC_ENC_WRITE_ZERO;
}

// Body bytes of fragment j (< k) of a body of B bytes, and its mark: every
// fragment but the last is full; the last carries bit 31 and the rest
// (j * F <= B for j < k, so nothing wraps).
ONC_HD inline uint64_t frag_rest(uint64_t B, uint64_t j, uint32_t F) { return B - j * F; }
ONC_HD inline uint32_t frag_body_len(uint64_t B, uint64_t j, uint32_t F) {
    const uint64_t rest = frag_rest(B, j, F);
    return rest > F ? F : uint32_t(rest);
}
ONC_HD inline uint32_t frag_mark(uint64_t B, uint64_t j, uint32_t F) {
    const uint64_t rest = frag_rest(B, j, F);
    return rest > F ? F : 0x80000000u | uint32_t(rest);
}
ONC_HD inline uint8_t frag_mark_byte(uint32_t mark, uint32_t r) { return uint8_t(mark >> (24 - 8 * r)); }

// Output position q (< len) of a fragmented record: every fragment before
// the last takes F + 4 bytes, so q lies in fragment j = q / (F + 4) at byte
// r = q % (F + 4) of it: r < 4 is byte r of that fragment's mark, otherwise
// the byte is body[j * F + r - 4]. No table, no search.
struct FragAt {
    uint64_t j;
    uint32_t r;   // < F + 4 <= 0x80000003
};
ONC_HD inline uint64_t frag_stride(uint32_t F) { return uint64_t(F) + 4; }
ONC_HD inline FragAt frag_at(uint64_t q, uint32_t F) {
    const uint64_t s = frag_stride(F);
    return FragAt{q / s, uint32_t(q % s)};
}
// The same for q < 2^32 (any position of a record whose output is shorter
// than 4 GiB): one 32-bit division.
ONC_HD inline FragAt frag_at32(uint32_t q, uint32_t F) {
    const uint32_t s = F + 4u;
    return FragAt{q / s, q % s};
}
ONC_HD inline bool frag_is_mark(const FragAt& a) { return a.r < 4; }
ONC_HD inline uint64_t frag_src(const FragAt& a, uint32_t F) { return a.j * F + (a.r - 4); }   // a.r >= 4
// The 16 output bytes from position `a` on lie inside that one fragment's body.
ONC_HD inline bool frag_run16(const FragAt& a, uint64_t B, uint32_t F) {
    return a.r >= 4 && uint64_t(a.r) - 4 + 16 <= frag_body_len(B, a.j, F);
}

// The plan is one sum scan over records of {output bytes, fragments, records
// of more than one fragment}; sums wrap modulo 2^64 the same way in any
// grouping, so blocks of records scan in parallel.
struct FragAgg {
    uint64_t bytes;
    uint64_t frags;
    uint64_t multi;
};
ONC_HD inline FragAgg frag_none() { return FragAgg{0, 0, 0}; }
ONC_HD inline FragAgg frag_elem(const FragRec& r) { return FragAgg{r.len, r.k, r.k > 1 ? 1u : 0u}; }
ONC_HD inline FragAgg frag_join(const FragAgg& a, const FragAgg& b) {
    return FragAgg{a.bytes + b.bytes, a.frags + b.frags, a.multi + b.multi};
}

}  // namespace onc
