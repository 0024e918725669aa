// fragment_iov_plan.h — the record arithmetic of onc_fragment_iov
// (fragment_iov.hip): a vectored record (onc_iov_rec: hdr_len header bytes,
// the first four of them its own mark, then payload_len payload bytes) cut
// into fragments of at most F body bytes without a wire byte being read. Its
// body is B = hdr_len + payload_len - 4 bytes: Hb = hdr_len - 4 from the
// header buffer, then the payload. What the call writes per record is k marks
// (fragment_plan.h frag_count / frag_mark) and a list of pieces: per fragment
// its mark, then the slice of the header it covers, then the slice of the
// payload. Exactly one fragment can hold both (x = 1): the one the header ends
// inside. The closed-form map from a piece's index inside the record back to
// (fragment, part) needs no table and no search. Plain C++ without HIP
// headers, as fragment_plan.h: tests/cpp_fragment_iov/plan_probe.cpp drives it
// at every length; on the device tests/test_gpu_far_offsets.py runs it on
// entries that name 4 GiB payloads (nothing is read behind an entry). hdr_len and payload_len are 32 bits, so
// B < 2^33, k <= 2^33 and a record has at most 2^34 + 1 pieces.
#pragma once

#include <stdint.h>

#include "fragment_plan.h"

namespace onc {

// Fragments of a body of B bytes (fragment_plan.h frag_count), with one
// 32-bit division where B allows it.
ONC_HD inline uint64_t fiv_count(uint64_t B, uint32_t F) {
    if (B > 0xFFFFFFFFull) return frag_count(B, F);
    const uint32_t b = uint32_t(B), k = b / F + (b % F != 0 ? 1u : 0u);
    return k ? k : 1;
}

// Where the header ends inside the body: Hb header bytes of B, the last of
// them in fragment s = Hb / F; x = 1 when that fragment holds header bytes,
// then payload bytes. Two 32-bit divisions (Hb < 2^32): all the fill needs.
struct FivShape {
    uint64_t Hb;
    uint64_t B;
    uint64_t s;
    uint32_t x;
};
ONC_HD inline FivShape fiv_shape(uint32_t hdr_len, uint32_t payload_len, uint32_t F) {   // hdr_len >= 4, F valid
    const uint32_t Hb = hdr_len - 4u;
    return FivShape{Hb, uint64_t(Hb) + payload_len, Hb / F, (Hb % F != 0 && payload_len > 0) ? 1u : 0u};
}

// What an entry becomes: k fragments in len stream bytes, listed as e pieces.
// An entry of no bytes (a failing record's) is nothing to send; one whose
// header has no room for a mark, or whose limit is not a fragment size, is
// ONC_ENC_BAD_DESCRIPTOR; neither takes marks, pieces or stream bytes.
struct FivRec {
    uint64_t k;
    uint64_t len;
    uint64_t e;
    int32_t status;   // before the capacity tests
};
ONC_HD inline FivRec fiv_rec(uint32_t hdr_len, uint32_t payload_len, uint32_t F) {
    if (hdr_len == 0 && payload_len == 0) return FivRec{0, 0, 0, ONC_OK};
    if (hdr_len < 4 || !frag_max_ok(F)) return FivRec{0, 0, 0, ONC_ENC_BAD_DESCRIPTOR};
    const FivShape sh = fiv_shape(hdr_len, payload_len, F);
    const uint64_t k = fiv_count(sh.B, F);
    return FivRec{k, 4 * k + sh.B, sh.B == 0 ? 1 : 2 * k + sh.x, ONC_OK};
}

// Status after both capacity tests: e pieces from piece np on within
// max_pieces, and k marks from mark nf on within marks_cap bytes. No sum and
// no product of a position is formed: 4 nf <= cap is nf <= cap / 4, and
// 4 k <= cap - 4 nf is k <= cap / 4 - nf (frag_fits).
ONC_HD inline bool fiv_fits(const FivRec& r, uint64_t np, uint64_t max_pieces, uint64_t nf, uint64_t marks_cap) {
    return frag_fits(np, r.e, max_pieces) && frag_fits(nf, r.k, marks_cap / 4);
}
ONC_HD inline int32_t fiv_status(const FivRec& r, uint64_t np, uint64_t max_pieces, uint64_t nf, uint64_t marks_cap) {
    if (r.k == 0) return r.status;
    return fiv_fits(r, np, max_pieces, nf, marks_cap) ? ONC_OK : ONC_ENC_WRITE_ZERO;
}

// Piece t (< e) of a record: fragment j, part c (0: the mark; 1: the first
// slice of its body; 2: the payload slice after a header slice). Fragment
// j's pieces start at 2 j + (j > s ? x : 0), so
//   t <= 2 s + 1          -> (t / 2, t % 2)
//   t == 2 s + 2, x == 1  -> (s, 2)
//   otherwise             -> ((t - x) / 2, (t - x) % 2)
struct FivAt {
    uint64_t j;
    uint32_t c;
};
ONC_HD inline FivAt fiv_at(const FivShape& r, uint64_t t) {
    if (t <= 2 * r.s + 1) return FivAt{t >> 1, uint32_t(t & 1)};
    if (r.x && t == 2 * r.s + 2) return FivAt{r.s, 2};
    const uint64_t u = t - r.x;
    return FivAt{u >> 1, uint32_t(u & 1)};
}
ONC_HD inline uint64_t fiv_first_piece(const FivShape& r, uint64_t j) { return 2 * j + (j > r.s ? r.x : 0); }

// The piece itself (include/onc_rpc.h onc_frag_piece), relative to the
// record: the caller adds the marks before the record, its hdr_off and its
// payload_off.
struct FivPiece {
    uint64_t off;   // MARK: 4 j; HDR: from the record's hdr_off; PAYLOAD: from its payload_off
    uint32_t len;
    uint32_t src;
};
ONC_HD inline FivPiece fiv_piece(const FivShape& r, uint32_t F, const FivAt& at) {
    if (at.c == 0) return FivPiece{4 * at.j, 4, ONC_PIECE_MARK};
    const uint64_t a = at.j * F, b = a + frag_body_len(r.B, at.j, F);
    if (at.c == 2) return FivPiece{0, uint32_t(b - r.Hb), ONC_PIECE_PAYLOAD};
    if (a < r.Hb) return FivPiece{4 + a, uint32_t((b < r.Hb ? b : r.Hb) - a), ONC_PIECE_HDR};
    return FivPiece{a - r.Hb, uint32_t(b - a), ONC_PIECE_PAYLOAD};
}

// The plan is one sum scan over records of {stream bytes, fragments, records
// of more than one fragment, pieces}: fragment_plan.h's, one field wider.
struct FivAgg {
    uint64_t bytes;
    uint64_t frags;
    uint64_t multi;
    uint64_t pieces;
};
ONC_HD inline FivAgg fiv_none() { return FivAgg{0, 0, 0, 0}; }
ONC_HD inline FivAgg fiv_elem(const FivRec& r) { return FivAgg{r.len, r.k, r.k > 1 ? 1u : 0u, r.e}; }
ONC_HD inline FivAgg fiv_join(const FivAgg& a, const FivAgg& b) {
    return FivAgg{a.bytes + b.bytes, a.frags + b.frags, a.multi + b.multi, a.pieces + b.pieces};
}

}  // namespace onc
