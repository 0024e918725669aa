// xdr_plan.h — the arithmetic of onc_xdr_unpack (xdr.hip): the rules a schema
// obeys (xdr_field_ok, xdr_schema_first_bad) with a column's width and byte
// range, a payload's extent in the three position forms (xdr_extent), and the
// parse of one record against the schema (xdr_parse) over a word reader and a
// column sink — the kernel's reader fetches 16-byte granules and its sink
// stores to the columns; tests/cpp_xdr/plan_probe.cpp reads a byte vector and
// prints. Every "need <= left" test compares against a difference that cannot
// be negative: no sum of a position and a length is formed, pad4 and
// count * 8 are 64 bits wide (pad4(0xFFFFFFFD) is 2^32, 0x20000000 * 8 too).
// Plain C++ without HIP headers, as route_plan.h.
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "extent.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ONC_XDR_INLINE __forceinline__
#else
#define ONC_XDR_INLINE inline
#endif

namespace onc {

constexpr uint32_t kXdrTile = 256;        // records per tile (= threads per workgroup)
constexpr uint32_t kXdrTypeMax = ONC_XDR_ARRAY64;
constexpr uint32_t kXdrFlags = ONC_XDR_SELECT | ONC_XDR_IF | ONC_XDR_NO_COLUMN;

ONC_HD inline uint64_t xdr_pad4(uint64_t x) { return (x + 3ull) & ~3ull; }
ONC_HD inline uint32_t xdr_type(uint32_t type_flags) { return type_flags & 0xFFu; }
ONC_HD inline uint64_t xdr_tiles(uint64_t n) { return (n + kXdrTile - 1) / kXdrTile; }

// Bytes a record takes in the field's column.
ONC_HD inline uint32_t xdr_col_width(uint32_t type) {
    return (type == ONC_XDR_U32 || type == ONC_XDR_BOOL || type == ONC_XDR_OPAQUE_FIXED) ? 4u : 8u;
}
ONC_HD inline uint32_t xdr_col_align(uint32_t type) { return type == ONC_XDR_U64 ? 8u : 4u; }
ONC_HD inline bool xdr_uses_arg(uint32_t type) { return type >= ONC_XDR_OPAQUE_FIXED; }
ONC_HD inline bool xdr_has_column(uint32_t type_flags) { return !(type_flags & ONC_XDR_NO_COLUMN); }

// The bytes a present field reads before anything else is known about it: its
// value, or its length / count word (an OPAQUE_FIXED body is never read).
ONC_HD inline uint32_t xdr_head_bytes(uint32_t type) {
    return type == ONC_XDR_U64 ? 8u : (type == ONC_XDR_OPAQUE_FIXED ? 0u : 4u);
}
// The bytes behind a length / count word of value v.
ONC_HD inline uint64_t xdr_body_bytes(uint32_t type, uint32_t v) {
    if (type == ONC_XDR_OPAQUE_VAR) return xdr_pad4(uint64_t(v));
    if (type == ONC_XDR_ARRAY32) return uint64_t(v) * 4ull;
    return uint64_t(v) * 8ull;                       // ARRAY64
}
ONC_HD inline bool xdr_fits(uint64_t need, uint64_t left) { return need <= left; }

// A field's rules that need no other field but `selected`: an earlier field
// carries SELECT. (The overlap rule is xdr_schema_first_bad's.)
ONC_HD inline bool xdr_field_ok(const onc_xdr_field& f, bool selected, uint64_t n, uint64_t cols_cap) {
    const uint32_t type = xdr_type(f.type_flags);
    if (type > kXdrTypeMax) return false;
    if ((f.type_flags & ~(0xFFu | kXdrFlags)) || f.reserved != 0) return false;
    if ((f.type_flags & ONC_XDR_SELECT) && type != ONC_XDR_U32 && type != ONC_XDR_BOOL) return false;
    if ((f.type_flags & ONC_XDR_IF) && !selected) return false;
    if (!(f.type_flags & ONC_XDR_IF) && f.cond_val != 0) return false;
    if (!xdr_uses_arg(type) && f.arg != 0) return false;
    if (!xdr_has_column(f.type_flags)) return f.col_off == 0;
    if (f.col_off & (xdr_col_align(type) - 1)) return false;
    if (f.col_off > cols_cap) return false;
    return n <= (cols_cap - f.col_off) / xdr_col_width(type);     // width * n <= cols_cap - col_off
}

// Byte ranges [a, a + wa) and [b, b + wb) inside cols_cap (so no end wraps).
ONC_HD inline bool xdr_ranges_overlap(uint64_t a, uint64_t wa, uint64_t b, uint64_t wb) {
    return wa != 0 && wb != 0 && a < b + wb && b < a + wa;
}

// The first bad field + 1, or 0 for a valid schema.
template <class Fields>
ONC_HD inline uint32_t xdr_schema_first_bad(const Fields& fields, uint32_t nf, uint64_t n, uint64_t cols_cap) {
    bool selected = false;
    for (uint32_t f = 0; f < nf; ++f) {
        const onc_xdr_field& fl = fields[f];
        if (!xdr_field_ok(fl, selected, n, cols_cap)) return f + 1;
        if (xdr_has_column(fl.type_flags)) {
            const uint64_t w = uint64_t(xdr_col_width(xdr_type(fl.type_flags))) * n;
            for (uint32_t e = 0; e < f; ++e) {
                const onc_xdr_field& el = fields[e];
                if (!xdr_has_column(el.type_flags)) continue;
                if (xdr_ranges_overlap(fl.col_off, w, el.col_off, uint64_t(xdr_col_width(xdr_type(el.type_flags))) * n))
                    return f + 1;
            }
        }
        if (fl.type_flags & ONC_XDR_SELECT) selected = true;
    }
    return 0;
}

// How far into its payload a record's word reads can reach, `cap` at most:
// the end of the last word read with every field present and every length and
// count at its maximum. The kernel fetches that many payload bytes (those the
// record has) before it has parsed anything, so that the words behind a
// length — an NFS file handle's, say — need no further round trip; a schema of
// one word still fetches one granule.
template <class Fields>
ONC_HD inline uint64_t xdr_reach(const Fields& fields, uint32_t nf, uint64_t cap) {
    uint64_t bytes = 0, reach = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        const onc_xdr_field& fl = fields[f];
        const uint32_t type = xdr_type(fl.type_flags);
        const uint32_t head = xdr_head_bytes(type);
        if (bytes >= cap) {                                  // a word this far out: the cap
            if (!head) continue;
            reach = cap;
            break;
        }
        if (head) reach = bytes + head;
        bytes += head;                                       // (below cap + 8: no sum here wraps)
        if (type == ONC_XDR_OPAQUE_FIXED) bytes += xdr_pad4(uint64_t(fl.arg));
        else if (type >= ONC_XDR_OPAQUE_VAR) bytes += xdr_body_bytes(type, fl.arg);
    }
    return reach < cap ? reach : cap;
}

// Does the record carry a payload? `kinds`: msg_type | reply_stat << 8 | stat << 16 (the descriptor's second word).
ONC_HD inline bool xdr_carries(int32_t status, uint32_t kinds) {
    if (status != ONC_OK) return false;
    const uint32_t msg_type = kinds & 0xFFu, reply_stat = (kinds >> 8) & 0xFFu, stat = (kinds >> 16) & 0xFFu;
    return msg_type == ONC_MSG_CALL ||
           (msg_type == ONC_MSG_REPLY && reply_stat == ONC_REPLY_ACCEPTED && stat == ONC_ACCEPT_SUCCESS);
}

struct XdrExtent {
    bool bad;
    uint64_t base;      // what a payload position adds to become a column's position
    uint64_t hi;        // the end of the readable window, as a wire offset
};

// The payload [o, o + L) of record r. heads: rec_start is not given and
// head_len != 0. start: rec_start[r] when has_start.
ONC_HD inline XdrExtent xdr_extent(uint64_t o, uint64_t L, uint64_t r, bool heads, uint32_t head_len, bool has_start,
                                   uint64_t start, uint64_t wire_len) {
    XdrExtent e{false, 0, 0};
    if (heads) {
        const uint64_t lo = r * uint64_t(head_len);          // (r < n and n * head_len <= wire_len)
        e.hi = lo + head_len;
        e.bad = o < lo || o > e.hi;
        e.base = o - lo;
    } else {
        e.hi = wire_len;
        e.bad = o > wire_len || L > wire_len - o;
        if (has_start) {
            e.bad = e.bad || o < start;
            e.base = o - start;
        }
    }
    if (!e.bad && (e.base > 0xFFFFFFFFull || L > 0xFFFFFFFFull - e.base)) e.bad = true;   // base + L > 0xFFFFFFFF
    if (e.bad) e.base = 0;
    return e;
}

struct XdrParsed {
    uint32_t code;      // ONC_XDR_*
    uint32_t fail;      // the failing field (nf: TRAILING), else 0
    uint64_t present;   // bit f: field f was completed
    uint64_t p;         // bytes consumed (an OK record)
};

// One record against the schema. `code`: ONC_XDR_OK to parse, or the code of a
// record that is not parsed (SKIPPED, BAD_EXTENT): every sink call then passes
// zeros, so that the caller's loop over the fields is the same for every
// record. Reader: uint32_t word(uint64_t p), the big-endian word at payload
// position p — called only for words inside the payload and the window.
// Sink: put32(field, v), put64(field, v), put_pair(field, pos, len), each
// called once per field of its kind, in field order.
// (Inlined into the kernel whatever its size: a reader passed by address
// would live in scratch memory.)
template <class Fields, class Reader, class Sink>
ONC_HD ONC_XDR_INLINE XdrParsed xdr_parse(const Fields& fields, uint32_t nf, uint32_t flags, uint32_t code, uint64_t o,
                                  uint64_t L, const XdrExtent& e, bool heads, Reader& rd, Sink& sink) {
    XdrParsed out{code, 0, 0, 0};
    uint64_t p = 0;
    uint32_t sel = 0;
    bool sel_ok = false;
    for (uint32_t f = 0; f < nf; ++f) {
        const onc_xdr_field& fl = fields[f];
        const uint32_t tf = fl.type_flags, type = xdr_type(tf);
        uint32_t v = 0, pos = 0;
        uint64_t v64 = 0;
        if (out.code == ONC_XDR_OK) {
            if ((tf & ONC_XDR_IF) && !(sel_ok && sel == fl.cond_val)) {
                if (tf & ONC_XDR_SELECT) sel_ok = false;                  // absent
            } else {
                const uint64_t left = L - p;
                const uint32_t head = xdr_head_bytes(type);
                uint32_t fail = ONC_XDR_OK;
                uint64_t step = head;
                if (!xdr_fits(head, left)) {
                    fail = ONC_XDR_SHORT;
                } else if (heads && head != 0 && o + p + head > e.hi) {   // (o <= hi and p + head <= 2^32)
                    fail = ONC_XDR_HEAD_SHORT;
                } else if (type == ONC_XDR_OPAQUE_FIXED) {
                    step = xdr_pad4(uint64_t(fl.arg));
                    if (!xdr_fits(step, left)) fail = ONC_XDR_SHORT;
                    else pos = uint32_t(e.base + p);
                } else {
                    v = rd.word(p);
                    if (type == ONC_XDR_U64) {
                        v64 = (uint64_t(v) << 32) | uint64_t(rd.word(p + 4));
                    } else if (type == ONC_XDR_BOOL) {
                        if (v > 1u) fail = ONC_XDR_BAD_BOOL;
                    } else if (type >= ONC_XDR_OPAQUE_VAR) {
                        const uint64_t body = xdr_body_bytes(type, v);
                        if (v > fl.arg) fail = ONC_XDR_TOO_LONG;
                        else if (!xdr_fits(body, left - 4)) fail = ONC_XDR_SHORT;
                        else {
                            pos = uint32_t(e.base + p + 4);
                            step = 4 + body;
                        }
                    }
                }
                if (fail != ONC_XDR_OK) {
                    out.code = fail;
                    out.fail = f;
                    v = 0;
                    v64 = 0;
                    pos = 0;
                } else {
                    p += step;
                    out.present |= 1ull << f;
                    if (tf & ONC_XDR_SELECT) {
                        sel = v;
                        sel_ok = true;
                    }
                }
            }
        }
        if (type == ONC_XDR_U64) sink.put64(fl, v64);
        else if (type >= ONC_XDR_OPAQUE_VAR) sink.put_pair(fl, pos, v);
        else if (type == ONC_XDR_OPAQUE_FIXED) sink.put32(fl, pos);
        else sink.put32(fl, v);
    }
    if (out.code == ONC_XDR_OK) {
        if ((flags & ONC_XDR_EXACT) && L - p != 0) {
            out.code = ONC_XDR_TRAILING;
            out.fail = nf;
        } else {
            out.p = p;
        }
    }
    return out;
}

}  // namespace onc
