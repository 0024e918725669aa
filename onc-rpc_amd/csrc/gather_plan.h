// gather_plan.h — the arithmetic of onc_piece_offsets / onc_gather_pieces
// (gather.hip): which pieces of a list may be read (gather_ok), what the
// list is cut to by a window of the stream (gather_window), and the sum the
// offsets are scanned with (GatherAgg). A piece {src, off, len} is `len` bytes
// at byte `off` of source `src` (include/onc_rpc.h onc_frag_piece); the stream
// is the pieces back to back. No sum of an offset and a length is formed
// anywhere: off + len may wrap near 2^64, and so may from + count. Plain C++
// without HIP headers, as fragment_iov_plan.h: tests/cpp_gather/plan_probe.cpp
// drives it on the host.
#pragma once

#include <stdint.h>

#include "extent.h"

namespace onc {

constexpr uint32_t kGatherSources = 3;   // ONC_PIECE_MARK, ONC_PIECE_HDR, ONC_PIECE_PAYLOAD

// The piece lies inside its source of src_len[src] bytes. An empty piece is
// fine wherever it points (nothing is read for it); off == the source's length
// is the empty slice at its end and holds no byte.
ONC_HD inline bool gather_ok(uint64_t off, uint32_t len, uint32_t src, uint64_t len0, uint64_t len1, uint64_t len2) {
    if (len == 0) return true;
    if (src >= kGatherSources) return false;
    const uint64_t L = src == 0 ? len0 : src == 1 ? len1 : len2;
    return off <= L && len <= L - off;
}

// How many bytes of the window [from, from + count) exist in a stream of
// `total` bytes: the window's end is never formed (from + count may wrap).
ONC_HD inline uint64_t gather_window(uint64_t from, uint64_t count, uint64_t total) {
    if (from >= total) return 0;
    return count < total - from ? count : total - from;
}

// The offsets are one scan over pieces of {stream bytes, bad pieces, index of
// the first bad piece (~0: none)}.
struct GatherAgg {
    uint64_t bytes;
    uint64_t bad;
    uint64_t first_bad;
};
ONC_HD inline GatherAgg gather_none() { return GatherAgg{0, 0, ~0ull}; }
ONC_HD inline GatherAgg gather_elem(uint64_t i, uint32_t len, bool ok) {
    return GatherAgg{len, ok ? 0u : 1u, ok ? ~0ull : i};
}
ONC_HD inline GatherAgg gather_join(const GatherAgg& a, const GatherAgg& b) {
    return GatherAgg{a.bytes + b.bytes, a.bad + b.bad, a.first_bad < b.first_bad ? a.first_bad : b.first_bad};
}

}  // namespace onc
