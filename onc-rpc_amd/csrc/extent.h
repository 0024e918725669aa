// extent.h — the slice bound of the wire-length checked decode entry points
// (onc_decode_bounded, onc_decode_lengths_bounded, onc_decode_body_bounded):
// the reference cuts every record as &wire[off..off + len], which panics
// ("slice index out of range") instead of reading outside the buffer. Plain
// C++ without HIP headers, so a host compiler takes it too (tests build it
// into a stand-alone probe).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ONC_HD __host__ __device__
#else
#define ONC_HD
#endif

namespace onc {

// aux0 of ONC_DEC_BAD_EXTENT, in the order the checks are made
constexpr uint32_t kExtentOk = 0;
constexpr uint32_t kExtentStart = 1;     // the record starts past wire_len
constexpr uint32_t kExtentEnd = 2;       // the record ends past wire_len
constexpr uint32_t kExtentOrder = 3;     // rec_off[i + 1] < rec_off[i]
constexpr uint32_t kExtentHeadShort = 4; // onc_decode_heads: the record's header does not fit its head

// Record [b, b + L) against a wire of wire_len readable bytes. b == wire_len
// with L == 0 is the legal empty slice &wire[len..len]. No sum is formed:
// b + L may wrap.
ONC_HD inline uint32_t extent_reason(uint64_t b, uint64_t L, uint64_t wire_len) {
    if (b > wire_len) return kExtentStart;
    if (L > wire_len - b) return kExtentEnd;
    return kExtentOk;
}

// Record [lo, hi) of an offsets array (rec_off[i], rec_off[i + 1]).
ONC_HD inline uint32_t extent_reason_off(uint64_t lo, uint64_t hi, uint64_t wire_len) {
    if (hi < lo) return kExtentOrder;
    return extent_reason(lo, hi - lo, wire_len);
}

// Record i of a lengths array: b = base + the lengths before it. The prefix
// is below 2^64 (n < 2^32 lengths below 2^32), so the sum wrapped exactly
// when it came out below base: then the record starts past any wire.
ONC_HD inline uint32_t extent_reason_len(uint64_t base, uint64_t b, uint64_t L, uint64_t wire_len) {
    if (b < base) return kExtentStart;
    return extent_reason(b, L, wire_len);
}

}  // namespace onc
