// route_plan.h — the arithmetic of onc_route_calls (route.hip): the rules a
// route table obeys (route_entry_ok, route_pair_ok, route_bad_at), the lookup
// of a Call's (program, version, procedure) in it (route_key_le, route_upper,
// route_lookup: handler or the RFC 5531 §9 rejection with its low / high), a
// record's bin (route_bin) and the scratch its partition needs
// (route_scratch_words). All keys are compared unsigned, word by word; no sum of a
// procedure and a count is formed in 32 bits (proc_first + proc_count may be
// 2^32). Plain C++ without HIP headers, as payload_plan.h:
// tests/cpp_route/plan_probe.cpp drives it on the host.
#pragma once

#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "partition_plan.h"

namespace onc {

constexpr uint32_t kRouteTile = 1024;     // records per tile (= threads per workgroup)

// Bins: the handlers, then rejected, not-a-Call, failed.
ONC_HD inline uint32_t route_bins(uint32_t nh) { return nh + 3; }
// u32 words of scratch: the counts (at bin_count_at) and one total per bin.
ONC_HD inline uint64_t route_scratch_words(uint64_t n, uint32_t nh, uint32_t tile) {
    return uint64_t(route_bins(nh)) * (tile_count(n, tile) + 1);
}

// An entry's own rules.
ONC_HD inline bool route_entry_ok(const onc_route& e, uint32_t nh) {
    if (e.proc_count == 0) return false;
    if (uint64_t(e.proc_first) + uint64_t(e.proc_count) > (1ull << 32)) return false;
    if (e.flags & ~uint32_t(ONC_ROUTE_ONE_HANDLER)) return false;
    const uint64_t handlers = (e.flags & ONC_ROUTE_ONE_HANDLER) ? 1ull : uint64_t(e.proc_count);
    return uint64_t(e.handler_first) + handlers <= uint64_t(nh);
}

// (program, version, procedure) of `a` at or before that of `b`.
ONC_HD inline bool route_key_le(uint32_t ap, uint32_t av, uint32_t ac, uint32_t bp, uint32_t bv, uint32_t bc) {
    if (ap != bp) return ap < bp;
    if (av != bv) return av < bv;
    return ac <= bc;
}

// Entries a, b that follow each other: strictly ascending, and the ranges of
// one (program, version) apart.
ONC_HD inline bool route_pair_ok(const onc_route& a, const onc_route& b) {
    if (route_key_le(b.program, b.version, b.proc_first, a.program, a.version, a.proc_first)) return false;
    if (a.program == b.program && a.version == b.version)
        return uint64_t(a.proc_first) + uint64_t(a.proc_count) <= uint64_t(b.proc_first);
    return true;
}

// Entry i breaks a rule of its own, or the pair (i, i + 1) an order rule.
template <class Table>
ONC_HD inline bool route_bad_at(const Table& t, uint32_t ntab, uint32_t nh, uint32_t i) {
    if (!route_entry_ok(t[i], nh)) return true;
    return i + 1 < ntab && !route_pair_ok(t[i], t[i + 1]);
}

// The first bad entry + 1, or 0 for a valid table (result[3]).
template <class Table>
ONC_HD inline uint32_t route_first_bad(const Table& t, uint32_t ntab, uint32_t nh) {
    for (uint32_t i = 0; i < ntab; ++i)
        if (route_bad_at(t, ntab, nh, i)) return i + 1;
    return 0;
}

// How many entries start at or before the key (a sorted table): the entry
// before that index is the only one that can hold the key.
template <class Table>
ONC_HD inline uint32_t route_upper(const Table& t, uint32_t ntab, uint32_t program, uint32_t version, uint32_t proc) {
    uint32_t lo = 0, hi = ntab;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (route_key_le(t[mid].program, t[mid].version, t[mid].proc_first, program, version, proc)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct RouteOutcome {
    uint32_t bin;           // the handler, or nh (rejected)
    uint32_t stat;          // ONC_ACCEPT_SUCCESS | _PROC_UNAVAIL | _PROG_MISMATCH | _PROG_UNAVAIL
    uint32_t low, high;     // PROG_MISMATCH: the program's least and greatest version; else 0
};

// A Call's route in a valid table.
template <class Table>
ONC_HD inline RouteOutcome route_lookup(const Table& t, uint32_t ntab, uint32_t nh, uint32_t program,
                                        uint32_t version, uint32_t proc) {
    const uint32_t u = route_upper(t, ntab, program, version, proc);
    // the entries around the key: t[u - 1] starts at or before it, t[u] after it
    bool same_pv = false, same_p = false;
    if (u > 0) {
        const onc_route e = t[u - 1];
        same_p = e.program == program;
        same_pv = same_p && e.version == version;
        if (same_pv && proc - e.proc_first < e.proc_count)          // (proc >= proc_first: the key order)
            return RouteOutcome{e.handler_first + ((e.flags & ONC_ROUTE_ONE_HANDLER) ? 0u : proc - e.proc_first),
                                ONC_ACCEPT_SUCCESS, 0, 0};
    }
    if (u < ntab) {
        const onc_route e = t[u];
        same_p = same_p || e.program == program;
        same_pv = same_pv || (e.program == program && e.version == version);
    }
    if (same_pv) return RouteOutcome{nh, ONC_ACCEPT_PROC_UNAVAIL, 0, 0};
    if (!same_p) return RouteOutcome{nh, ONC_ACCEPT_PROG_UNAVAIL, 0, 0};
    // the program's entries are [first, last]: the first starting at or after
    // (program, 0, 0), the last starting at or before (program, max, max)
    const uint32_t before = route_upper(t, ntab, program, 0, 0);
    const uint32_t first = (before > 0 && t[before - 1].program == program) ? before - 1 : before;
    const uint32_t last = route_upper(t, ntab, program, 0xFFFFFFFFu, 0xFFFFFFFFu) - 1;
    return RouteOutcome{nh, ONC_ACCEPT_PROG_MISMATCH, t[first].version, t[last].version};
}

// A record's bin; `call`: the lookup's bin of an OK Call.
ONC_HD inline uint32_t route_bin(int32_t status, uint32_t msg_type, uint32_t call, uint32_t nh) {
    if (status != ONC_OK) return ONC_ROUTE_BIN_FAILED(nh);
    if (msg_type != ONC_MSG_CALL) return ONC_ROUTE_BIN_NOT_CALL(nh);
    return call;
}

}  // namespace onc
