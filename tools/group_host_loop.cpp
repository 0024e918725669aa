// group_host_loop.cpp — the route taken before onc_group_by_conn: one thread's
// counting sort of a send batch by connection and the gather of its
// descriptors, over arrays copied to the host. Built by tools/group_timing.py
// as a shared object and timed beside the device call; its outputs are what
// the first repetition of that call is checked against. The contract is
// include/onc_rpc.h's.
#include <cstdint>
#include <cstring>
#include <vector>

#include "group_plan.h"

extern "C" void group_host_loop(const uint32_t* rec_conn, uint64_t nsrc, const uint32_t* via, uint64_t n,
                                uint32_t nconn, uint32_t* order, uint64_t* conn_first, const onc_msg* msgs,
                                onc_msg* msgs_out, uint64_t* result) {
    const uint64_t groups = uint64_t(nconn) + 1;
    std::vector<uint32_t> key(n);
    std::vector<uint64_t> at(groups + 1, 0);
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t s = via ? via[k] : k;
        key[k] = onc::group_clamp(s < nsrc ? rec_conn[s] : nconn, nconn);
        ++at[key[k] + 1];
    }
    uint64_t active = 0;
    for (uint64_t c = 0; c < groups; ++c) {
        active += c < nconn && at[c + 1] != 0;
        at[c + 1] += at[c];
    }
    std::memcpy(conn_first, at.data(), 8 * (groups + 1));
    for (uint64_t k = 0; k < n; ++k) order[at[key[k]]++] = uint32_t(k);
    if (msgs_out)
        for (uint64_t j = 0; j < n; ++j) msgs_out[j] = msgs[order[j]];
    result[0] = conn_first[nconn];
    result[1] = n - conn_first[nconn];
    result[2] = active;
}
