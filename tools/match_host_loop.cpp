// match_host_loop.cpp — what a client does today instead of onc_match_replies,
// as tools/match_timing.py times it: one thread's loop over the descriptors a
// decode left (copied to the host), a std::unordered_map from (conn, xid) to
// the lowest pending index built over the same list, every OK Reply looked up
// in it, the first Reply of an entry told from its duplicates, and hit[].
// Built by the tool with the host compiler into a shared object.
#include <cstring>
#include <unordered_map>
#include <vector>

#include "match_plan.h"

extern "C" void match_host_loop(const onc_msg* msgs, const int32_t* status, const uint32_t* rec_conn, uint64_t n,
                                const onc_pending* pending, uint64_t np, uint32_t* match, uint32_t* hit,
                                uint64_t* result) {
    std::unordered_map<uint64_t, uint32_t> lead;
    lead.reserve(size_t(np));
    for (uint64_t p = 0; p < np; ++p)
        lead.emplace((uint64_t(pending[p].conn) << 32) | pending[p].xid, uint32_t(p));     // (the first stays)
    for (uint64_t p = 0; p < np; ++p) hit[p] = ONC_MATCH_NONE;
    uint64_t count[5] = {0, 0, 0, 0, 0};
    for (uint64_t r = 0; r < n; ++r) {
        uint32_t m = onc::match_class(status[r], msgs[r].msg_type);
        if (m == 0) {
            const auto it = lead.find((uint64_t(rec_conn ? rec_conn[r] : 0u) << 32) | msgs[r].xid);
            if (it == lead.end()) m = ONC_MATCH_UNKNOWN;
            else if (hit[it->second] != ONC_MATCH_NONE) m = ONC_MATCH_DUPLICATE;
            else {
                m = it->second;
                hit[m] = uint32_t(r);
            }
        }
        match[r] = m;
        ++count[onc::match_result_class(m)];
    }
    uint64_t k = 0;
    for (uint64_t p = 0; p < np; ++p) k += hit[p] == ONC_MATCH_NONE;
    for (int c = 0; c < 5; ++c) result[c] = count[c];
    result[5] = k;
}
