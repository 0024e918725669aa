// route_host_loop.cpp — what a server does today instead of onc_route_calls,
// as tools/route_timing.py times it: one thread's loop over the descriptors a
// decode left (copied to the host), the lookup of onc-rpc_amd/csrc/route_plan.h
// per Call, a counting sort into `order`, and the reply descriptors in that
// order. Built by the tool with the host compiler into a shared object.
#include <cstring>
#include <vector>

#include "route_plan.h"

extern "C" void route_host_loop(const onc_msg* msgs, const int32_t* status, uint64_t n, const onc_route* table,
                                uint32_t ntab, uint32_t nh, uint32_t* route, uint32_t* order, uint64_t* bin_first,
                                onc_msg* replies) {
    using namespace onc;
    const uint32_t bins = route_bins(nh);
    std::vector<uint64_t> at(bins + 1, 0);
    std::vector<RouteOutcome> out(n);
    for (uint64_t r = 0; r < n; ++r) {
        const onc_msg& m = msgs[r];
        RouteOutcome o{0, 0, 0, 0};
        if (status[r] == ONC_OK && m.msg_type == ONC_MSG_CALL)
            o = route_lookup(table, ntab, nh, m.u.call.program, m.u.call.program_version, m.u.call.procedure);
        out[r] = o;
        route[r] = route_bin(status[r], m.msg_type, o.bin, nh);
        ++at[route[r] + 1];
    }
    for (uint32_t b = 0; b < bins; ++b) at[b + 1] += at[b];
    for (uint32_t b = 0; b <= bins; ++b) bin_first[b] = at[b];
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t k = at[route[r]]++;
        order[k] = uint32_t(r);
        onc_msg& d = replies[k];
        std::memset(&d, 0, sizeof(d));
        if (route[r] > nh) continue;
        d.xid = msgs[r].xid;
        d.msg_type = ONC_MSG_REPLY;
        d.reply_stat = ONC_REPLY_ACCEPTED;
        d.stat = uint8_t(out[r].stat);
        d.u.mismatch.low = out[r].low;
        d.u.mismatch.high = out[r].high;
        d.verf.kind_len = ONC_AUTH_PACK(ONC_KIND_NONE, 0);
    }
}
