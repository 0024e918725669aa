// xdr_host_loop.cpp — the route onc_xdr_unpack replaces, for
// tools/xdr_unpack_timing.py: one thread walks the descriptors and parses every
// payload on the host with the same parse the kernel runs
// (onc-rpc_amd/csrc/xdr_plan.h xdr_parse), writing the same outputs.
#include <cstdint>
#include <cstring>

#include "xdr_plan.h"

using namespace onc;

namespace {

struct HostReader {
    const uint8_t* pay;
    uint32_t word(uint64_t p) const {
        uint32_t v;
        std::memcpy(&v, pay + p, 4);
        return __builtin_bswap32(v);
    }
};

struct HostSink {
    uint8_t* cols;
    uint64_t r, n;
    void put32(const onc_xdr_field& f, uint32_t v) const {
        if (xdr_has_column(f.type_flags)) std::memcpy(cols + f.col_off + 4 * r, &v, 4);
    }
    void put64(const onc_xdr_field& f, uint64_t v) const {
        if (xdr_has_column(f.type_flags)) std::memcpy(cols + f.col_off + 8 * r, &v, 8);
    }
    void put_pair(const onc_xdr_field& f, uint32_t pos, uint32_t len) const {
        if (!xdr_has_column(f.type_flags)) return;
        std::memcpy(cols + f.col_off + 4 * r, &pos, 4);
        std::memcpy(cols + f.col_off + 4 * n + 4 * r, &len, 4);
    }
};

}  // namespace

extern "C" void xdr_host_loop(const uint8_t* wire, uint64_t wire_len, const onc_msg* msgs, const int32_t* status,
                              uint64_t n, const uint64_t* rec_start, const onc_xdr_field* fields, uint32_t nf,
                              uint32_t flags, uint8_t* cols, uint32_t* xstat, uint64_t* present, uint32_t* rest_pos,
                              uint32_t* rest_len, uint64_t* result) {
    uint64_t count[3] = {0, 0, 0};
    for (uint64_t r = 0; r < n; ++r) {
        uint32_t code = ONC_XDR_SKIPPED;
        uint64_t o = 0, L = 0;
        XdrExtent e{false, 0, 0};
        if (status[r] == ONC_OK) {
            const onc_msg& m = msgs[r];
            const uint32_t kinds = uint32_t(m.msg_type) | uint32_t(m.reply_stat) << 8 | uint32_t(m.stat) << 16;
            if (xdr_carries(status[r], kinds)) {
                o = m.payload_off;
                L = m.payload_len;
                e = xdr_extent(o, L, r, false, 0, rec_start != nullptr, rec_start ? rec_start[r] : 0, wire_len);
                code = e.bad ? ONC_XDR_BAD_EXTENT : ONC_XDR_OK;
            }
        }
        HostReader rd{wire + (code == ONC_XDR_OK ? o : 0)};
        const HostSink sink{cols, r, n};
        const XdrParsed out = xdr_parse(fields, nf, flags, code, o, L, e, false, rd, sink);
        const bool ok = out.code == ONC_XDR_OK;
        xstat[r] = out.code | (out.fail << 8);
        present[r] = out.present;
        rest_pos[r] = ok ? uint32_t(e.base + out.p) : 0u;
        rest_len[r] = ok ? uint32_t(L - out.p) : 0u;
        ++count[ok ? 0 : ((out.code >= ONC_XDR_SHORT && out.code <= ONC_XDR_TRAILING) ? 1 : 2)];
    }
    result[0] = count[0];
    result[1] = count[1];
    result[2] = count[2];
    result[3] = 0;
}
