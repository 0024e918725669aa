// test_route.cpp — RouteTable, route_calls and RoutedCalls::reject_replies
// (include/onc_rpc.hpp: onc_route_calls) over a stream of records: decoded with
// BatchDecoder::try_from_stream, dispatched against a table whose rows arrive
// unsorted, every handler's span checked against the decoded messages, the
// rejected Calls' replies serialised through BatchEncoder and decoded again.
// The table and the stream are a file written by the test that runs this
// (tests/test_gpu_route.py, -m gpu); a summary goes to a second file, which
// that test compares with its model.
// Usage: test_route <in> <out>
//   in : u64 nh, u64 rows, u64 wire_len, rows x 6 u32 (program, version,
//        proc_first, proc_count, handler_first, flags), wire bytes
//   out: u64 n, u64 bins, u64 bin_first[nh + 4], u32 order[n], u32 xid of
//        calls[k] for k < n, u64 reply bytes, the rejected Calls' replies
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/onc_rpc.hpp"

using namespace onc_rpc;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            throw std::runtime_error("check failed");                                    \
        }                                                                                \
    } while (0)

static std::vector<uint8_t> read_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

template <class T>
static void put(std::vector<uint8_t>& out, T v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    out.insert(out.end(), p, p + sizeof(T));
}

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const CodecError&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_route <in> <out>\n");
        return 2;
    }
    try {
        const std::vector<uint8_t> in = read_file(argv[1]);
        CHECK(in.size() >= 24);
        uint64_t nh = 0, nrows = 0, wire_len = 0;
        std::memcpy(&nh, in.data(), 8);
        std::memcpy(&nrows, in.data() + 8, 8);
        std::memcpy(&wire_len, in.data() + 16, 8);
        CHECK(in.size() == 24 + 24 * nrows + wire_len);
        RouteTable table{uint32_t(nh)};
        for (uint64_t i = 0; i < nrows; ++i) {
            uint32_t w[6];
            std::memcpy(w, in.data() + 24 + 24 * i, 24);
            table.add(w[0], w[1], w[2], w[3], w[4], w[5]);
        }
        const uint8_t* wire = in.data() + 24 + 24 * nrows;
        const std::vector<onc_route> sorted = table.sorted();
        CHECK(sorted.size() == nrows && table.n_handlers() == nh);

        Codec c;
        BatchDecoder dec;
        size_t consumed = 0;
        const std::vector<Decoded> results = dec.try_from_stream(c, wire, wire_len, DecodeMode::Slice, &consumed);
        CHECK(consumed == wire_len);
        const size_t n = results.size();
        const RoutedCalls routed = route_calls(c, results, table);
        CHECK(routed.order.size() == n && routed.bin_first.size() == nh + 4 && routed.bin_first[nh + 3] == n);
        CHECK(routed.n_served + routed.n_rejected + routed.n_other == n);
        CHECK(routed.rejected().n == routed.n_rejected && routed.failed().n == 0);

        // the handler of a Call, on the host, from the sorted rows
        auto handler_of = [&](const CallBody& cb) -> int64_t {
            for (const onc_route& e : sorted)
                if (e.program == cb.program() && e.version == cb.program_version() && cb.procedure() >= e.proc_first &&
                    uint64_t(cb.procedure()) < uint64_t(e.proc_first) + e.proc_count)
                    return e.handler_first + ((e.flags & ONC_ROUTE_ONE_HANDLER) ? 0 : cb.procedure() - e.proc_first);
            return -1;
        };
        size_t served = 0;
        for (uint32_t h = 0; h < nh; ++h) {
            const RoutedCalls::Span s = routed.handler(h);
            served += s.n;
            for (size_t k = 0; k < s.n; ++k) {
                CHECK(k == 0 || s.index[k] > s.index[k - 1]);             // arrival order
                const RpcMessage& m = *results[s.index[k]].message;
                CHECK(m.call_body() && handler_of(*m.call_body()) == int64_t(h));
                CHECK(s.calls[k].xid == m.xid() && s.calls[k].u.call.procedure == m.call_body()->procedure());
                CHECK(s.replies[k].xid == m.xid() && s.replies[k].msg_type == ONC_MSG_REPLY &&
                      s.replies[k].stat == ONC_ACCEPT_SUCCESS);
            }
        }
        CHECK(served == routed.n_served);
        const RoutedCalls::Span rej = routed.rejected();
        for (size_t k = 0; k < rej.n; ++k) {
            const RpcMessage& m = *results[rej.index[k]].message;
            CHECK(m.call_body() && handler_of(*m.call_body()) < 0 && rej.replies[k].stat != ONC_ACCEPT_SUCCESS);
        }
        const RoutedCalls::Span other = routed.not_calls();
        for (size_t k = 0; k < other.n; ++k) CHECK(results[other.index[k]].message->reply_body());

        // the rejections, serialised and decoded again
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> rec_off;
        const std::vector<int32_t> est = routed.reject_replies(c, bytes, &rec_off);
        CHECK(est.size() == rej.n && rec_off.size() == rej.n + 1 && rec_off[rej.n] == bytes.size());
        for (int32_t s : est) CHECK(s == ONC_OK);
        const std::vector<Decoded> back = dec.try_from_stream(c, bytes.data(), bytes.size());
        CHECK(back.size() == rej.n);
        for (size_t k = 0; k < rej.n; ++k) {
            CHECK(back[k].ok() && back[k].message->xid() == rej.calls[k].xid);
            const AcceptedReply* a = back[k].message->reply_body()->accepted();
            CHECK(a && uint32_t(a->status().kind()) == rej.replies[k].stat);
            if (a->status().kind() == AcceptedStatus::Kind::ProgramMismatch)
                CHECK(a->status().mismatch().first == rej.replies[k].u.mismatch.low &&
                      a->status().mismatch().second == rej.replies[k].u.mismatch.high);
        }

        // no records; an empty table (every Call rejected); tables the host refuses
        const RoutedCalls none = route_calls(c, {}, table);
        CHECK(none.order.empty() && none.bin_first.size() == nh + 4 && none.rejected().n == 0);
        std::vector<uint8_t> nothing;
        CHECK(none.reject_replies(c, nothing).empty() && nothing.empty());
        const RoutedCalls all = route_calls(c, results, RouteTable(0));
        CHECK(all.n_served == 0 && all.n_rejected + all.n_other == n && all.bin_first.size() == 4);
        CHECK(throws([] { RouteTable(254); }));
        CHECK(throws([] { RouteTable(4).add(1, 1, 0, 3, 0).add(1, 1, 2, 1, 3).sorted(); }));       // overlap
        CHECK(throws([] { RouteTable(4).add(1, 1, 0, 0, 0).sorted(); }));                           // empty range
        CHECK(throws([] { RouteTable(4).add(1, 1, 0xFFFFFFFFu, 2, 0, 1).sorted(); }));              // wraps
        CHECK(throws([] { RouteTable(4).add(1, 1, 0, 5, 0).sorted(); }));                           // handler 4 of 4
        CHECK(throws([] { RouteTable(4).add(1, 1, 0, 1, 0, 2).sorted(); }));                        // flags
        CHECK(!throws([] { RouteTable(4).add(1, 1, 3, 1, 3).add(1, 1, 0, 3, 0).add(0, 9, 0, 9, 3, 1).sorted(); }));

        std::vector<uint8_t> out;
        put<uint64_t>(out, n);
        put<uint64_t>(out, nh + 3);
        for (uint64_t v : routed.bin_first) put<uint64_t>(out, v);
        for (uint32_t v : routed.order) put<uint32_t>(out, v);
        for (const onc_msg& d : routed.calls) put<uint32_t>(out, d.xid);
        put<uint64_t>(out, bytes.size());
        out.insert(out.end(), bytes.begin(), bytes.end());
        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
        CHECK(bool(o));
        std::printf("PASS test_route: %zu records, %zu served by %llu handlers, %zu rejected, %zu other\n", n,
                    routed.n_served, (unsigned long long)nh, routed.n_rejected, routed.n_other);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_route: %s\n", e.what());
        return 1;
    }
}
