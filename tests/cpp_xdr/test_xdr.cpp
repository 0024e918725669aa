// test_xdr.cpp — XdrSchema, unpack_args and UnpackedArgs (include/onc_rpc.hpp:
// onc_xdr_unpack) over a stream of records: decoded with
// BatchDecoder::try_from_stream, dispatched with route_calls to two handlers
// (procedure 7: WRITE-shaped arguments, procedure 2: an optional and a
// three-way union), each handler's arguments unpacked against its schema, the
// bodies checked against the decoded payloads, the GARBAGE_ARGS answers
// serialised through BatchEncoder and decoded again. The stream is a file
// written by the test that runs this (tests/test_gpu_xdr.py, -m gpu); a summary
// goes to a second file, which that test compares with its model.
// Usage: test_xdr <in> <out>
//   in : the stream's bytes
//   out: per handler (WRITE, then the other): u64 n, then per record u32 index
//        in the decoded batch, u32 xstat, u64 present, u32 rest_pos, u32
//        rest_len, u32 reply stat, then the handler's columns: WRITE {u32 fh
//        pos, u32 fh len, u64 offset, u32 count, u32 stable, u32 data pos, u32
//        data len}; the other {u32 set_it, u64 size, u32 how, u32 sec, u32 nsec}
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

static void put_common(std::vector<uint8_t>& out, const RoutedCalls::Span& s, const UnpackedArgs& a, size_t k) {
    put<uint32_t>(out, s.index[k]);
    put<uint32_t>(out, a.xstat[k]);
    put<uint64_t>(out, a.present[k]);
    put<uint32_t>(out, a.rest_pos[k]);
    put<uint32_t>(out, a.rest_len[k]);
    put<uint32_t>(out, a.replies[k].stat);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_xdr <in> <out>\n");
        return 2;
    }
    try {
        const std::vector<uint8_t> wire = read_file(argv[1]);
        Codec c;
        BatchDecoder dec;
        size_t consumed = 0;
        const std::vector<Decoded> results = dec.try_from_stream(c, wire.data(), wire.size(), DecodeMode::Slice, &consumed);
        CHECK(consumed == wire.size());
        RouteTable table{2};
        table.add(100003, 3, 7, 1, 0).add(100003, 3, 2, 1, 1);
        const RoutedCalls routed = route_calls(c, results, table);

        XdrSchema write;            // WRITE3args: file, offset, count, stable, data
        write.opaque(64).u64().u32().u32().opaque(0xFFFFFFFFu);
        XdrSchema other;            // a file handle nobody stores, an optional size, a time_how union
        other.opaque(64).skip().boolean().select().u64().when(1).u32().select().u32().when(2).u32().when(2);
        CHECK(write.size() == 5 && other.size() == 6);

        std::vector<uint8_t> out;
        size_t garbage = 0;
        {
            const RoutedCalls::Span s = routed.handler(0);
            const UnpackedArgs a = unpack_args(c, wire.data(), wire.size(), results, s, write, ONC_XDR_EXACT);
            CHECK(a.n == s.n && a.n_ok + a.n_garbage + a.n_other == s.n && a.n_other == 0);
            put<uint64_t>(out, a.n);
            const uint32_t* fh_pos = a.column<uint32_t>(0);
            const uint64_t* offset = a.column<uint64_t>(1);
            const uint32_t* count = a.column<uint32_t>(2);
            const uint32_t* stable = a.column<uint32_t>(3);
            const uint32_t* data_pos = a.column<uint32_t>(4);
            CHECK(throws([&] { a.column<uint64_t>(0); }) && throws([&] { a.column<uint32_t>(1); }));
            CHECK(throws([&] { a.lengths(2); }) && throws([&] { a.bytes(3, 0); }) && throws([&] { a.column<uint32_t>(5); }));
            for (size_t k = 0; k < a.n; ++k) {
                const Bytes pay = results[s.index[k]].message->call_body()->payload();
                CHECK(a.payloads[k].ptr == pay.ptr && a.payloads[k].len == pay.len);
                CHECK(a.replies[k].xid == s.calls[k].xid && a.replies[k].msg_type == ONC_MSG_REPLY);
                CHECK(a.replies[k].stat == (a.ok(k) ? ONC_ACCEPT_SUCCESS : ONC_ACCEPT_GARBAGE_ARGS));
                garbage += !a.ok(k);
                if (a.ok(k)) {
                    // the bodies are where the columns say, inside the decoded payload
                    const Bytes fh = a.bytes(0, k), data = a.bytes(4, k);
                    CHECK(fh.ptr == pay.ptr + 4 && fh.len == a.lengths(0)[k] && fh_pos[k] == 4);
                    CHECK(data.len == count[k] && data.ptr + ((data.len + 3) & ~size_t(3)) == pay.ptr + pay.len);
                    CHECK(a.rest_pos[k] == pay.len && a.rest_len[k] == 0 && a.present[k] == 31);
                } else {
                    // (trailing bytes fail at field 5, behind the last: its columns stay)
                    CHECK(a.failed_field(k) <= 5 && a.rest_pos[k] == 0 && a.has(4, k) == (a.code(k) == ONC_XDR_TRAILING));
                    CHECK(a.bytes(4, k).empty() == !a.has(4, k) || a.lengths(4)[k] == 0);
                }
                put_common(out, s, a, k);
                put<uint32_t>(out, fh_pos[k]);
                put<uint32_t>(out, a.lengths(0)[k]);
                put<uint64_t>(out, offset[k]);
                put<uint32_t>(out, count[k]);
                put<uint32_t>(out, stable[k]);
                put<uint32_t>(out, data_pos[k]);
                put<uint32_t>(out, a.lengths(4)[k]);
            }
            CHECK(garbage == a.n_garbage);
            // the answers to the Calls that did not parse, serialised and decoded again
            BatchEncoder enc;
            size_t sent = 0;
            for (size_t k = 0; k < a.n; ++k)
                if (!a.ok(k)) {
                    enc.push(RpcMessage(a.replies[k].xid, MessageType::reply(ReplyBody::accepted(AcceptedReply(
                                                              AuthFlavor::none(), AcceptedStatus::of(AcceptedStatus::Kind::GarbageArgs))))));
                    ++sent;
                }
            if (sent) {
                std::vector<uint8_t> bytes;
                const std::vector<int32_t> est = enc.serialise_into(c, bytes);
                const std::vector<Decoded> back = dec.try_from_stream(c, bytes.data(), bytes.size());
                CHECK(est.size() == sent && back.size() == sent);
                for (const Decoded& d : back)
                    CHECK(d.ok() && d.message->reply_body()->accepted()->status().kind() == AcceptedStatus::Kind::GarbageArgs);
            }
        }
        {
            const RoutedCalls::Span s = routed.handler(1);
            const UnpackedArgs a = unpack_args(c, wire.data(), wire.size(), results, s, other);
            CHECK(a.n == s.n);
            put<uint64_t>(out, a.n);
            CHECK(throws([&] { a.column<uint32_t>(0); }));                       // skipped: no column
            for (size_t k = 0; k < a.n; ++k) {
                CHECK(a.replies[k].stat == (a.code(k) >= ONC_XDR_SHORT && a.code(k) <= ONC_XDR_TRAILING
                                                ? ONC_ACCEPT_GARBAGE_ARGS
                                                : ONC_ACCEPT_SUCCESS));
                if (a.ok(k)) CHECK(a.has(2, k) == (a.column<uint32_t>(1)[k] == 1) && a.has(4, k) == (a.column<uint32_t>(3)[k] == 2));
                put_common(out, s, a, k);
                put<uint32_t>(out, a.column<uint32_t>(1)[k]);
                put<uint64_t>(out, a.column<uint64_t>(2)[k]);
                put<uint32_t>(out, a.column<uint32_t>(3)[k]);
                put<uint32_t>(out, a.column<uint32_t>(4)[k]);
                put<uint32_t>(out, a.column<uint32_t>(5)[k]);
            }
        }
        // the whole decoded list against one schema: records that are no Calls are skipped
        const UnpackedArgs all = unpack_args(c, wire.data(), wire.size(), results, write);
        CHECK(all.n == results.size() && all.n_ok + all.n_garbage + all.n_other == all.n);
        for (size_t r = 0; r < all.n; ++r)
            if (!results[r].ok() || !results[r].message->call_body()) CHECK(all.code(r) == ONC_XDR_SKIPPED);
        // no records; schemas the host refuses
        const UnpackedArgs none = unpack_args(c, wire.data(), wire.size(), {}, write);
        CHECK(none.n == 0 && none.cols.empty() && none.n_ok == 0);
        uint64_t cap = 0;
        CHECK(throws([&] { XdrSchema().u32().when(1).layout(4, &cap); }));       // IF without a selector
        CHECK(throws([&] { XdrSchema().u64().select().layout(4, &cap); }));      // SELECT on a hyper
        CHECK(throws([] { XdrSchema().select(); }));
        CHECK(throws([] {
            XdrSchema s;
            for (int i = 0; i < 65; ++i) s.u32();
        }));
        const std::vector<onc_xdr_field> f = XdrSchema().u32().u64().opaque(9).boolean().skip().layout(3, &cap);
        CHECK(f[0].col_off == 0 && f[1].col_off == 16 && f[2].col_off == 40 && f[3].col_off == 0 && cap == 64);

        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
        CHECK(bool(o));
        std::printf("PASS test_xdr: %zu records, %zu WRITE calls (%zu garbage), %zu others\n", results.size(),
                    routed.handler(0).n, garbage, routed.handler(1).n);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_xdr: %s\n", e.what());
        return 1;
    }
}
