// test_group.cpp — group_by_conn and GroupedSends::connection_streams
// (include/onc_rpc.hpp: onc_group_by_conn, onc_conn_extents) over a stream of
// records and the connection each goes out on: decoded with
// BatchDecoder::try_from_stream, grouped by connection, every connection's
// span checked against the decoded messages, the sent messages serialised in
// connection order through BatchEncoder and every connection's byte range taken
// from the offsets. The connection list and the stream are a file written by
// the test that runs this (tests/test_gpu_group.py, -m gpu); a summary goes to
// a second file, which that test compares with its model.
// Usage: test_group <in> <out>
//   in : u64 nconn, u64 nsrc, u64 nvia, u64 wire_len, nsrc x u32 connection,
//        nvia x u32 via (nvia == 0: item k is connection k), wire bytes: a
//        record per item
//   out: u64 n, u64 sent, u64 dropped, u64 active, u64 conn_first[nconn + 2],
//        u32 order[n], u32 xid of msgs[j] for j < n, (nconn + 1) x 2 u64 byte
//        ranges, u64 stream bytes, the stream
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
        std::fprintf(stderr, "usage: test_group <in> <out>\n");
        return 2;
    }
    try {
        const std::vector<uint8_t> in = read_file(argv[1]);
        CHECK(in.size() >= 32);
        uint64_t head[4];
        std::memcpy(head, in.data(), 32);
        const uint64_t nconn = head[0], nsrc = head[1], nvia = head[2], wire_len = head[3];
        CHECK(in.size() == 32 + 4 * nsrc + 4 * nvia + wire_len);
        std::vector<uint32_t> conn_of(nsrc), via(nvia);
        if (nsrc) std::memcpy(conn_of.data(), in.data() + 32, 4 * nsrc);
        if (nvia) std::memcpy(via.data(), in.data() + 32 + 4 * nsrc, 4 * nvia);
        const uint8_t* wire = in.data() + 32 + 4 * nsrc + 4 * nvia;

        Codec c;
        BatchDecoder dec;
        size_t consumed = 0;
        const std::vector<Decoded> results = dec.try_from_stream(c, wire, wire_len, DecodeMode::Slice, &consumed);
        CHECK(consumed == wire_len);
        const size_t n = results.size();
        CHECK(n == (nvia ? nvia : nsrc));
        std::vector<onc_msg> descs(n);
        for (size_t k = 0; k < n; ++k) {
            CHECK(results[k].ok());
            std::memset(&descs[k], 0, sizeof(onc_msg));
            descs[k].xid = results[k].message->xid();
            descs[k].payload_off = (uint64_t(k) << 33) | 5;           // carried untouched
        }
        const GroupedSends g = group_by_conn(c, conn_of, via, uint32_t(nconn), descs);
        CHECK(g.order.size() == n && g.msgs.size() == n && g.conn_first.size() == nconn + 2);
        CHECK(g.conn_first[0] == 0 && g.conn_first[nconn + 1] == n);
        CHECK(g.n_sent + g.n_dropped == n && g.dropped().n == g.n_dropped);

        // the connection of an item, on the host
        auto conn = [&](size_t k) -> uint64_t {
            const uint64_t s = nvia ? via[k] : k;
            return s < nsrc && conn_of[s] < nconn ? conn_of[s] : nconn;
        };
        size_t active = 0, seen = 0;
        for (uint32_t cc = 0; cc <= nconn; ++cc) {
            const GroupedSends::Span s = cc < nconn ? g.of(cc) : g.dropped();
            active += cc < nconn && s.n;
            seen += s.n;
            for (size_t k = 0; k < s.n; ++k) {
                CHECK(k == 0 || s.index[k] > s.index[k - 1]);             // the order the items were given in
                CHECK(conn(s.index[k]) == cc);
                CHECK(std::memcmp(&s.msgs[k], &descs[s.index[k]], sizeof(onc_msg)) == 0);
            }
        }
        CHECK(seen == n && active == g.active());
        CHECK(throws([&] { g.of(uint32_t(nconn)); }));

        // the sent messages serialised in connection order; every connection's bytes
        BatchEncoder enc;
        for (size_t j = 0; j < g.n_sent; ++j) enc.push(*results[g.order[j]].message);
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> rec_off(1, 0);
        if (g.n_sent) {
            const std::vector<int32_t> est = enc.serialise_into(c, bytes, &rec_off);
            for (int32_t s : est) CHECK(s == ONC_OK);
        }
        CHECK(rec_off.size() == g.n_sent + 1 && rec_off[g.n_sent] == bytes.size());
        const std::vector<std::pair<uint64_t, uint64_t>> streams = g.connection_streams(c, rec_off);
        CHECK(streams.size() == nconn + 1);
        uint64_t at = 0;
        for (uint32_t cc = 0; cc <= nconn; ++cc) {
            CHECK(streams[cc].first == at && streams[cc].second >= at);    // the ranges tile the stream
            at = streams[cc].second;
            const GroupedSends::Span s = cc < nconn ? g.of(cc) : g.dropped();
            uint64_t want = 0;
            if (cc < nconn)
                for (size_t k = 0; k < s.n; ++k) want += results[s.index[k]].message->serialised_len(c);
            CHECK(streams[cc].second - streams[cc].first == want);          // (the dropped group: nothing encoded)
        }
        CHECK(at == bytes.size());

        // without via and descriptors; no items; what the host refuses
        if (nsrc) {
            const GroupedSends plain = group_by_conn(c, conn_of, {}, uint32_t(nconn));
            CHECK(plain.order.size() == nsrc && plain.msgs.empty() && plain.group(0).msgs == nullptr);
        }
        const GroupedSends none = group_by_conn(c, {}, {}, uint32_t(nconn));
        CHECK(none.order.empty() && none.conn_first.size() == nconn + 2 && none.active() == 0 && none.n_dropped == 0);
        for (uint64_t v : none.conn_first) CHECK(v == 0);
        CHECK(throws([&] { group_by_conn(c, conn_of, via, ONC_GROUP_CONN_MAX + 1); }));
        CHECK(throws([&] { group_by_conn(c, conn_of, via, uint32_t(nconn), std::vector<onc_msg>(n + 1)); }));
        CHECK(throws([&] { g.connection_streams(c, {}); }));

        std::vector<uint8_t> out;
        put<uint64_t>(out, n);
        put<uint64_t>(out, g.n_sent);
        put<uint64_t>(out, g.n_dropped);
        put<uint64_t>(out, g.active());
        for (uint64_t v : g.conn_first) put<uint64_t>(out, v);
        for (uint32_t v : g.order) put<uint32_t>(out, v);
        for (const onc_msg& d : g.msgs) put<uint32_t>(out, d.xid);
        for (const auto& r : streams) {
            put<uint64_t>(out, r.first);
            put<uint64_t>(out, r.second);
        }
        put<uint64_t>(out, bytes.size());
        out.insert(out.end(), bytes.begin(), bytes.end());
        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
        CHECK(bool(o));
        std::printf("PASS test_group: %zu items, %zu sent on %zu of %llu connections, %zu dropped\n", n, g.n_sent,
                    g.active(), (unsigned long long)nconn, g.n_dropped);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_group: %s\n", e.what());
        return 1;
    }
}
