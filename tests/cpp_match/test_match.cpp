// test_match.cpp — PendingCalls, match_replies and MatchedReplies
// (include/onc_rpc.hpp: onc_match_replies) over a stream of records: decoded
// with BatchDecoder::try_from_stream, paired with a pending list, then paired
// again with what the first round left waiting (MatchedReplies::still). The
// list, the records' connections and the stream are a file written by the
// test that runs this (tests/test_gpu_match.py, -m gpu); both rounds go to a
// second file, which that test compares with its model.
// Usage: test_match <in> <out>
//   in : u64 np, u64 n, u64 wire_len, np x (u32 conn, u32 xid, u64 tag),
//        n x u32 conn, wire bytes
//   out: per round: u64 n, u64 np, u32 match[n], u64 tag[n], u32 hit[np],
//        u64 counts[5], u64 k, k x (u32 conn, u32 xid, u64 tag)
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

static void put_round(std::vector<uint8_t>& out, const MatchedReplies& m) {
    put<uint64_t>(out, m.match.size());
    put<uint64_t>(out, m.hit.size());
    for (uint32_t v : m.match) put<uint32_t>(out, v);
    for (uint64_t v : m.tag) put<uint64_t>(out, v);
    for (uint32_t v : m.hit) put<uint32_t>(out, v);
    for (size_t v : {m.n_matched, m.n_unknown, m.n_duplicate, m.n_not_reply, m.n_failed}) put<uint64_t>(out, v);
    put<uint64_t>(out, m.still().size());
    for (const onc_pending& e : m.still().list()) {
        put<uint32_t>(out, e.conn);
        put<uint32_t>(out, e.xid);
        put<uint64_t>(out, e.tag);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_match <in> <out>\n");
        return 2;
    }
    try {
        static_assert(sizeof(onc_pending) == 16, "onc_pending is 16 bytes");
        const std::vector<uint8_t> in = read_file(argv[1]);
        CHECK(in.size() >= 24);
        uint64_t np = 0, n = 0, wire_len = 0;
        std::memcpy(&np, in.data(), 8);
        std::memcpy(&n, in.data() + 8, 8);
        std::memcpy(&wire_len, in.data() + 16, 8);
        CHECK(in.size() == 24 + 16 * np + 4 * n + wire_len);
        PendingCalls pending;
        for (uint64_t p = 0; p < np; ++p) {
            uint32_t w[2];
            uint64_t tag;
            std::memcpy(w, in.data() + 24 + 16 * p, 8);
            std::memcpy(&tag, in.data() + 24 + 16 * p + 8, 8);
            pending.add(w[0], w[1], tag);
        }
        CHECK(pending.size() == np);
        std::vector<uint32_t> conns(n);
        if (n) std::memcpy(conns.data(), in.data() + 24 + 16 * np, 4 * n);
        const uint8_t* wire = in.data() + 24 + 16 * np + 4 * n;

        Codec c;
        BatchDecoder dec;
        size_t consumed = 0;
        const std::vector<Decoded> results = dec.try_from_stream(c, wire, wire_len, DecodeMode::Slice, &consumed);
        CHECK(consumed == wire_len && results.size() == n);
        const MatchedReplies first = match_replies(c, results, conns, pending);
        CHECK(first.match.size() == n && first.tag.size() == n && first.hit.size() == np);
        CHECK(first.n_matched + first.n_unknown + first.n_duplicate + first.n_not_reply + first.n_failed == n);
        size_t answered = 0;
        for (size_t p = 0; p < np; ++p) {
            if (!first.answered(p)) continue;
            ++answered;
            const size_t r = first.hit[p];
            CHECK(r < n && first.match[r] == p && first.matched(r) && first.tag[r] == pending.list()[p].tag);
            CHECK(results[r].message->reply_body() && results[r].message->xid() == pending.list()[p].xid &&
                  conns[r] == pending.list()[p].conn);
        }
        CHECK(answered == first.n_matched && first.still().size() == np - answered);
        // the same batch again over what is left: what a repeated key kept back is answered now
        const MatchedReplies second = match_replies(c, results, conns, first.still());
        CHECK(second.hit.size() == first.still().size());

        // no records; no list; a connection count that does not fit
        const MatchedReplies none = match_replies(c, {}, {}, pending);
        CHECK(none.match.empty() && none.hit.size() == np && none.still().size() == np && none.n_matched == 0);
        for (size_t p = 0; p < np; ++p) CHECK(!none.answered(p));
        const MatchedReplies lost = match_replies(c, results, conns, PendingCalls());
        CHECK(lost.n_matched == 0 && lost.n_duplicate == 0 && lost.still().empty() && lost.hit.empty());
        bool threw = false;
        try {
            (void)match_replies(c, results, std::vector<uint32_t>(n + 1, 0u), pending);
        } catch (const CodecError&) {
            threw = true;
        }
        CHECK(threw);

        std::vector<uint8_t> out;
        put_round(out, first);
        put_round(out, second);
        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
        CHECK(bool(o));
        std::printf("PASS test_match: %zu records, %zu of %llu entries answered, then %zu of %zu\n", size_t(n),
                    first.n_matched, (unsigned long long)np, second.n_matched, first.still().size());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_match: %s\n", e.what());
        return 1;
    }
}
