// test_payload.cpp — FragmentedHeads::place_payloads and place_payloads
// (include/onc_rpc.hpp: onc_payload_slots + onc_place_payloads) on a slab of
// connection buffers holding fragmented records: every payload placed in an
// aligned slot of a device buffer, fetched back and compared with the payload
// gathered on the host (FragmentedHeads::payload), and the records of the
// connections that do not fragment placed from try_from_streams' results and
// compared with their payload views. The slab and its segment list are a file
// written by the test that runs this (tests/test_gpu_payload.py, -m gpu); a
// summary goes to a second file, which that test compares with what it built.
// Usage: test_payload <in> <out> <align>
//   in : u64 nseg, u64 slab_len, u64 seg_off[nseg], u64 seg_len[nseg], slab bytes
//   out: u64 n_rec, u64 n_payloads, u64 payload_bytes, u64 capacity, u64 records
//        placed from try_from_streams, then per record i32 status, u32 xid, u32
//        payload length, u32 FNV-1a of the placed payload, u64 slot_off
#include <cstdio>
#include <cstdlib>
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

static uint32_t fnv1a(const uint8_t* p, size_t n) {
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

static Bytes payload_of(const RpcMessage& m) {
    if (const CallBody* cb = m.call_body()) return cb->payload();
    const ReplyBody* rb = m.reply_body();
    if (const AcceptedReply* a = rb->accepted())
        if (a->status().kind() == AcceptedStatus::Kind::Success) return a->status().payload();
    return Bytes();
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: test_payload <in> <out> <align>\n");
        return 2;
    }
    try {
        const std::vector<uint8_t> in = read_file(argv[1]);
        const uint32_t align = uint32_t(std::strtoul(argv[3], nullptr, 10));
        CHECK(in.size() >= 16);
        uint64_t nseg = 0, slab_len = 0;
        std::memcpy(&nseg, in.data(), 8);
        std::memcpy(&slab_len, in.data() + 8, 8);
        CHECK(in.size() == 16 + 16 * nseg + slab_len);
        std::vector<Segment> segs(nseg);
        for (uint64_t i = 0; i < nseg; ++i) {
            std::memcpy(&segs[i].off, in.data() + 16 + 8 * i, 8);
            std::memcpy(&segs[i].len, in.data() + 16 + 8 * (nseg + i), 8);
        }
        const uint8_t* slab = in.data() + 16 + 16 * nseg;

        Codec c;
        BatchDecoder dec;
        const FragmentedHeads f = dec.try_from_fragmented_heads(c, slab, slab_len, segs);
        const size_t n = f.results.size();
        CHECK(f.descriptors.size() == n && f.status.size() == n);
        const PlacedPayloads p = f.place_payloads(c, align);
        CHECK(p.views.size() == n && p.slot_off.size() == n + 1 && p.align == align);
        CHECK(p.slot_off[0] == 0 && p.slot_off[n] == p.bytes);

        std::vector<uint8_t> out;
        put<uint64_t>(out, n);
        put<uint64_t>(out, p.n_payloads);
        put<uint64_t>(out, p.payload_bytes);
        put<uint64_t>(out, p.bytes);
        const size_t streams_at = out.size();
        put<uint64_t>(out, 0);
        size_t with = 0;
        uint64_t total = 0;
        for (size_t r = 0; r < n; ++r) {
            const Decoded& a = f.results[r];
            std::vector<uint8_t> placed;
            if (a.ok()) {
                const std::vector<uint8_t> want = f.payload(r);           // gathered on the host
                CHECK(p.views[r].len == want.size());
                placed = p.fetch(r);
                CHECK(placed == want);
                if (!want.empty()) {
                    ++with;
                    total += want.size();
                    CHECK(p.views[r].ptr == p.dev + p.slot_off[r] && p.slot_off[r] % align == 0);
                    CHECK(p.slot_off[r + 1] == ((p.slot_off[r] + want.size() + align - 1) / align) * align);
                } else {
                    CHECK(p.slot_off[r + 1] == p.slot_off[r]);
                }
            } else {
                CHECK(p.views[r].len == 0 && p.slot_off[r + 1] == p.slot_off[r]);
            }
            put<int32_t>(out, a.status);
            put<uint32_t>(out, a.ok() ? a.message->xid() : 0u);
            put<uint32_t>(out, uint32_t(placed.size()));
            put<uint32_t>(out, fnv1a(placed.data(), placed.size()));
            put<uint64_t>(out, p.slot_off[r]);
        }
        CHECK(with == p.n_payloads && total == p.payload_bytes);

        // the connections that do not fragment: decoded in place, then placed
        std::vector<SegmentResult> per;
        const std::vector<Decoded> plain = dec.try_from_streams(c, slab, slab_len, segs, &per);
        const PlacedPayloads q = place_payloads(c, slab, slab_len, plain, align);
        CHECK(q.views.size() == plain.size());
        uint64_t placed_plain = 0;
        for (size_t r = 0; r < plain.size(); ++r) {
            if (!plain[r].ok()) {
                CHECK(q.views[r].len == 0);
                continue;
            }
            const Bytes want = payload_of(*plain[r].message);
            CHECK(q.views[r].len == want.len);
            if (!want.len) continue;
            CHECK(q.slot_off[r] % align == 0 && q.fetch(r) == want.to_vec());
            ++placed_plain;
        }
        CHECK(placed_plain == q.n_payloads);
        std::memcpy(out.data() + streams_at, &placed_plain, 8);

        // no records, and a bad alignment
        CHECK(place_payloads(c, slab, slab_len, {}, align).bytes == 0);
        CHECK(FragmentedHeads().place_payloads(c, align).views.empty());
        int threw = 0;
        try {
            f.place_payloads(c, 24);
        } catch (const CodecError&) {
            ++threw;
        }
        CHECK(threw == 1);

        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
        CHECK(bool(o));
        std::printf("PASS test_payload: %zu records, %zu payloads in %llu bytes at align %u, %llu placed in place\n", n,
                    p.n_payloads, (unsigned long long)p.bytes, align, (unsigned long long)placed_plain);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_payload: %s\n", e.what());
        return 1;
    }
}
