// test_fragment_streams.cpp — reassemble_streams and
// BatchDecoder::try_from_mixed_streams (include/onc_rpc.hpp) on a slab of
// connection buffers some of which hold multi-fragment records. The slab and
// its segment list are a file written by the test that runs this
// (tests/test_gpu_fragment_streams.py, -m gpu); what was reassembled and
// decoded goes to a second file, which that test compares with the host model
// and the oracle.
// Usage: test_fragment_streams <in> <out>
//   in : u64 nseg, u64 slab_len, u64 seg_off[nseg], u64 seg_len[nseg], slab bytes
//   out: reassemble_streams of every segment:
//          u64 n_rec, u64 n_frags, u64 n_multi, u64 n_bytes,
//          u64 rows[6 * nseg] {first_rec, n_rec, consumed, status, aux0, aux1},
//          u64 rec_off[n_rec + 1], i32 status[n_rec], the bytes;
//        then try_from_mixed_streams: per connection u64 n, u64 consumed,
//          u64 status, and per result i32 status, u32 xid, u32 payload length,
//          u32 FNV-1a of the payload
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

static uint32_t fnv1a(Bytes b) {
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < b.len; ++i) h = (h ^ b.ptr[i]) * 16777619u;
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
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_fragment_streams <in> <out>\n");
        return 2;
    }
    try {
        const std::vector<uint8_t> in = read_file(argv[1]);
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
        std::vector<uint8_t> out;
        std::vector<SegmentRecords> rows;
        const ReassembledStreams r = reassemble_streams(c, slab, slab_len, segs, &rows);
        CHECK(rows.size() == nseg && r.rec_off.size() == r.status.size() + 1 && r.rec_off.back() == r.bytes.size());
        put<uint64_t>(out, r.status.size());
        put<uint64_t>(out, r.n_frags);
        put<uint64_t>(out, r.n_multi);
        put<uint64_t>(out, r.bytes.size());
        uint64_t k = 0;
        for (const SegmentRecords& g : rows) {
            CHECK(g.first_rec == k && g.consumed <= segs[&g - rows.data()].len);
            k += g.n_rec;
            put<uint64_t>(out, g.first_rec);
            put<uint64_t>(out, g.n_rec);
            put<uint64_t>(out, g.consumed);
            put<uint64_t>(out, uint64_t(int64_t(g.status)));
            put<uint64_t>(out, g.aux0);
            put<uint64_t>(out, g.aux1);
        }
        CHECK(k == r.status.size());
        for (uint64_t o : r.rec_off) put<uint64_t>(out, o);
        for (int32_t s : r.status) put<int32_t>(out, s);
        out.insert(out.end(), r.bytes.begin(), r.bytes.end());

        BatchDecoder dec;
        const MixedStreams m = dec.try_from_mixed_streams(c, slab, slab_len, segs);
        CHECK(m.per_connection.size() == nseg && m.segments.size() == nseg);
        size_t total = 0;
        for (uint64_t i = 0; i < nseg; ++i) {
            const std::vector<Decoded>& list = m.per_connection[i];
            CHECK(m.segments[i].n == list.size() && m.segments[i].consumed <= segs[i].len);
            CHECK(m.segments[i].status != ONC_ERR_FRAGMENTED);
            total += list.size();
            put<uint64_t>(out, list.size());
            put<uint64_t>(out, m.segments[i].consumed);
            put<uint64_t>(out, uint64_t(int64_t(m.segments[i].status)));
            for (const Decoded& d : list) {
                const Bytes p = d.ok() ? payload_of(*d.message) : Bytes();
                // a payload view borrows the slab or the reassembled bytes
                if (p.len) {
                    const bool in_slab = p.ptr >= slab && p.ptr + p.len <= slab + slab_len;
                    const uint8_t* rb = m.reassembled.data();
                    CHECK(in_slab || (p.ptr >= rb && p.ptr + p.len <= rb + m.reassembled.size()));
                }
                put<int32_t>(out, d.status);
                put<uint32_t>(out, d.ok() ? d.message->xid() : 0u);
                put<uint32_t>(out, uint32_t(p.len));
                put<uint32_t>(out, fnv1a(p));
            }
        }

        // no segments, and a segment outside the slab
        CHECK(reassemble_streams(c, slab, slab_len, {}, &rows).bytes.empty() && rows.empty());
        CHECK(dec.try_from_mixed_streams(c, slab, slab_len, {}).per_connection.empty());
        bool threw = false;
        try {
            reassemble_streams(c, slab, slab_len, {Segment{slab_len - 4, 8}});
        } catch (const CodecError&) {
            threw = true;
        }
        CHECK(threw);

        std::ofstream f(argv[2], std::ios::binary);
        f.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
        CHECK(bool(f));
        std::printf("PASS test_fragment_streams: %zu segments, %zu records reassembled, %zu results\n", size_t(nseg),
                    r.status.size(), total);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_fragment_streams: %s\n", e.what());
        return 1;
    }
}
