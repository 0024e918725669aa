// test_heads.cpp — reassemble_heads and BatchDecoder::try_from_fragmented_heads
// (include/onc_rpc.hpp) on a slab of connection buffers holding fragmented
// records, checked against BatchDecoder::try_from_mixed_streams — the copying
// path — on the same slab: the same results per connection, and every payload,
// gathered from its slices of the caller's slab, byte for byte the one the
// copying path returns. The slab and its segment list are a file written by
// the test that runs this (tests/test_gpu_heads.py, -m gpu); a summary goes to
// a second file, which that test compares with what it built.
// Usage: test_heads <in> <out>
//   in : u64 nseg, u64 slab_len, u64 seg_off[nseg], u64 seg_len[nseg], slab bytes
//   out: u64 n_rec, u64 n_frags, u64 n_multi, u64 retried, u64 head_len used,
//        then per record i32 status, u32 xid, u32 payload length, u32 FNV-1a of
//        the gathered payload, u32 number of payload pieces
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

static std::vector<uint8_t> serialised(Codec& c, const RpcMessage& m) { return m.serialise(c); }

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_heads <in> <out>\n");
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
        BatchDecoder dec;
        const MixedStreams m = dec.try_from_mixed_streams(c, slab, slab_len, segs);
        const FragmentedHeads f = dec.try_from_fragmented_heads(c, slab, slab_len, segs);
        CHECK(f.segments.size() == nseg && m.per_connection.size() == nseg);
        CHECK(f.results.size() == f.heads.n() && f.payload_pos.size() == f.results.size());
        CHECK(f.heads.head_len == (f.retried ? 736u : 160u));

        std::vector<uint8_t> out;
        put<uint64_t>(out, f.results.size());
        put<uint64_t>(out, f.heads.n_frags());
        put<uint64_t>(out, f.heads.n_multi);
        put<uint64_t>(out, f.retried ? 1 : 0);
        put<uint64_t>(out, f.heads.head_len);
        uint64_t k = 0;
        for (uint64_t s = 0; s < nseg; ++s) {
            const SegmentRecords& g = f.segments[s];
            const std::vector<Decoded>& want = m.per_connection[s];
            CHECK(g.first_rec == k && g.n_rec == want.size());
            CHECK(g.consumed == m.segments[s].consumed);
            for (uint64_t q = 0; q < g.n_rec; ++q, ++k) {
                const Decoded& a = f.results[k];
                const Decoded& b = want[q];
                CHECK(a.status == b.status && a.aux0 == b.aux0 && a.aux1 == b.aux1);
                CHECK(a.status != ONC_DEC_BAD_EXTENT);           // the retry leaves no HEAD_SHORT behind
                std::vector<uint8_t> pay;
                size_t pieces = 0;
                if (a.ok()) {
                    CHECK(a.message->xid() == b.message->xid());
                    const Bytes bp = payload_of(*b.message);
                    const std::vector<Bytes> ps = f.payload_pieces(k);
                    pieces = ps.size();
                    size_t total = 0;
                    for (const Bytes& p : ps) {
                        // every piece is a slice of the caller's slab: nothing was copied
                        CHECK(p.len != 0 && p.ptr >= slab && p.ptr + p.len <= slab + slab_len);
                        total += p.len;
                    }
                    pay = f.payload(k);
                    CHECK(total == bp.len && pay.size() == bp.len && f.payload_len[k] == bp.len);
                    CHECK(bp.len == 0 || std::memcmp(pay.data(), bp.ptr, bp.len) == 0);
                    // the message's own view: the part of the payload inside the head
                    const Bytes ap = payload_of(*a.message);
                    CHECK(ap.len <= bp.len && (ap.len == 0 || std::memcmp(ap.ptr, bp.ptr, ap.len) == 0));
                    // everything but the payload is the same message: put the
                    // whole payload back and it serialises to the same bytes
                    if (ap.len == bp.len) CHECK(serialised(c, *a.message) == serialised(c, *b.message));
                }
                put<int32_t>(out, a.status);
                put<uint32_t>(out, a.ok() ? a.message->xid() : 0u);
                put<uint32_t>(out, uint32_t(pay.size()));
                put<uint32_t>(out, fnv1a(pay.data(), pay.size()));
                put<uint32_t>(out, uint32_t(pieces));
            }
        }
        CHECK(k == f.results.size());

        // reassemble_heads on its own: slot r is the head of record r
        const ReassembledHeads h = reassemble_heads(c, slab, slab_len, segs, 64);
        CHECK(h.n() == f.heads.n() && h.heads.size() == h.n() * 64 && h.rec_len == f.heads.rec_len);
        for (size_t r = 0; r < h.n(); ++r) {
            const size_t p = std::min<size_t>(h.rec_len[r], 64);
            CHECK(std::memcmp(h.heads.data() + 64 * r, f.heads.heads.data() + size_t(f.heads.head_len) * r, p) == 0);
        }

        // no segments, a bad head_len, and a segment outside the slab
        CHECK(dec.try_from_fragmented_heads(c, slab, slab_len, {}).results.empty());
        CHECK(reassemble_heads(c, slab, slab_len, {}).n() == 0);
        int threw = 0;
        try {
            reassemble_heads(c, slab, slab_len, segs, 100);
        } catch (const CodecError&) {
            ++threw;
        }
        try {
            reassemble_heads(c, slab, slab_len, {Segment{slab_len - 4, 8}});
        } catch (const CodecError&) {
            ++threw;
        }
        CHECK(threw == 2);

        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
        CHECK(bool(o));
        std::printf("PASS test_heads: %zu segments, %zu records, %zu fragments, retried %d\n", size_t(nseg),
                    f.results.size(), f.heads.n_frags(), int(f.retried));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_heads: %s\n", e.what());
        return 1;
    }
}
