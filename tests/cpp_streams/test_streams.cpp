// test_streams.cpp — BatchDecoder::try_from_streams (include/onc_rpc.hpp) on a
// slab of connection buffers: every segment framed on its own and every whole
// record decoded, over a staged copy of the slab and over a HostRegistration
// of it. The slab and its segment list are a file written by the test that
// runs this (tests/test_gpu_extents.py, -m gpu); what was framed and decoded
// goes to a second file, which that test compares with the host model and the
// oracle.
// Usage: test_streams <in> <out>
//   in : u64 nseg, u64 slab_len, u64 seg_off[nseg], u64 seg_len[nseg], slab bytes
//   out: u64 n, u64 rows[6 * nseg], then per record i32 status, u32 xid, u64 payload offset, u32 payload length
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

static std::vector<uint8_t> digest(const std::vector<Decoded>& recs, const std::vector<SegmentResult>& segs,
                                   const uint8_t* wire) {
    std::vector<uint8_t> out;
    put<uint64_t>(out, recs.size());
    for (const SegmentResult& g : segs) {
        put<uint64_t>(out, g.first);
        put<uint64_t>(out, g.n);
        put<uint64_t>(out, g.consumed);
        put<uint64_t>(out, uint64_t(int64_t(g.status)));
        put<uint64_t>(out, g.aux0);
        put<uint64_t>(out, g.aux1);
    }
    for (const Decoded& d : recs) {
        put<int32_t>(out, d.status);
        put<uint32_t>(out, d.ok() ? d.message->xid() : 0u);
        // the payload view borrows the caller's slab
        uint64_t off = 0;
        uint32_t len = 0;
        if (d.ok()) {
            const CallBody* cb = d.message->call_body();
            if (cb) {
                off = uint64_t(cb->payload().ptr - wire);
                len = uint32_t(cb->payload().len);
            }
        }
        put<uint64_t>(out, off);
        put<uint32_t>(out, len);
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_streams <in> <out>\n");
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
        // the slab in page-aligned memory of its own, as a server's would be
        void* mem = nullptr;
        CHECK(posix_memalign(&mem, 4096, (slab_len + 4095) / 4096 * 4096 + 4096) == 0);
        uint8_t* slab = static_cast<uint8_t*>(mem);
        std::memcpy(slab, in.data() + 16 + 16 * nseg, slab_len);

        Codec c;
        BatchDecoder dec;
        std::vector<SegmentResult> rows;
        const std::vector<Decoded> staged = dec.try_from_streams(c, slab, slab_len, segs, &rows);
        CHECK(rows.size() == nseg);
        uint64_t k = 0;
        for (const SegmentResult& g : rows) {
            CHECK(g.first == k && g.consumed <= segs[&g - rows.data()].len);
            k += g.n;
        }
        CHECK(k == staged.size());
        const std::vector<uint8_t> a = digest(staged, rows, slab);

        std::vector<SegmentResult> rows2;
        std::vector<uint8_t> b;
        {
            HostRegistration reg(c, slab, slab_len);
            const std::vector<Decoded> mapped = dec.try_from_streams(c, reg, segs, &rows2);
            b = digest(mapped, rows2, slab);
        }
        CHECK(a == b);                                   // staged copy == decoded in place

        // no segments, and a segment outside the slab
        CHECK(dec.try_from_streams(c, slab, slab_len, {}, &rows2).empty() && rows2.empty());
        bool threw = false;
        try {
            dec.try_from_streams(c, slab, slab_len, {Segment{slab_len - 4, 8}});
        } catch (const CodecError&) {
            threw = true;
        }
        CHECK(threw);

        std::ofstream f(argv[2], std::ios::binary);
        f.write(reinterpret_cast<const char*>(a.data()), std::streamsize(a.size()));
        CHECK(bool(f));
        std::free(mem);
        std::printf("PASS test_streams: %zu segments, %zu records\n", size_t(nseg), staged.size());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL test_streams: %s\n", e.what());
        return 1;
    }
}
