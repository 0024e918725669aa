// test_fragment.cpp — fragment_stream (include/onc_rpc.hpp) on a packed
// stream of single-fragment records: the reference's framer stops at its
// output with Fragmented once a record is cut, and reassemble_stream of it
// gives the input back byte for byte. The stream is a file written by the
// test that runs this (tests/test_gpu_fragment_encode.py, -m gpu): the golden
// vectors back to back.
// Usage: test_fragment <stream> <max_frag>
#include <cstdio>
#include <cstdlib>
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

static void run(Codec& c, const std::vector<uint8_t>& orig, uint32_t max_frag) {
    const Fragmented f = fragment_stream(c, orig.data(), orig.size(), max_frag);
    CHECK(!f.stop.has_value());
    const size_t n = f.status.size();
    CHECK(n > 0 && f.out_off.size() == n + 1 && f.out_off[0] == 0 && f.out_off.back() == f.bytes.size());
    for (int32_t st : f.status) CHECK(st == ONC_OK);
    CHECK(f.n_frags >= n && f.bytes.size() == orig.size() + 4 * (f.n_frags - n));
    CHECK((f.n_multi > 0) == (f.n_frags > n));
    // every fragment body is at most max_frag long, and the marks chain to the end
    size_t p = 0, frags = 0;
    while (p < f.bytes.size()) {
        CHECK(p + 4 <= f.bytes.size());
        const uint32_t m = uint32_t(f.bytes[p]) << 24 | uint32_t(f.bytes[p + 1]) << 16 | uint32_t(f.bytes[p + 2]) << 8 |
                           uint32_t(f.bytes[p + 3]);
        CHECK((m & 0x7FFFFFFFu) <= max_frag);
        p += 4 + (m & 0x7FFFFFFFu);
        ++frags;
    }
    CHECK(p == f.bytes.size() && frags == f.n_frags);

    if (f.n_multi) {
        // the reference's view of it: Fragmented at the first cut record
        BatchDecoder dec;
        std::optional<Error> stop;
        size_t consumed = 0;
        dec.try_from_stream(c, f.bytes.data(), f.bytes.size(), DecodeMode::Slice, &consumed, &stop);
        CHECK(stop.has_value() && stop->code() == ONC_ERR_FRAGMENTED && consumed < f.bytes.size());
    } else {
        CHECK(f.bytes == orig);
    }

    const Reassembled r = reassemble_stream(c, f.bytes.data(), f.bytes.size());
    CHECK(!r.stop.has_value());
    CHECK(r.bytes == orig);
    CHECK(r.consumed == f.bytes.size() && r.pending_frags == 0);
    CHECK(r.n_multi == f.n_multi && r.status.size() == n);
    for (int32_t st : r.status) CHECK(st == ONC_OK);

    // a cut stream: the framer's stop is carried, the whole records are fragmented
    const Fragmented t = fragment_stream(c, orig.data(), orig.size() - 1, max_frag);
    CHECK(t.stop.has_value() && t.status.size() == n - 1 && t.out_off.back() == f.out_off[n - 1]);
    // an empty buffer
    const Fragmented e = fragment_stream(c, nullptr, 0, max_frag);
    CHECK(e.bytes.empty() && e.out_off.size() == 1 && e.out_off[0] == 0 && e.status.empty() && !e.stop);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s stream max_frag\n", argv[0]);
        return 2;
    }
    try {
        Codec codec(0);
        run(codec, read_file(argv[1]), uint32_t(std::strtoul(argv[2], nullptr, 10)));
    } catch (const std::exception& e) {
        std::printf("FAIL test_fragment: %s\n", e.what());
        return 1;
    }
    std::printf("PASS test_fragment\n");
    return 0;
}
