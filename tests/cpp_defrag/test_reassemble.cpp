// test_reassemble.cpp — reassemble_stream (include/onc_rpc.hpp) on a stream
// whose records come in several fragments: its bytes are the unfragmented
// stream, and BatchDecoder::try_from_stream on them gives what it gives on
// the original. Both streams are files written by the test that runs this
// (tests/test_gpu_fragments.py, -m gpu): the golden vectors back to back, and
// the same cut into fragments, with `tail` bytes of an unfinished record behind.
// Usage: test_reassemble <original> <fragmented> <tail>
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

static void run(Codec& c, const std::vector<uint8_t>& orig, const std::vector<uint8_t>& frag, size_t tail) {
    BatchDecoder dec;
    // the reference's view of the fragmented stream: Fragmented at the first cut record
    std::optional<Error> stop;
    size_t consumed = 0;
    dec.try_from_stream(c, frag.data(), frag.size(), DecodeMode::Slice, &consumed, &stop);
    CHECK(stop.has_value() && stop->code() == ONC_ERR_FRAGMENTED && consumed < frag.size());

    const Reassembled r = reassemble_stream(c, frag.data(), frag.size());
    CHECK(!r.stop.has_value());
    CHECK(r.bytes == orig);
    CHECK(r.consumed == frag.size() - tail);
    CHECK((r.pending_frags == 0) == (tail == 0));
    CHECK(r.n_multi > 0);
    CHECK(r.rec_off.size() == r.status.size() + 1 && r.rec_off.back() == orig.size());
    for (int32_t st : r.status) CHECK(st == ONC_OK);

    for (DecodeMode mode : {DecodeMode::Slice, DecodeMode::Bytes}) {
        size_t c0 = 0, c1 = 0;
        std::optional<Error> s0, s1;
        const std::vector<Decoded> want = dec.try_from_stream(c, orig.data(), orig.size(), mode, &c0, &s0);
        const std::vector<Decoded> got = dec.try_from_stream(c, r.bytes.data(), r.bytes.size(), mode, &c1, &s1);
        CHECK(c0 == orig.size() && c1 == c0 && !s0.has_value() && !s1.has_value());
        CHECK(got.size() == want.size() && got.size() == r.status.size());
        size_t ok = 0;
        for (size_t i = 0; i < got.size(); ++i) {
            CHECK(got[i].status == want[i].status && got[i].aux0 == want[i].aux0 && got[i].aux1 == want[i].aux1);
            CHECK(got[i].message.has_value() == want[i].message.has_value());
            if (got[i].message) {
                CHECK(*got[i].message == *want[i].message);
                ++ok;
            }
        }
        CHECK(ok > 0 && ok < got.size());     // the vectors hold good messages and bad ones
    }
    // an empty buffer
    const Reassembled e = reassemble_stream(c, nullptr, 0);
    CHECK(e.bytes.empty() && e.rec_off.size() == 1 && e.rec_off[0] == 0 && e.status.empty() && !e.stop);
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s original fragmented tail\n", argv[0]);
        return 2;
    }
    try {
        Codec codec(0);
        run(codec, read_file(argv[1]), read_file(argv[2]), size_t(std::atol(argv[3])));
    } catch (const std::exception& e) {
        std::printf("FAIL test_reassemble: %s\n", e.what());
        return 1;
    }
    std::printf("PASS test_reassemble\n");
    return 0;
}
