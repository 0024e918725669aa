// test_bounded.cpp — BatchDecoder::try_from (include/onc_rpc.hpp) with record
// lengths that run past the wire: the mirror decodes through
// onc_decode_lengths_bounded, so the overrunning records come back as
// Error(ONC_DEC_BAD_EXTENT) — where the caller's own &wire[off..off + len]
// would have panicked — and the records before them decode as before.
// Run by tests/test_gpu_bounded.py (-m gpu).
#include <cstdio>
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

static void run(Codec& c) {
    const int kN = 70;                       // two decode workgroups
    const int kBadAt = 50;
    std::vector<std::vector<uint8_t>> payloads;
    std::vector<RpcMessage> msgs;
    payloads.reserve(kN);
    for (int i = 0; i < kN; ++i) payloads.emplace_back(size_t(8 + 4 * (i % 5)), uint8_t(i));
    const std::vector<uint32_t> gids = {1, 2, 3};
    const std::vector<uint8_t> name = {'h', 'o', 's', 't'};
    BatchEncoder enc;
    for (int i = 0; i < kN; ++i) {
        const AuthFlavor cred = i % 3 == 0 ? AuthFlavor::unix(AuthUnixParams(uint32_t(i), Bytes(name), 501, 20, gids))
                                           : AuthFlavor::none();
        msgs.emplace_back(uint32_t(1000 + i), MessageType::call(CallBody(100003, 4, uint32_t(i), cred, AuthFlavor::none(),
                                                                         Bytes(payloads[size_t(i)]))));
    }
    for (const RpcMessage& m : msgs) enc.push(m);
    std::vector<uint8_t> wire;
    std::vector<uint64_t> off;
    const std::vector<int32_t> st = enc.serialise_into(c, wire, &off);
    std::vector<uint32_t> rec_len(kN);
    for (int i = 0; i < kN; ++i) {
        CHECK(st[size_t(i)] == ONC_OK);
        rec_len[size_t(i)] = uint32_t(off[size_t(i) + 1] - off[size_t(i)]);
    }
    BatchDecoder dec;
    for (DecodeMode mode : {DecodeMode::Slice, DecodeMode::Bytes}) {
        // good lengths: as before
        std::vector<Decoded> out = dec.try_from(c, wire.data(), wire.size(), rec_len, mode);
        for (int i = 0; i < kN; ++i) CHECK(out[size_t(i)].ok() && *out[size_t(i)].message == msgs[size_t(i)]);
        // the whole wire, then an empty record at its end: a legal empty slice
        std::vector<uint32_t> with_empty = rec_len;
        with_empty.push_back(0);
        out = dec.try_from(c, wire.data(), wire.size(), with_empty, mode);
        CHECK(out[kN].status == ONC_ERR_INCOMPLETE_HEADER);
        // one length inflated past the end of the wire: that record ends past
        // it, every later one starts past it
        std::vector<uint32_t> bad = rec_len;
        bad[kBadAt] += uint32_t(wire.size());
        out = dec.try_from(c, wire.data(), wire.size(), bad, mode);
        for (int i = 0; i < kN; ++i) {
            const Decoded& d = out[size_t(i)];
            if (i < kBadAt) {
                CHECK(d.ok() && *d.message == msgs[size_t(i)]);
                continue;
            }
            CHECK(d.status == ONC_DEC_BAD_EXTENT && !d.message.has_value());
            CHECK(d.aux0 == uint32_t(i == kBadAt ? ONC_EXTENT_END_PAST_WIRE : ONC_EXTENT_START_PAST_WIRE) && d.aux1 == 0);
            const Error e = d.error();
            CHECK(e.code() == ONC_DEC_BAD_EXTENT);
            CHECK(std::string(e.what()).find("slice index out of range") != std::string::npos);
        }
    }
}

int main() {
    try {
        Codec codec(0);
        run(codec);
    } catch (const std::exception& e) {
        std::printf("FAIL test_bounded: %s\n", e.what());
        return 1;
    }
    std::printf("PASS test_bounded\n");
    return 0;
}
