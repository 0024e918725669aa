// test_fragment_iov.cpp — BatchEncoder::serialise_vectored (include/onc_rpc.hpp:
// onc_encode_iov + onc_compact_iov + onc_fragment_iov) against the packed path
// (serialise_into + fragment_stream): a handful of messages with AUTH_NONE and
// AUTH_UNIX credentials, an empty and a 1000-byte payload, and one that fails.
// Gathering the pieces must give the packed path's bytes at every max_frag,
// and serialise_into's own at 0x7FFFFFFF. Run by
// tests/test_gpu_fragment_iov.py (-m gpu).
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

static std::vector<uint8_t> ramp(size_t n, uint8_t seed) {
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = uint8_t(seed + 7 * i);
    return v;
}

static void run(Codec& c) {
    const std::vector<uint8_t> none, small = ramp(5, 3), big = ramp(1000, 11), name = ramp(9, 40), over(201, 1);
    const std::vector<uint32_t> gids = {1, 2, 3};
    const AuthFlavor unix_cred = AuthFlavor::unix(AuthUnixParams(77, Bytes(name), 501, 20, gids));
    std::vector<RpcMessage> msgs;
    msgs.emplace_back(1, MessageType::call(CallBody(100000, 2, 1, AuthFlavor::none(), AuthFlavor::none(), Bytes(none))));
    msgs.emplace_back(2, MessageType::call(CallBody(100003, 3, 7, unix_cred, AuthFlavor::none(), Bytes(big))));
    // 201 bytes of AuthNone data: the reference panics, the message writes nothing
    msgs.emplace_back(3, MessageType::call(CallBody(1, 1, 1, AuthFlavor::none(Bytes(over)), AuthFlavor::none(),
                                                    Bytes(small))));
    msgs.emplace_back(4, MessageType::call(CallBody(100003, 3, 1, unix_cred, unix_cred, Bytes(none))));
    msgs.emplace_back(5, MessageType::call(CallBody(100005, 1, 4, AuthFlavor::none(), AuthFlavor::none(), Bytes(small))));
    BatchEncoder enc;
    for (const RpcMessage& m : msgs) enc.push(m);
    const size_t n = msgs.size();

    std::vector<uint8_t> packed;
    std::vector<uint64_t> rec_off;
    const std::vector<int32_t> st = enc.serialise_into(c, packed, &rec_off);
    CHECK(st[2] == ONC_ENC_AUTH_GT_200 && rec_off[2] == rec_off[3]);
    for (size_t i = 0; i < n; ++i) CHECK(i == 2 || st[i] == ONC_OK);

    for (uint32_t max_frag : {1u, 7u, 28u, 0x7FFFFFFFu}) {
        const Fragmented f = fragment_stream(c, packed.data(), packed.size(), max_frag);
        CHECK(!f.stop.has_value());
        const VectoredStream v = enc.serialise_vectored(c, max_frag);
        const uint8_t* arena = enc.payload_arena().data();
        const std::vector<uint8_t> got = v.gather(arena);
        CHECK(got == f.bytes);
        if (max_frag == 0x7FFFFFFFu) CHECK(got == packed);
        CHECK(v.status == st);
        CHECK(v.bytes == f.bytes.size() && v.n_frags == f.n_frags && v.n_multi == f.n_multi);
        CHECK(v.marks.size() == 4 * v.n_frags);
        CHECK(v.out_off.size() == n + 1 && v.piece_off.size() == n + 1);
        CHECK(v.out_off.back() == v.bytes && v.piece_off.back() == v.pieces.size() && v.piece_off[0] == 0);
        // the failing message contributes nothing; every other one its own fragments
        CHECK(v.piece_off[2] == v.piece_off[3] && v.out_off[2] == v.out_off[3]);
        size_t at = 0;   // fragment_stream numbers the four framed records
        for (size_t i = 0; i < n; ++i) {
            if (i == 2) continue;
            CHECK(v.out_off[i] == f.out_off[at] && v.out_off[i + 1] - v.out_off[i] == f.out_off[at + 1] - f.out_off[at]);
            CHECK(v.piece_off[i + 1] > v.piece_off[i]);
            CHECK(v.pieces[size_t(v.piece_off[i])].src == ONC_PIECE_MARK);
            ++at;
        }
        // the writev() view: the same bytes piece by piece, none empty
        size_t pos = 0;
        for (size_t i = 0; i < v.pieces.size(); ++i) {
            const auto p = v.piece_ptr(i, arena);
            CHECK(p.second > 0 && pos + p.second <= got.size());
            CHECK(std::memcmp(p.first, got.data() + pos, p.second) == 0);
            pos += p.second;
        }
        CHECK(pos == got.size());
        // and back through the receive side
        const Reassembled r = reassemble_stream(c, got.data(), got.size());
        CHECK(!r.stop.has_value() && r.bytes == packed);
    }

    // an invalid max_frag, a body-level batch, an empty batch
    for (uint32_t bad : {0u, 0x80000000u}) {
        bool threw = false;
        try {
            (void)enc.serialise_vectored(c, bad);
        } catch (const CodecError&) {
            threw = true;
        }
        CHECK(threw);
    }
    BatchEncoder body;
    body.push(*msgs[0].call_body());
    bool threw = false;
    try {
        (void)body.serialise_vectored(c);
    } catch (const CodecError&) {
        threw = true;
    }
    CHECK(threw);
    BatchEncoder empty;
    const VectoredStream e = empty.serialise_vectored(c);
    CHECK(e.pieces.empty() && e.marks.empty() && e.bytes == 0 && e.out_off.size() == 1 && e.gather(nullptr).empty());
}

int main() {
    try {
        Codec codec(0);
        run(codec);
    } catch (const std::exception& e) {
        std::printf("FAIL test_fragment_iov: %s\n", e.what());
        return 1;
    }
    std::printf("PASS test_fragment_iov\n");
    return 0;
}
