// test_gather.cpp — BatchEncoder::serialise_fragmented (include/onc_rpc.hpp:
// onc_encode_iov + onc_fragment_iov + onc_piece_offsets + onc_gather_pieces)
// against the host gather of serialise_vectored's pieces and against the
// packed path (serialise_into + fragment_stream), with one limit for the batch
// and with a limit per message; VectoredStream::gather_window against slices
// of gather. Run by tests/test_gpu_gather.py (-m gpu).
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
    const std::vector<uint8_t> none, small = ramp(5, 3), big = ramp(1000, 11), huge = ramp(20000, 5), name = ramp(9, 40),
                               over(201, 1);
    const std::vector<uint32_t> gids = {1, 2, 3};
    const AuthFlavor unix_cred = AuthFlavor::unix(AuthUnixParams(77, Bytes(name), 501, 20, gids));
    std::vector<RpcMessage> msgs;
    msgs.emplace_back(1, MessageType::call(CallBody(100000, 2, 1, AuthFlavor::none(), AuthFlavor::none(), Bytes(none))));
    msgs.emplace_back(2, MessageType::call(CallBody(100003, 3, 7, unix_cred, AuthFlavor::none(), Bytes(big))));
    // 201 bytes of AuthNone data: the reference panics, the message writes nothing
    msgs.emplace_back(3, MessageType::call(CallBody(1, 1, 1, AuthFlavor::none(Bytes(over)), AuthFlavor::none(),
                                                    Bytes(small))));
    msgs.emplace_back(4, MessageType::call(CallBody(100003, 3, 1, unix_cred, unix_cred, Bytes(none))));
    msgs.emplace_back(5, MessageType::call(CallBody(100005, 1, 4, AuthFlavor::none(), AuthFlavor::none(), Bytes(huge))));
    msgs.emplace_back(6, MessageType::call(CallBody(100005, 1, 4, AuthFlavor::none(), AuthFlavor::none(), Bytes(small))));
    BatchEncoder enc;
    for (const RpcMessage& m : msgs) enc.push(m);
    const size_t n = msgs.size();

    std::vector<uint8_t> packed;
    std::vector<uint64_t> rec_off;
    const std::vector<int32_t> st = enc.serialise_into(c, packed, &rec_off);
    CHECK(st[2] == ONC_ENC_AUTH_GT_200 && rec_off[2] == rec_off[3]);

    // one limit for the batch
    for (uint32_t max_frag : {1u, 7u, 28u, 1024u, 0x7FFFFFFFu}) {
        const Fragmented f = fragment_stream(c, packed.data(), packed.size(), max_frag);
        CHECK(!f.stop.has_value());
        const VectoredStream v = enc.serialise_vectored(c, max_frag);
        const uint8_t* arena = enc.payload_arena().data();
        const std::vector<uint8_t> host = v.gather(arena);
        const FragmentedStream g = enc.serialise_fragmented(c, max_frag);
        CHECK(g.bytes == host);
        CHECK(g.bytes == f.bytes);
        if (max_frag == 0x7FFFFFFFu) CHECK(g.bytes == packed);
        CHECK(g.status == st && g.out_off == v.out_off);
        CHECK(g.n_frags == f.n_frags && g.n_multi == f.n_multi && g.out_off.back() == g.bytes.size());
        // the host's windows are slices of the whole
        const uint64_t total = host.size();
        const uint64_t wins[][2] = {{0, total}, {0, 0}, {1, 1}, {total, 16}, {8191, 2}, {total - 3, 100},
                                    {5, ~uint64_t(0)}, {total + 1, 5}};
        for (const auto& w : wins) {
            const std::vector<uint8_t> got = v.gather_window(w[0], w[1], arena);
            const uint64_t a = std::min(w[0], total), b = w[1] > total - a ? total : a + w[1];
            CHECK(got == std::vector<uint8_t>(host.begin() + a, host.begin() + b));
        }
        // and back through the receive side
        const Reassembled r = reassemble_stream(c, g.bytes.data(), g.bytes.size());
        CHECK(!r.stop.has_value() && r.bytes == packed);
    }

    // a limit per message, one of them no fragment size: that message
    // contributes nothing, every other one is cut at its own limit
    const std::vector<uint32_t> limits = {16, 100, 3, 0, 4096, 1};
    const FragmentedStream g = enc.serialise_fragmented(c, 28, &limits);
    std::vector<uint8_t> want;
    for (size_t i = 0; i < n; ++i) {
        CHECK(g.out_off[i] == want.size());
        if (i == 2) {
            CHECK(g.status[i] == ONC_ENC_AUTH_GT_200);
            continue;
        }
        if (limits[i] == 0) {
            CHECK(g.status[i] == ONC_ENC_BAD_DESCRIPTOR);
            continue;
        }
        CHECK(g.status[i] == ONC_OK);
        const Fragmented f = fragment_stream(c, packed.data() + rec_off[i], size_t(rec_off[i + 1] - rec_off[i]), limits[i]);
        CHECK(!f.stop.has_value());
        want.insert(want.end(), f.bytes.begin(), f.bytes.end());
    }
    CHECK(g.bytes == want && g.out_off[n] == want.size());

    // an invalid max_frag, limits of another size, a body-level batch, an empty batch
    auto throws = [&](auto&& call) {
        try {
            call();
        } catch (const CodecError&) {
            return true;
        }
        return false;
    };
    for (uint32_t bad : {0u, 0x80000000u}) CHECK(throws([&] { (void)enc.serialise_fragmented(c, bad); }));
    const std::vector<uint32_t> three = {1, 2, 3};
    CHECK(throws([&] { (void)enc.serialise_fragmented(c, 16, &three); }));
    BatchEncoder body;
    body.push(*msgs[0].call_body());
    CHECK(throws([&] { (void)body.serialise_fragmented(c); }));
    BatchEncoder empty;
    const FragmentedStream e = empty.serialise_fragmented(c);
    CHECK(e.bytes.empty() && e.out_off.size() == 1 && e.status.empty() && e.n_frags == 0);
}

int main() {
    try {
        Codec codec(0);
        run(codec);
    } catch (const std::exception& e) {
        std::printf("FAIL test_gather: %s\n", e.what());
        return 1;
    }
    std::printf("PASS test_gather\n");
    return 0;
}
