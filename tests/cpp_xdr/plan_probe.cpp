// plan_probe.cpp — the arithmetic of onc_xdr_unpack
// (onc-rpc_amd/csrc/xdr_plan.h) on the CPU: compiled with the host compiler
// and -fsanitize=address,undefined and run by tests/test_xdr_host.py, which
// writes the schemas and payloads, and compares what is printed here with
// tests/xdr_model.py. The kernel calls the same functions. A payload's bytes
// live in a heap block of exactly their number, so a read past them is a
// sanitizer report. Commands on stdin, one a line, answers on stdout in order:
//   S nf, then nf lines "type_flags arg col_off cond_val reserved"
//                         the schema of the commands that follow
//   V n cols_cap          -> "V <first bad field + 1, or 0>"
//   F cap                 -> "F <how far the schema's word reads can reach, cap at most>"
//   X o L r heads head_len has_start start wire_len
//                         -> "X <bad> <base> <hi>"
//   P flags heads o hi base L nbytes <hex of nbytes bytes, or ->
//                         one record of payload_len L whose first nbytes bytes exist
//                         -> "P <code> <fail> <present> <p> <value per field>":
//                            a u32 or u64 in decimal, or pos:len
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "xdr_plan.h"

using namespace onc;

static std::vector<onc_xdr_field> g_fields;

struct HeapReader {
    const uint8_t* bytes;
    uint64_t size;
    uint32_t word(uint64_t p) {
        if (p > size || size - p < 4) {                  // the parse asked for bytes it had not checked
            std::printf("READ PAST THE PAYLOAD at %" PRIu64 "\n", p);
            std::exit(3);
        }
        return uint32_t(bytes[p]) << 24 | uint32_t(bytes[p + 1]) << 16 | uint32_t(bytes[p + 2]) << 8 | bytes[p + 3];
    }
};

struct PrintSink {
    std::string out;
    void put32(const onc_xdr_field&, uint32_t v) { out += " " + std::to_string(v); }
    void put64(const onc_xdr_field&, uint64_t v) { out += " " + std::to_string(v); }
    void put_pair(const onc_xdr_field&, uint32_t pos, uint32_t len) {
        out += " " + std::to_string(pos) + ":" + std::to_string(len);
    }
};

int main() {
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        if (cmd == 'S') {
            uint32_t nf;
            if (std::scanf("%u", &nf) != 1 || nf > 1000) return 2;
            g_fields.assign(nf, onc_xdr_field{});
            for (auto& f : g_fields)
                if (std::scanf("%u %u %" SCNu64 " %u %u", &f.type_flags, &f.arg, &f.col_off, &f.cond_val,
                               &f.reserved) != 5)
                    return 2;
        } else if (cmd == 'V') {
            uint64_t n, cap;
            if (std::scanf("%" SCNu64 " %" SCNu64, &n, &cap) != 2) return 2;
            std::printf("V %u\n", xdr_schema_first_bad(g_fields.data(), uint32_t(g_fields.size()), n, cap));
        } else if (cmd == 'F') {
            uint64_t cap;
            if (std::scanf("%" SCNu64, &cap) != 1) return 2;
            std::printf("F %" PRIu64 "\n", xdr_reach(g_fields.data(), uint32_t(g_fields.size()), cap));
        } else if (cmd == 'X') {
            uint64_t o, L, r, start, wire_len;
            uint32_t heads, head_len, has_start;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %u %u %u %" SCNu64 " %" SCNu64, &o, &L, &r, &heads,
                           &head_len, &has_start, &start, &wire_len) != 8)
                return 2;
            const XdrExtent e = xdr_extent(o, L, r, heads != 0, head_len, has_start != 0, start, wire_len);
            std::printf("X %d %" PRIu64 " %" PRIu64 "\n", int(e.bad), e.base, e.hi);
        } else if (cmd == 'P') {
            uint32_t flags, heads;
            uint64_t o, hi, base, L, nbytes;
            char hex[8192];
            if (std::scanf("%u %u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %8191s", &flags, &heads, &o,
                           &hi, &base, &L, &nbytes, hex) != 8)
                return 2;
            if (nbytes ? std::strlen(hex) != 2 * nbytes : std::strcmp(hex, "-") != 0) return 2;
            std::unique_ptr<uint8_t[]> bytes(new uint8_t[nbytes ? nbytes : 1]);
            for (uint64_t i = 0; i < nbytes; ++i) {
                unsigned b;
                if (std::sscanf(hex + 2 * i, "%2x", &b) != 1) return 2;
                bytes[i] = uint8_t(b);
            }
            HeapReader rd{bytes.get(), nbytes};
            PrintSink sink;
            const XdrExtent e{false, base, hi};
            const XdrParsed out = xdr_parse(g_fields.data(), uint32_t(g_fields.size()), flags, ONC_XDR_OK, o, L, e,
                                            heads != 0, rd, sink);
            std::printf("P %u %u %" PRIu64 " %" PRIu64 "%s\n", out.code, out.fail, out.present, out.p,
                        sink.out.c_str());
        } else {
            return 2;
        }
    }
    return 0;
}
