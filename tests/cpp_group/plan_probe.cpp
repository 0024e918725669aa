// plan_probe.cpp — the arithmetic of onc_group_by_conn
// (onc-rpc_amd/csrc/group_plan.h) on the CPU: compiled with the host compiler
// (and -fsanitize=undefined where the toolchain has it) and run by
// tests/test_group_host.py, which writes the lists, and compares what is
// printed here with tests/group_model.py. The kernels call the same functions.
// Commands on stdin, one a line, answers on stdout in their order:
//   P nconn               -> "P <bits> <passes>"
//   D nconn conn          -> "D <clamped key> <digit of pass 0> .. <digit of the last pass>"
//   Z n                   -> "Z <scratch bytes at ONC_GROUP_TILE items a tile>"
//   S tile nconn nsrc nvia, then nsrc connections, then nvia via entries (nvia == 0: no via)
//                         -> "S <order[0 .. n)> | <conn_first[0 .. nconn + 2)> | <result[0 .. 3)>": the
//                         items sorted pass by pass through per-tile digit counts
//                         laid out by bin_count_at and scanned in memory order,
//                         in the buffers group_layout places, at `tile` items a tile
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "group_plan.h"

using namespace onc;

static void sort(uint32_t tile, uint32_t nconn, const std::vector<uint32_t>& rec_conn, const std::vector<uint32_t>& via,
                 bool has_via) {
    const uint64_t nsrc = rec_conn.size(), n = has_via ? via.size() : nsrc;
    const GroupLayout l = group_layout(n, tile);
    const uint64_t tiles = tile_count(n, tile);
    std::vector<uint32_t> w(l.words, 0xA5A5A5A5u), order(n, 0xFFFFFFFFu);
    const uint32_t passes = group_passes(nconn);
    const uint32_t* sorted = nullptr;
    if (passes == 0)
        for (uint64_t k = 0; k < n; ++k) order[k] = uint32_t(k);
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t d = group_pass_dst(p);
        const uint32_t *src_key = &w[l.key[d ^ 1]], *src_idx = &w[l.idx[d ^ 1]];
        uint32_t* dst_key = &w[l.key[d]];
        uint32_t* dst_idx = p + 1 == passes ? order.data() : &w[l.idx[d]];
        auto item = [&](uint64_t k, uint32_t& key, uint32_t& idx) {
            if (p) {
                key = src_key[k];
                idx = src_idx[k];
                return;
            }
            const uint64_t s = has_via ? via[k] : k;
            key = group_clamp(s < nsrc ? rec_conn[s] : nconn, nconn);
            idx = uint32_t(k);
        };
        uint32_t* cnt = &w[l.counts];
        for (uint64_t i = 0; i < uint64_t(kGroupDigits) * tiles; ++i) cnt[i] = 0;
        uint32_t key, idx;
        for (uint64_t k = 0; k < n; ++k) {
            item(k, key, idx);
            ++cnt[bin_count_at(group_digit(key, p), k / tile, tiles)];
        }
        // the scan per digit, then the scan of the totals
        for (uint32_t g = 0; g < kGroupDigits; ++g) {
            uint32_t sum = 0;
            for (uint64_t t = 0; t < tiles; ++t) {
                const uint64_t at = bin_count_at(g, t, tiles);
                const uint32_t c = cnt[at];
                cnt[at] = sum;
                sum += c;
            }
            w[l.totals + g] = sum;
        }
        uint32_t sum = 0;
        for (uint32_t g = 0; g < kGroupDigits; ++g) {
            w[l.first + g] = sum;
            sum += w[l.totals + g];
        }
        for (uint64_t k = 0; k < n; ++k) {
            item(k, key, idx);
            const uint32_t g = group_digit(key, p);
            const uint64_t j = uint64_t(w[l.first + g]) + cnt[bin_count_at(g, k / tile, tiles)]++;
            if (j >= n) {
                std::printf("S out of range\n");
                return;
            }
            dst_key[j] = key;
            dst_idx[j] = idx;
        }
        sorted = dst_key;
    }
    std::printf("S");
    for (uint64_t k = 0; k < n; ++k) std::printf(" %u", order[k]);
    std::printf(" |");
    uint64_t sent = 0, active = 0, before = 0;
    for (uint64_t c = 0; c <= uint64_t(nconn) + 1; ++c) {
        const uint64_t lb = passes ? group_lower_bound(sorted, n, uint32_t(c)) : (c == 0 ? 0 : n);
        std::printf(" %" PRIu64, lb);
        if (c == nconn) sent = lb;
        if (c >= 1 && c <= nconn && lb > before) ++active;
        before = lb;
    }
    std::printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", sent, n - sent, active);
}

int main() {
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        if (cmd == 'P') {
            uint32_t nconn;
            if (std::scanf("%u", &nconn) != 1) return 2;
            std::printf("P %u %u\n", group_bits(nconn), group_passes(nconn));
        } else if (cmd == 'D') {
            uint32_t nconn, conn;
            if (std::scanf("%u %u", &nconn, &conn) != 2) return 2;
            const uint32_t key = group_clamp(conn, nconn);
            std::printf("D %u", key);
            for (uint32_t p = 0; p < group_passes(nconn); ++p) std::printf(" %u", group_digit(key, p));
            std::printf("\n");
        } else if (cmd == 'Z') {
            uint64_t n;
            if (std::scanf("%" SCNu64, &n) != 1) return 2;
            std::printf("Z %" PRIu64 "\n", group_scratch_bytes(n, kGroupTile));
        } else if (cmd == 'S') {
            uint32_t tile, nconn;
            uint64_t nsrc, nvia;
            if (std::scanf("%u %u %" SCNu64 " %" SCNu64, &tile, &nconn, &nsrc, &nvia) != 4 || tile == 0) return 2;
            std::vector<uint32_t> rc(nsrc), via(nvia);
            for (auto& v : rc)
                if (std::scanf("%u", &v) != 1) return 2;
            for (auto& v : via)
                if (std::scanf("%u", &v) != 1) return 2;
            sort(tile, nconn, rc, via, nvia != 0);
        } else {
            return 2;
        }
    }
    return 0;
}
