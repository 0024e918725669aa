// plan_probe.cpp — the arithmetic of onc_route_calls
// (onc-rpc_amd/csrc/route_plan.h) on the CPU: compiled with the host compiler
// (and -fsanitize=undefined where the toolchain has it) and run by
// tests/test_route_host.py, which writes the tables and keys, and compares
// what is printed here with tests/route_model.py. The kernels call the same
// functions. Commands on stdin, one a line, answers on stdout in their order:
//   T ntab nh, then ntab lines "program version proc_first proc_count handler_first flags"
//                         the table of the commands that follow
//   V                     -> "V <first bad entry + 1, or 0>"
//   K program version procedure
//                         -> "K <bin> <stat> <low> <high>" (a valid table)
//   B tile n, then n bins -> "B <order[0 .. n)> | <bin_first[0 .. nh + 4)>": the records grouped
//                         through per-tile bin counts laid out by bin_count_at
//                         and scanned in memory order, at `tile` records a tile
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "route_plan.h"

using namespace onc;

static std::vector<onc_route> g_tab;
static uint32_t g_nh = 0;

static void blocks(uint32_t tile, const std::vector<uint32_t>& bin) {
    const uint64_t n = bin.size();
    const uint32_t bins = route_bins(g_nh);
    const uint64_t tiles = tile_count(n, tile);
    std::vector<uint32_t> cnt(route_scratch_words(n, g_nh, tile), 0);
    for (uint64_t r = 0; r < n; ++r) ++cnt[bin_count_at(bin[r], r / tile, tiles)];
    // one exclusive scan in memory order; a bin's first record where its row starts
    std::vector<uint64_t> first(bins + 1, 0);
    uint64_t sum = 0;
    for (uint32_t b = 0; b < bins; ++b) {
        first[b] = sum;
        for (uint64_t t = 0; t < tiles; ++t) {
            const uint64_t at = bin_count_at(b, t, tiles);
            const uint32_t c = cnt[at];
            cnt[at] = uint32_t(sum);
            sum += c;
        }
    }
    first[bins] = sum;
    std::vector<uint32_t> order(n, 0xFFFFFFFFu);
    for (uint64_t r = 0; r < n; ++r) order[cnt[bin_count_at(bin[r], r / tile, tiles)]++] = uint32_t(r);
    std::printf("B");
    for (uint64_t k = 0; k < n; ++k) std::printf(" %u", order[k]);
    std::printf(" |");
    for (uint32_t b = 0; b <= bins; ++b) std::printf(" %" PRIu64, first[b]);
    std::printf("\n");
}

int main() {
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        if (cmd == 'T') {
            uint32_t ntab;
            if (std::scanf("%u %u", &ntab, &g_nh) != 2) return 2;
            g_tab.assign(ntab, onc_route{});
            for (auto& e : g_tab)
                if (std::scanf("%u %u %u %u %u %u", &e.program, &e.version, &e.proc_first, &e.proc_count,
                               &e.handler_first, &e.flags) != 6)
                    return 2;
        } else if (cmd == 'V') {
            std::printf("V %u\n", route_first_bad(g_tab.data(), uint32_t(g_tab.size()), g_nh));
        } else if (cmd == 'K') {
            uint32_t p, v, c;
            if (std::scanf("%u %u %u", &p, &v, &c) != 3) return 2;
            const RouteOutcome o = route_lookup(g_tab.data(), uint32_t(g_tab.size()), g_nh, p, v, c);
            std::printf("K %u %u %u %u\n", o.bin, o.stat, o.low, o.high);
        } else if (cmd == 'B') {
            uint32_t tile;
            uint64_t n;
            if (std::scanf("%u %" SCNu64, &tile, &n) != 2 || tile == 0) return 2;
            std::vector<uint32_t> bin(n);
            for (auto& b : bin)
                if (std::scanf("%u", &b) != 1 || b >= route_bins(g_nh)) return 2;
            blocks(tile, bin);
        } else {
            return 2;
        }
    }
    return 0;
}
