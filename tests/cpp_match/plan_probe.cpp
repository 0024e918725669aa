// plan_probe.cpp — onc-rpc_amd/csrc/match_plan.h driven on the host: the
// arithmetic match.hip's kernels call, stand-alone (no HIP, no library), so
// that tests/test_match_host.py checks it against tests/match_model.py and a
// sanitizer build runs it. Commands on stdin, an answer line each:
//   S np                  -> "S slots"
//   N slot slots          -> "N next"
//   W n np                -> "W slots first_rec clear_words rec_counts pend_counts words rtiles ptiles"
//   C cls tile rtiles     -> "C at"
//   H conn xid slots var  -> "H slot"
//   R m                   -> "R result class of a final match[] value"
//   E var order np n, then np lines "conn xid", then n lines "conn xid"
//                         -> "E lead ..." (-1: none): match_insert and
//                            match_probe emulated one lane after the other on
//                            a table of match_slots(np) slots; the entries are
//                            inserted in ascending (order 0), descending (1)
//                            or interleaved (2: odd indices first) order, the
//                            orders a race can produce. Every probe loop is
//                            bounded by the slot count, and every key is found
//                            in exactly one slot afterwards.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "match_plan.h"

using namespace onc;

static void die(const char* what) {
    std::fprintf(stderr, "plan_probe: %s\n", what);
    std::exit(1);
}

struct Key {
    uint32_t conn, xid;
};

static void emulate(uint32_t variant, int order, const std::vector<Key>& pend, const std::vector<Key>& recs) {
    const uint64_t np = pend.size(), S = match_slots(np);
    if (S < 2 * np || S < kMatchSlotsMin || (S & (S - 1))) die("slot count");
    std::vector<uint32_t> table(S, kMatchEmpty);
    std::vector<uint64_t> seq;
    if (order == 0)
        for (uint64_t p = 0; p < np; ++p) seq.push_back(p);
    else if (order == 1)
        for (uint64_t p = np; p-- > 0;) seq.push_back(p);
    else {
        for (uint64_t p = 1; p < np; p += 2) seq.push_back(p);
        for (uint64_t p = 0; p < np; p += 2) seq.push_back(p);
    }
    for (uint64_t p : seq) {                                       // match_insert, a lane
        const Key k = pend[p];
        uint64_t s = match_hash(k.conn, k.xid, S, variant);
        if (s >= S) die("hash out of range");
        bool placed = false;
        for (uint64_t i = 0; i < S && !placed; ++i) {
            const uint32_t q = table[s];                           // what atomicCAS(slot, EMPTY, p) returns
            if (q == kMatchEmpty) {
                table[s] = uint32_t(p);
                placed = true;
            } else if (pend[q].conn == k.conn && pend[q].xid == k.xid) {
                if (q > p) table[s] = uint32_t(p);                 // atomicMin
                placed = true;
            } else {
                s = match_next(s, S);
                if (s >= S) die("next out of range");
            }
        }
        if (!placed) die("an entry found no slot");
    }
    // each key in exactly one slot
    uint64_t taken = 0;
    for (uint64_t s = 0; s < S; ++s) {
        if (table[s] == kMatchEmpty) continue;
        ++taken;
        if (table[s] >= np) die("a slot holds no index");
        for (uint64_t t = s + 1; t < S; ++t)
            if (table[t] != kMatchEmpty && pend[table[t]].conn == pend[table[s]].conn &&
                pend[table[t]].xid == pend[table[s]].xid)
                die("a key in two slots");
    }
    if (taken > np) die("more slots than entries");
    std::printf("E");
    for (const Key& k : recs) {                                    // match_probe, a lane
        uint64_t s = match_hash(k.conn, k.xid, S, variant);
        long long lead = -1;
        for (uint64_t i = 0; i < S; ++i) {
            const uint32_t q = table[s];
            if (q == kMatchEmpty) break;
            if (pend[q].conn == k.conn && pend[q].xid == k.xid) {
                lead = q;
                break;
            }
            s = match_next(s, S);
        }
        std::printf(" %lld", lead);
    }
    std::printf("\n");
}

int main() {
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        if (cmd == 'S') {
            unsigned long long np;
            if (std::scanf("%llu", &np) != 1) die("S");
            std::printf("S %llu\n", (unsigned long long)match_slots(np));
        } else if (cmd == 'N') {
            unsigned long long s, S;
            if (std::scanf("%llu %llu", &s, &S) != 2) die("N");
            std::printf("N %llu\n", (unsigned long long)match_next(s, S));
        } else if (cmd == 'W') {
            unsigned long long n, np;
            if (std::scanf("%llu %llu", &n, &np) != 2) die("W");
            const MatchLayout l = match_layout(n, np);
            if (l.words != match_scratch_words(n, np)) die("W words");
            std::printf("W %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)l.slots,
                        (unsigned long long)l.first_rec, (unsigned long long)l.clear_words,
                        (unsigned long long)l.rec_counts, (unsigned long long)l.pend_counts,
                        (unsigned long long)l.words, (unsigned long long)l.rtiles, (unsigned long long)l.ptiles);
        } else if (cmd == 'C') {
            unsigned cls;
            unsigned long long tile, rtiles;
            if (std::scanf("%u %llu %llu", &cls, &tile, &rtiles) != 3) die("C");
            std::printf("C %llu\n", (unsigned long long)bin_count_at(cls, tile, rtiles));
        } else if (cmd == 'H') {
            unsigned conn, xid, var;
            unsigned long long S;
            if (std::scanf("%u %u %llu %u", &conn, &xid, &S, &var) != 4) die("H");
            std::printf("H %llu\n", (unsigned long long)match_hash(conn, xid, S, var));
        } else if (cmd == 'R') {
            unsigned m;
            if (std::scanf("%u", &m) != 1) die("R");
            std::printf("R %u\n", match_result_class(m));
        } else if (cmd == 'E') {
            unsigned var;
            int order;
            unsigned long long np, n;
            if (std::scanf("%u %d %llu %llu", &var, &order, &np, &n) != 4) die("E");
            std::vector<Key> pend(np), recs(n);
            for (Key& k : pend)
                if (std::scanf("%u %u", &k.conn, &k.xid) != 2) die("E list");
            for (Key& k : recs)
                if (std::scanf("%u %u", &k.conn, &k.xid) != 2) die("E records");
            emulate(var, order, pend, recs);
        } else {
            die("unknown command");
        }
    }
    return 0;
}
