// match.hip — decoded Replies paired with the pending Calls they answer on
// gfx950 (onc_match_replies, include/onc_rpc.h): a hash join of the records'
// (connection, xid) against the caller's pending list, the first Reply of a
// Call told from its duplicates, and a stable compaction of the entries
// nobody answered. The table lives in the scratch and is built anew by every
// call; a slot holds a pending *index*, the keys stay in the caller's list.
//
//   match_clear    the slots and first_rec[np] filled with 0xFFFFFFFF, a
//                  16-byte store per lane.
//   match_insert   a lane per pending entry: linear probing from the key's
//                  hash; atomicCAS(slot, EMPTY, p) claims an empty slot; the
//                  index q it returns otherwise names the slot's key
//                  (pending[q], a plain load: the list is an input). The same
//                  key: atomicMin(slot, p), done; another: the next slot. The
//                  kernel decides only from what the atomics return and never
//                  reads the table plainly. A claimed slot's key never
//                  changes and all entries of a key walk the same chain, so
//                  every key ends in exactly one slot that holds its lowest
//                  index: which slot depends on the race, no output does.
//   match_probe    a lane per record: its status and, for an OK record only,
//                  the descriptor's first 16-byte granule (xid, msg_type) and
//                  rec_conn[r]; the chain walked with plain loads up to an
//                  equal key or an empty slot; match[r] = the lead p or a
//                  sentinel (provisional); atomicMin(&first_rec[p], r).
//   match_resolve  the record tiles: a provisional p whose first_rec[p] != r
//                  becomes DUPLICATE; tag_out; the tile's five classes counted
//                  (ballots, LDS) into the scratch. The pending tiles behind
//                  them in the same grid: hit[p] = first_rec[p]; the tile's
//                  unanswered entries counted.
//   match_scan     one workgroup: the pending tiles' counts scanned in place
//                  (partition.h scan_bin_row), the class counts summed, result.
//   match_compact  only with `still`. A lane per pending entry: its rank among
//                  its wave's unanswered entries by a ballot, the waves' counts
//                  added in wave order on top of the tile's scanned count; the
//                  entry moved as one 16-byte load and store.
//
// No workgroup waits for another and nothing spins on memory: the launch
// boundary is the only barrier between workgroups, and both probe loops end
// after S slots whatever the table holds. Atomics go to the scratch alone;
// the caller's arrays see plain loads and stores. Every index that addresses
// memory is 64-bit.
#include "kernels.h"
#include "match_plan.h"
#include "partition.h"

namespace onc {

constexpr int kMtThreads = int(kMatchTile);
constexpr int kMtWaves = kMtThreads / 64;
constexpr int kMtClearThreads = 256;
static_assert(kMatchTile == ONC_MATCH_TILE, "the tile the header names");
static_assert(kMtThreads * kMatchTile == 1048576,
              "a round of match_scan: tests/test_gpu_scan_rounds.py reaches rounds two and three by this number");
static_assert(kMatchEmpty == ONC_MATCH_NONE, "an untouched first_rec is hit[]'s NONE");
static_assert(sizeof(onc_pending) == 16, "moved as one 16-byte granule");
static_assert(ONC_MATCH_MAX <= ONC_MATCH_FAILED, "an index is never a sentinel");

struct MtKey {
    uint32_t conn, xid;
};
__device__ __forceinline__ MtKey mt_key(const onc_pending* pending, uint64_t p) {
    const uint64_t w = gload<uint64_t>(reinterpret_cast<uintptr_t>(pending + p));
    return MtKey{uint32_t(w), uint32_t(w >> 32)};
}

__global__ __launch_bounds__(kMtClearThreads) void match_clear_kernel(MatchArgs a) {
    const uint64_t g = uint64_t(blockIdx.x) * kMtClearThreads + threadIdx.x;   // a 16-byte granule
    if (4 * g >= a.clear_words) return;
    const u32x4 fill = {kMatchEmpty, kMatchEmpty, kMatchEmpty, kMatchEmpty};
    reinterpret_cast<u32x4*>(a.table)[g] = fill;
}

__global__ __launch_bounds__(kMtThreads) void match_insert_kernel(MatchArgs a) {
    const uint64_t p = uint64_t(blockIdx.x) * kMatchTile + threadIdx.x;
    if (p >= a.np) return;
    const MtKey k = mt_key(a.pending, p);
    uint64_t s = match_hash(k.conn, k.xid, a.slots, a.variant);
    for (uint64_t i = 0; i < a.slots; ++i) {                       // (bounded: at most np < S / 2 slots are ever taken)
        const uint32_t q = atomicCAS(&a.table[s], kMatchEmpty, uint32_t(p));
        if (q == kMatchEmpty) return;                              // claimed
        const MtKey o = mt_key(a.pending, q);
        if (o.conn == k.conn && o.xid == k.xid) {
            if (q > p) atomicMin(&a.table[s], uint32_t(p));
            return;
        }
        s = match_next(s, a.slots);
    }
}

__global__ __launch_bounds__(kMtThreads) void match_probe_kernel(MatchArgs a) {
    const uint64_t r = uint64_t(blockIdx.x) * kMatchTile + threadIdx.x;
    if (r >= a.n) return;
    const int32_t st = a.status[r];
    uint32_t xid = 0, msg_type = 0, conn = 0;
    if (st == ONC_OK) {
        const u32x4 q0 = gload<u32x4>(reinterpret_cast<uintptr_t>(a.msgs + r));
        xid = q0.x;
        msg_type = q0.y & 0xFFu;
        if (a.rec_conn) conn = a.rec_conn[r];
    }
    uint32_t m = match_class(st, msg_type);
    if (m == 0) {
        m = ONC_MATCH_UNKNOWN;
        uint64_t s = match_hash(conn, xid, a.slots, a.variant);
        for (uint64_t i = 0; i < a.slots; ++i) {
            const uint32_t q = a.table[s];
            if (q == kMatchEmpty) break;
            const MtKey o = mt_key(a.pending, q);
            if (o.conn == conn && o.xid == xid) {
                m = q;
                atomicMin(&a.first_rec[q], uint32_t(r));
                break;
            }
            s = match_next(s, a.slots);
        }
    }
    a.match[r] = m;
}

__global__ __launch_bounds__(kMtThreads) void match_resolve_kernel(MatchArgs a) {
    __shared__ uint32_t s_cnt[kMatchClasses + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid <= kMatchClasses) s_cnt[tid] = 0;
    __syncthreads();
    if (blockIdx.x < a.rtiles) {
        const uint64_t r = uint64_t(blockIdx.x) * kMatchTile + tid;
        const bool active = r < a.n;
        uint32_t cls = kMatchClasses;                              // (no record: no class)
        if (active) {
            uint32_t m = a.match[r];
            uint64_t tag = 0;
            if (m < ONC_MATCH_FAILED) {                            // a lead
                if (a.first_rec[m] != uint32_t(r)) {
                    m = ONC_MATCH_DUPLICATE;
                    a.match[r] = m;
                } else if (a.tag_out) {
                    tag = gload<uint64_t>(reinterpret_cast<uintptr_t>(a.pending + m) + 8);
                }
            }
            if (a.tag_out) a.tag_out[r] = tag;
            cls = match_result_class(m);
        }
#pragma unroll
        for (uint32_t c = 0; c < kMatchClasses; ++c) {
            const uint64_t b = __ballot(cls == c);
            if (lane == 0 && b) atomicAdd(&s_cnt[c], uint32_t(__popcll(b)));
        }
        __syncthreads();
        if (tid < kMatchClasses) a.rec_counts[bin_count_at(tid, blockIdx.x, a.rtiles)] = s_cnt[tid];
    } else {
        const uint64_t tile = uint64_t(blockIdx.x) - a.rtiles;
        const uint64_t p = tile * kMatchTile + tid;
        bool waiting = false;
        if (p < a.np) {
            const uint32_t f = a.first_rec[p];
            a.hit[p] = f;
            waiting = f == kMatchEmpty;
        }
        const uint64_t b = __ballot(waiting);
        if (lane == 0 && b) atomicAdd(&s_cnt[kMatchClasses], uint32_t(__popcll(b)));
        __syncthreads();
        if (tid == 0) a.pend_counts[tile] = s_cnt[kMatchClasses];
    }
}

// pend_counts[t] := the unanswered entries in the tiles before t; result.
__global__ __launch_bounds__(kMtThreads) void match_scan_kernel(MatchArgs a) {
    __shared__ uint64_t s_wave[kMtWaves];
    __shared__ uint64_t s_sum[kMatchClasses];
    const uint32_t tid = threadIdx.x;
    const uint64_t waiting = scan_bin_row<kMtThreads>(a.pend_counts, a.ptiles, s_wave);    // (np < 2^32)
    for (uint32_t c = 0; c < kMatchClasses; ++c) {
        uint64_t v = 0;
        for (uint64_t t = tid; t < a.rtiles; t += kMtThreads) v += a.rec_counts[bin_count_at(c, t, a.rtiles)];
        const uint64_t total = block_sum_u64<kMtThreads>(v, s_wave);
        if (tid == 0) s_sum[c] = total;
    }
    if (tid == 0) {
        for (uint32_t c = 0; c < kMatchClasses; ++c) a.result[c] = s_sum[c];
        a.result[kMatchClasses] = waiting;
    }
}

__global__ __launch_bounds__(kMtThreads) void match_compact_kernel(MatchArgs a) {
    __shared__ uint32_t s_wcnt[kMtWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t p = uint64_t(blockIdx.x) * kMatchTile + tid;
    const bool waiting = p < a.np && a.first_rec[p] == kMatchEmpty;
    const uint64_t b = __ballot(waiting);
    if (lane == 0) s_wcnt[wave] = uint32_t(__popcll(b));
    __syncthreads();
    if (!waiting) return;
    uint64_t k = a.pend_counts[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) k += s_wcnt[w];
    k += uint32_t(__popcll(b & ((1ull << lane) - 1)));
    reinterpret_cast<u32x4*>(a.still)[k] = gload<u32x4>(reinterpret_cast<uintptr_t>(a.pending + p));
}

hipError_t launch_match_clear(const MatchArgs& a, hipStream_t s) {
    const uint64_t granules = a.clear_words / 4;
    const uint64_t wgs = (granules + kMtClearThreads - 1) / kMtClearThreads;
    ONC_LAUNCH(match_clear_kernel, dim3(uint32_t(wgs)), dim3(kMtClearThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_insert(const MatchArgs& a, hipStream_t s) {
    ONC_LAUNCH(match_insert_kernel, dim3(uint32_t(a.ptiles)), dim3(kMtThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_probe(const MatchArgs& a, hipStream_t s) {
    ONC_LAUNCH(match_probe_kernel, dim3(uint32_t(a.rtiles)), dim3(kMtThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_resolve(const MatchArgs& a, hipStream_t s) {
    ONC_LAUNCH(match_resolve_kernel, dim3(uint32_t(a.rtiles + a.ptiles)), dim3(kMtThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_scan(const MatchArgs& a, hipStream_t s) {
    ONC_LAUNCH(match_scan_kernel, dim3(1), dim3(kMtThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_compact(const MatchArgs& a, hipStream_t s) {
    ONC_LAUNCH(match_compact_kernel, dim3(uint32_t(a.ptiles)), dim3(kMtThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
