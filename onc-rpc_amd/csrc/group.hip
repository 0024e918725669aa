// group.hip — a send batch grouped by connection on gfx950 (onc_group_by_conn
// and onc_conn_extents, include/onc_rpc.h): a stable least-significant-digit
// radix sort of (key, index) pairs, key = the item's clamped connection id,
// with 8-bit digits; each pass is partition.h's stable partition, a digit's
// 256 values its bins.
//
//   group_identity     no pass (nconn == 0): order[k] = k.
//   per pass p (group_plan.h):
//   group_count        the partition's count over tiles of kGroupTile items.
//                      Pass 0 reads rec_conn through via and clamps; later
//                      passes read the pairs the pass before wrote, in
//                      sequence.
//   group_scan_digits  the partition's scan, a row per digit; its total kept.
//   group_scan_total   one workgroup: the 256 totals scanned into first[].
//   group_scatter      the partition's scatter: the items read again, and the
//                      pair goes to its slot. The last pass writes the index
//                      into the caller's order.
//   group_bounds       a lane per entry of conn_first: a lower-bound binary
//                      search of the sorted keys (32 steps at most). A
//                      workgroup takes runs of 255 entries and the one behind
//                      them, so that each entry sees its group's end, and
//                      counts its non-empty groups into the scratch.
//   group_result       one workgroup: the partial counts summed; result.
//   group_gather       only with msgs_out: four consecutive lanes on the four
//                      16-byte pieces of descriptor msgs[order[j]] ->
//                      msgs_out[j]; a wave stores 1 KiB without a gap.
//   conn_extents       a lane per entry: conn_off[c] = rec_off[min(conn_first[c], nrec)].
//
// No workgroup waits for another: the launch boundary is the only barrier
// between them, and inside a launch every workgroup reads only what an earlier
// launch wrote. Caller arrays see plain loads and stores only.
#include <algorithm>

#include "group_plan.h"
#include "kernels.h"
#include "partition.h"

namespace onc {

constexpr int kGrThreads = int(kGroupTile);
constexpr int kGrWaves = kGrThreads / 64;
constexpr int kGrDigits = int(kGroupDigits);
constexpr int kGrFlat = 256;                   // threads of the lane-per-element kernels
constexpr int kGrRun = kGrFlat - 1;            // conn_first entries a bounds workgroup writes per round
static_assert(kGroupTile == ONC_GROUP_TILE, "the tile the header names");
static_assert(kGrFlat * kGroupTile == 262144,
              "a round of group_scan_digits: tests/test_gpu_scan_rounds.py reaches rounds two and three by it");
static_assert(kGrDigits == kGrFlat, "the scans take a digit per thread");

struct GrItem {
    uint32_t key, idx;
};
// Item k of this pass (k < a.n).
__device__ __forceinline__ GrItem gr_item(const GroupArgs& a, uint64_t k) {
    if (a.pass != 0) return GrItem{a.src_key[k], a.src_idx[k]};
    const uint64_t s = a.via ? uint64_t(a.via[k]) : k;
    const uint32_t c = s < a.nsrc ? a.rec_conn[s] : a.nconn;      // an index outside rec_conn is never read
    return GrItem{group_clamp(c, a.nconn), uint32_t(k)};
}

__global__ __launch_bounds__(kGrFlat) void group_identity_kernel(GroupArgs a) {
    for (uint64_t k = uint64_t(blockIdx.x) * kGrFlat + threadIdx.x; k < a.n; k += uint64_t(gridDim.x) * kGrFlat)
        a.order[k] = uint32_t(k);
}

__global__ __launch_bounds__(kGrThreads) void group_count_kernel(GroupArgs a) {
    __shared__ uint32_t s_cnt[kGrDigits];
    const uint32_t tid = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {      // (one round below 2^31 items)
        if (tid < kGrDigits) s_cnt[tid] = 0;
        __syncthreads();
        const uint64_t k = tile * kGroupTile + tid;
        const bool active = k < a.n;
        const uint32_t digit = active ? group_digit(gr_item(a, k).key, a.pass) : 0u;
        tile_count_add(s_cnt, digit, active, wave_peers(digit, active, a.digit_bits));
        __syncthreads();
        if (tid < kGrDigits) a.counts[bin_count_at(tid, tile, a.tiles)] = s_cnt[tid];
    }
}

// counts[digit][t] := the digit's items in the tiles before t; totals[digit].
__global__ __launch_bounds__(kGrFlat) void group_scan_digits_kernel(GroupArgs a) {
    __shared__ uint64_t s_wave[kGrFlat / 64];
    const uint32_t digit = blockIdx.x;
    const uint64_t total = scan_bin_row<kGrFlat>(a.counts + bin_count_at(digit, 0, a.tiles), a.tiles, s_wave);
    if (threadIdx.x == 0) a.totals[digit] = uint32_t(total);       // (n < 2^32)
}

__global__ __launch_bounds__(kGrFlat) void group_scan_total_kernel(GroupArgs a) {
    __shared__ uint64_t s_wave[kGrFlat / 64];
    uint64_t total;
    const uint64_t ex = block_excl_scan_u64<kGrFlat>(a.totals[threadIdx.x], s_wave, &total);
    a.first[threadIdx.x] = uint32_t(ex);
}

__global__ __launch_bounds__(kGrThreads) void group_scatter_kernel(GroupArgs a) {
    __shared__ uint32_t s_wcnt[kGrWaves][kGrDigits];
    const uint32_t tid = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {      // (one round below 2^31 items)
        __syncthreads();        // the round before has read s_wcnt
        const uint64_t k = tile * kGroupTile + tid;
        const bool active = k < a.n;
        const GrItem it = active ? gr_item(a, k) : GrItem{0u, 0u};
        const uint32_t digit = active ? group_digit(it.key, a.pass) : 0u;
        // (d: where the tile's items of digit d start)
        const uint64_t j = scatter_slot(s_wcnt, digit, active, wave_peers(digit, active, a.digit_bits), kGrDigits,
                                        [&](uint32_t d) { return a.first[d] + a.counts[bin_count_at(d, tile, a.tiles)]; });
        // (j >= n only if the caller's arrays changed between the count and here)
        if (active && j < a.n) {
            a.dst_key[j] = it.key;
            a.dst_idx[j] = it.idx;
        }
    }
}

__global__ __launch_bounds__(kGrFlat) void group_bounds_kernel(GroupArgs a) {
    __shared__ uint64_t s_lb[kGrFlat];
    __shared__ uint32_t s_active;
    const uint32_t tid = threadIdx.x;
    const uint64_t entries = uint64_t(a.nconn) + 2;
    if (tid == 0) s_active = 0;
    uint32_t mine = 0;
    // (the rounds depend on nconn and the grid only: every thread takes them all)
    for (uint64_t run = blockIdx.x; run * kGrRun < entries; run += gridDim.x) {
        const uint64_t c = run * kGrRun + tid;
        uint64_t lb = 0;
        if (c < entries) lb = a.passes ? group_lower_bound(a.sorted_key, a.n, uint32_t(c)) : (c == 0 ? 0ull : a.n);
        __syncthreads();        // the round before has read s_lb
        s_lb[tid] = lb;
        __syncthreads();
        if (tid < kGrRun && c < entries) {
            a.conn_first[c] = lb;
            if (c < a.nconn && s_lb[tid + 1] > lb) ++mine;
        }
    }
    __syncthreads();
    if (mine) atomicAdd(&s_active, mine);
    __syncthreads();
    if (tid == 0) a.partial[blockIdx.x] = s_active;
}

__global__ __launch_bounds__(kGrFlat) void group_result_kernel(GroupArgs a) {
    __shared__ uint64_t s_wave[kGrFlat / 64];
    uint64_t v = 0;
    for (uint32_t g = threadIdx.x; g < a.bounds_groups; g += kGrFlat) v += a.partial[g];
    const uint64_t total = block_sum_u64<kGrFlat>(v, s_wave);
    if (threadIdx.x < 3) {
        const uint64_t sent = a.passes ? group_lower_bound(a.sorted_key, a.n, a.nconn) : 0ull;
        a.result[threadIdx.x] = threadIdx.x == 0 ? sent : threadIdx.x == 1 ? a.n - sent : total;
    }
}

__global__ __launch_bounds__(kGrFlat) void group_gather_kernel(GroupArgs a) {
    for (uint64_t g = uint64_t(blockIdx.x) * kGrFlat + threadIdx.x; (g >> 2) < a.n; g += uint64_t(gridDim.x) * kGrFlat) {
        const uint64_t j = g >> 2;
        const uint64_t piece = 16ull * (g & 3u);
        const uint64_t r = a.order[j];
        if (r >= a.n) continue;     // (order is the caller's: only if it changed under the call)
        const u32x4 q = gload<u32x4>(reinterpret_cast<uintptr_t>(a.msgs + r) + piece);
        *reinterpret_cast<u32x4*>(reinterpret_cast<uintptr_t>(a.msgs_out + j) + piece) = q;
    }
}

__global__ __launch_bounds__(kGrFlat) void conn_extents_kernel(const uint64_t* rec_off, uint64_t nrec,
                                                               const uint64_t* conn_first, uint64_t entries,
                                                               uint64_t* conn_off) {
    const uint64_t c = uint64_t(blockIdx.x) * kGrFlat + threadIdx.x;
    if (c >= entries) return;
    const uint64_t f = conn_first[c];
    conn_off[c] = rec_off[f < nrec ? f : nrec];
}

// A launch stays below 2^31 threads; the kernels walk what is beyond that.
static inline dim3 gr_flat_grid(uint64_t lanes) {
    return dim3(uint32_t(std::min<uint64_t>((lanes + kGrFlat - 1) / kGrFlat, (1ull << 31) / kGrFlat)));
}
static inline dim3 gr_tile_grid(uint64_t tiles) { return dim3(uint32_t(std::min<uint64_t>(tiles, (1ull << 31) / kGrThreads))); }

uint32_t group_bounds_groups(uint32_t nconn) {
    const uint64_t runs = (uint64_t(nconn) + 2 + kGrRun - 1) / kGrRun;
    return uint32_t(runs < kGroupBoundsGroups ? runs : kGroupBoundsGroups);
}

hipError_t launch_group_identity(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_identity_kernel, gr_flat_grid(a.n), dim3(kGrFlat), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_count(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_count_kernel, gr_tile_grid(a.tiles), dim3(kGrThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_scan_digits(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_scan_digits_kernel, dim3(kGrDigits), dim3(kGrFlat), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_scan_total(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_scan_total_kernel, dim3(1), dim3(kGrFlat), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_scatter(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_scatter_kernel, gr_tile_grid(a.tiles), dim3(kGrThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_bounds(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_bounds_kernel, dim3(a.bounds_groups), dim3(kGrFlat), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_result(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_result_kernel, dim3(1), dim3(kGrFlat), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_gather(const GroupArgs& a, hipStream_t s) {
    ONC_LAUNCH(group_gather_kernel, gr_flat_grid(4 * a.n), dim3(kGrFlat), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_conn_extents(const uint64_t* rec_off, uint64_t nrec, const uint64_t* conn_first, uint32_t nconn,
                               uint64_t* conn_off, hipStream_t s) {
    const uint64_t entries = uint64_t(nconn) + 2;
    ONC_LAUNCH(conn_extents_kernel, gr_flat_grid(entries), dim3(kGrFlat), 0, s, rec_off, nrec, conn_first, entries,
               conn_off);
    return hipGetLastError();
}

}  // namespace onc
