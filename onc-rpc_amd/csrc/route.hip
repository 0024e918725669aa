// route.hip — decoded Calls dispatched to their handlers on gfx950
// (onc_route_calls, include/onc_rpc.h): a stable multi-way partition of the
// records by bin (the handlers, then rejected, not-a-Call, failed), with a
// table lookup in front of it and a 64-byte descriptor gather behind it. The
// partition (count, scan, scatter) is partition.h's.
//
//   route_classify    a workgroup per tile of kRouteTile records. The table is
//                     staged in LDS and validated by every workgroup (an entry
//                     per thread, the first bad one by an LDS minimum), so that
//                     none writes anything for a bad table; the first
//                     publishes bad + 1 in result[3]. A lane per record: its
//                     status and, for an OK record only, the descriptor's
//                     first two 16-byte granules (msg_type, program, version |
//                     procedure); binary search of the table (route_plan.h);
//                     route[r]. The partition's count.
//   route_scan_bins   the partition's scan, a row per bin; its total kept.
//   route_scan_total  one workgroup: the totals scanned into bin_first, and
//                     result[0 .. 2]. For a bad table: zeros.
//   route_scatter     the partition's scatter over route[] re-read: slot k;
//                     order[k], calls_out[k] (four 16-byte loads and stores)
//                     and replies[k] (four 16-byte stores). A reply is built
//                     from the descriptor's xid and the bin; for a rejected
//                     Call stat, low and high are derived again from the
//                     table in LDS (staged only when replies are asked for):
//                     nothing is carried in route[] or in a side array.
//
// No workgroup waits for another: the launch boundary is the only barrier
// between them, and inside a launch every workgroup reads only what an earlier
// launch wrote.
#include "kernels.h"
#include "partition.h"
#include "route_plan.h"

namespace onc {

constexpr int kRtThreads = int(kRouteTile);
constexpr int kRtWaves = kRtThreads / 64;
constexpr int kRtBinsMax = 256;
constexpr int kRtScanThreads = 256;
static_assert(kRouteTile == ONC_ROUTE_TILE, "the tile the header names");
static_assert(kRtScanThreads * kRouteTile == 262144,
              "a round of route_scan_bins: tests/test_gpu_scan_rounds.py reaches rounds two and three by it");
static_assert(ONC_ROUTE_HANDLERS_MAX + 3 <= kRtBinsMax, "a bin is 8 bits");
static_assert(ONC_ROUTE_TABLE_MAX <= kRouteTile, "the table is validated an entry per thread");
static_assert(sizeof(onc_route) == 24, "staged as six words an entry");

// The table into LDS (it is only 4-byte aligned: word by word).
__device__ __forceinline__ void rt_stage(const RouteArgs& a, onc_route* s_tab) {
    const uintptr_t src = reinterpret_cast<uintptr_t>(a.table);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_tab);
    for (uint32_t w = threadIdx.x; w < 6u * a.ntab; w += kRtThreads) dst[w] = gload<uint32_t>(src + 4ull * w);
}

__device__ __forceinline__ uint32_t rt_bits(uint32_t bins) { return 32u - __builtin_clz(bins - 1); }   // bins >= 3

__global__ __launch_bounds__(kRtThreads) void route_classify_kernel(RouteArgs a) {
    __shared__ onc_route s_tab[ONC_ROUTE_TABLE_MAX];
    __shared__ uint32_t s_cnt[kRtBinsMax];
    __shared__ uint32_t s_bad;
    const uint32_t tid = threadIdx.x;
    const uint32_t bins = route_bins(a.nh);
    rt_stage(a, s_tab);
    if (tid < kRtBinsMax) s_cnt[tid] = 0;
    if (tid == 0) s_bad = ~0u;
    __syncthreads();
    if (tid < a.ntab && route_bad_at(s_tab, a.ntab, a.nh, tid)) atomicMin(&s_bad, tid);
    __syncthreads();
    const uint32_t bad = s_bad;
    if (blockIdx.x == 0 && tid == 0) a.result[3] = bad == ~0u ? 0ull : uint64_t(bad) + 1;
    if (bad != ~0u || blockIdx.x >= a.tiles) return;              // (no records: the one workgroup validates)
    const uint64_t r = uint64_t(blockIdx.x) * kRouteTile + tid;
    const bool active = r < a.n;
    uint32_t bin = 0;
    if (active) {
        const int32_t st = a.status[r];
        uint32_t msg_type = 0, call = 0;
        if (st == ONC_OK) {
            const uintptr_t m = reinterpret_cast<uintptr_t>(a.msgs + r);
            const u32x4 q0 = gload<u32x4>(m), q1 = gload<u32x4>(m + 16);
            msg_type = q0.y & 0xFFu;
            if (msg_type == ONC_MSG_CALL) call = route_lookup(s_tab, a.ntab, a.nh, q0.z, q0.w, q1.x).bin;
        }
        bin = route_bin(st, msg_type, call, a.nh);
        a.route[r] = bin;
    }
    tile_count_add(s_cnt, bin, active, wave_peers(bin, active, rt_bits(bins)));
    __syncthreads();
    if (tid < bins) a.counts[bin_count_at(tid, blockIdx.x, a.tiles)] = s_cnt[tid];
}

// counts[bin][t] := the bin's records in the tiles before t; totals[bin].
__global__ __launch_bounds__(kRtScanThreads) void route_scan_bins_kernel(RouteArgs a) {
    __shared__ uint64_t s_wave[kRtScanThreads / 64];
    if (a.result[3] != 0) return;                                  // a bad table: nothing was counted
    const uint32_t bin = blockIdx.x;
    const uint64_t total = scan_bin_row<kRtScanThreads>(a.counts + bin_count_at(bin, 0, a.tiles), a.tiles, s_wave);
    if (threadIdx.x == 0) a.totals[bin] = uint32_t(total);         // (n < 2^32)
}

__global__ __launch_bounds__(kRtScanThreads) void route_scan_total_kernel(RouteArgs a) {
    __shared__ uint64_t s_wave[kRtScanThreads / 64];
    __shared__ uint64_t s_first[kRtBinsMax + 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t bins = route_bins(a.nh);
    const bool bad = a.result[3] != 0;
    const uint64_t v = (tid < bins && !bad) ? a.totals[tid] : 0ull;
    uint64_t total;
    const uint64_t ex = block_excl_scan_u64<kRtScanThreads>(v, s_wave, &total);
    if (tid < bins) s_first[tid] = ex;
    if (tid == 0) s_first[bins] = total;
    __syncthreads();
    for (uint32_t b = tid; b <= bins; b += kRtScanThreads) a.bin_first[b] = s_first[b];
    if (tid == 0) {
        a.result[0] = s_first[a.nh];
        a.result[1] = s_first[a.nh + 1] - s_first[a.nh];
        a.result[2] = s_first[a.nh + 3] - s_first[a.nh + 1];
    }
}

__global__ __launch_bounds__(kRtThreads) void route_scatter_kernel(RouteArgs a) {
    __shared__ onc_route s_tab[ONC_ROUTE_TABLE_MAX];
    __shared__ uint32_t s_wcnt[kRtWaves][kRtBinsMax];
    if (a.result[3] != 0) return;                                  // a bad table: nothing is written
    const uint32_t tid = threadIdx.x;
    const uint32_t bins = route_bins(a.nh);
    if (a.replies) rt_stage(a, s_tab);                             // (scatter_slot's barriers stand behind it)
    const uint64_t r = uint64_t(blockIdx.x) * kRouteTile + tid;
    const bool active = r < a.n;
    const uint32_t bin = active ? a.route[r] : 0u;
    const uint64_t k = scatter_slot(s_wcnt, bin, active, wave_peers(bin, active, rt_bits(bins)), bins, [&](uint32_t b) {
        return uint32_t(a.bin_first[b]) + a.counts[bin_count_at(b, blockIdx.x, a.tiles)];   // bin b's start in the tile
    });
    if (!active) return;
    a.order[k] = uint32_t(r);
    if (!a.calls_out && !a.replies) return;
    const uintptr_t src = reinterpret_cast<uintptr_t>(a.msgs + r);
    if (a.calls_out) {
        const MsgRegs m = issue_msg(a.msgs + r);
        u32x4* q = reinterpret_cast<u32x4*>(a.calls_out + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = m.q[i];
    }
    if (a.replies) {
        u32x4 head = {0u, 0u, 0u, 0u};
        if (bin <= a.nh) {                                         // an OK Call: served or rejected
            const u32x4 q0 = gload<u32x4>(src);
            RouteOutcome o{bin, ONC_ACCEPT_SUCCESS, 0, 0};
            if (bin == a.nh) o = route_lookup(s_tab, a.ntab, a.nh, q0.z, q0.w, gload<uint32_t>(src + 16));
            head.x = q0.x;
            head.y = ONC_MSG_REPLY | (ONC_REPLY_ACCEPTED << 8) | (o.stat << 16);
            head.z = o.low;
            head.w = o.high;
        }
        // (the rest is zero: reserved, payload_len / payload_off, cred, and
        // the verifier AuthNone(None) = {0, ONC_AUTH_PACK(ONC_KIND_NONE, 0), 0})
        static_assert(ONC_AUTH_PACK(ONC_KIND_NONE, 0) == 0, "AuthNone(None) is sixteen zero bytes");
        u32x4* q = reinterpret_cast<u32x4*>(a.replies + k);
        const u32x4 zero = {0u, 0u, 0u, 0u};
        q[0] = head;
        q[1] = zero;
        q[2] = zero;
        q[3] = zero;
    }
}

hipError_t launch_route_classify(const RouteArgs& a, hipStream_t s) {
    const uint64_t wgs = a.tiles ? a.tiles : 1;
    ONC_LAUNCH(route_classify_kernel, dim3(uint32_t(wgs)), dim3(kRtThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_scan_bins(const RouteArgs& a, hipStream_t s) {
    ONC_LAUNCH(route_scan_bins_kernel, dim3(route_bins(a.nh)), dim3(kRtScanThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_scan_total(const RouteArgs& a, hipStream_t s) {
    ONC_LAUNCH(route_scan_total_kernel, dim3(1), dim3(kRtScanThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_scatter(const RouteArgs& a, hipStream_t s) {
    ONC_LAUNCH(route_scatter_kernel, dim3(uint32_t(a.tiles)), dim3(kRtThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
