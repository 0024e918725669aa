// partition.h — the stable partition that route.hip (by handler bin) and
// group.hip (by one 8-bit digit of the key, per radix pass) share; match.hip
// uses its row scan and does the one-bin scatter in its own shape. Device
// code for the .hip files only, as tile_walk.h; the index arithmetic is
// partition_plan.h's.
//
// An element of bin b goes to first[b] + the number of b's elements before it,
// counted in the order bin, then tile, then wave, then rank:
//   count    a workgroup per tile, a lane per element: a wave's lanes of one bin
//            by a ballot per bin bit (wave_peers), the lowest adding their
//            number to the tile's count in LDS (tile_count_add); the counts go
//            to the scratch bin-major, at bin_count_at(bin, tile, tiles).
//   scan     a workgroup per bin: its row of counts scanned in place, exclusive
//            (scan_bin_row); the rows' totals scanned in bin order are first[].
//   scatter  a workgroup per tile: the waves' counts per bin turned into starts
//            in wave order on top of first[bin] + counts[bin][tile]; the slot
//            is the wave's start plus the rank among the peers (scatter_slot).
// Elements ascend with tile, wave and lane, so two of one bin keep their order:
// the partition is stable.
#pragma once

#include "common.h"
#include "partition_plan.h"

namespace onc {

// The wave's active lanes of this lane's bin; nbits: the bits a bin has.
__device__ __forceinline__ uint64_t wave_peers(uint32_t bin, bool active, uint32_t nbits) {
    uint64_t m = __ballot(active);
    for (uint32_t k = 0; k < nbits; ++k) {
        const bool bit = (bin >> k) & 1u;
        const uint64_t b = __ballot(bit);
        m &= bit ? b : ~b;
    }
    return m;
}

// The tile's count of each bin in s_cnt (LDS; zeroed, and fenced on both
// sides, by the caller): the lowest peer adds all of them.
__device__ __forceinline__ void tile_count_add(uint32_t* s_cnt, uint32_t bin, bool active, uint64_t peers) {
    const uint32_t lane = threadIdx.x & 63u;
    if (active && (peers & ((1ull << lane) - 1)) == 0) atomicAdd(&s_cnt[bin], uint32_t(__popcll(peers)));
}

// row[t] := row[0] + ... + row[t - 1] for a row of `tiles` counts, in rounds
// of NT threads with the carry between them; returns the row's total. Holds
// __syncthreads(): the whole workgroup calls it, unconditionally.
template <int NT>
__device__ __forceinline__ uint64_t scan_bin_row(uint32_t* row, uint64_t tiles, uint64_t* s_wave) {
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < tiles; t0 += NT) {
        const uint64_t t = t0 + threadIdx.x;
        const uint64_t v = t < tiles ? row[t] : 0ull;
        uint64_t total;
        const uint64_t ex = block_excl_scan_u64<NT>(v, s_wave, &total);
        if (t < tiles) row[t] = uint32_t(carry + ex);              // (a row sums to below 2^32)
        carry += total;
    }
    return carry;
}

// This lane's slot in the output. s_wcnt (LDS) is zeroed here, takes each
// wave's count per bin from its lowest peers, and thread b < bins turns column
// b into starts in wave order on top of base(b): the caller's first[b] +
// counts[b][this tile]. A workgroup of W waves. Holds __syncthreads(): the
// whole workgroup calls it, unconditionally (an inactive lane's slot is void).
template <int W, int B, class Base>
__device__ __forceinline__ uint64_t scatter_slot(uint32_t (&s_wcnt)[W][B], uint32_t bin, bool active, uint64_t peers,
                                                 uint32_t bins, Base base) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < W * B; i += W * 64) (&s_wcnt[0][0])[i] = 0;
    __syncthreads();
    const uint32_t rank = uint32_t(__popcll(peers & ((1ull << lane) - 1)));
    if (active && rank == 0) s_wcnt[wave][bin] = uint32_t(__popcll(peers));
    __syncthreads();
    if (tid < bins) {
        uint32_t at = base(tid);
        for (int w = 0; w < W; ++w) {
            const uint32_t c = s_wcnt[w][tid];
            s_wcnt[w][tid] = at;
            at += c;
        }
    }
    __syncthreads();
    return uint64_t(s_wcnt[wave][bin]) + rank;
}

}  // namespace onc
