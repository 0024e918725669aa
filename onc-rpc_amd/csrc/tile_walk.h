// tile_walk.h — what the copy kernels share (defrag_copy, frag_copy,
// fragiov_fill, gather_copy, place_copy): the block scan of a plan's
// aggregate, the searches of a sorted array of positions, and the walk of a
// wave over its run of output tiles. Device code, for the .hip files only:
// the *_plan.h headers stay free of intrinsics (the host probes compile them).
#pragma once

#include "common.h"

namespace onc {

constexpr int kCopyThreads = 256;          // per workgroup of a plan or copy kernel: four waves
static_assert(kCopyThreads * kCopyThreads == 65536,
              "a round of scan_blocks: tests/test_gpu_scan_rounds.py reaches rounds two and three by this number");
constexpr uint32_t kCopyStage = 128;       // entries of a tile kept in LDS (more: searched in global memory)
constexpr uint32_t kCopyMaxBlocks = 2048;  // workgroups of a copy kernel (the tiles are dealt out among their waves)

// ---------------------------------------------------------------------------
// Block scan of an aggregate
// ---------------------------------------------------------------------------
// An aggregate is a struct of 64-bit words (DefragAgg, FragAgg, ...) with an
// identity and an associative join; Ops names them: Ops::Agg, Ops::none(),
// Ops::join(a, b) (a before b).

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), d, 64));
    const uint32_t hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), d, 64));
    return uint64_t(lo) | (uint64_t(hi) << 32);
}
template <class Agg>
__device__ __forceinline__ Agg shfl_up_agg(const Agg& v, int d) {
    static_assert(sizeof(Agg) % 8 == 0 && alignof(Agg) == 8, "an aggregate is 64-bit words");
    uint64_t w[sizeof(Agg) / 8];
    __builtin_memcpy(w, &v, sizeof(Agg));
#pragma unroll
    for (size_t i = 0; i < sizeof(Agg) / 8; ++i) w[i] = shfl_up_u64(w[i], d);
    Agg r;
    __builtin_memcpy(&r, w, sizeof(Agg));
    return r;
}

// The join of the block's elements before this thread's; *total = the block.
// s_wave: NT / 64 aggregates in LDS.
template <class Ops, int NT = kCopyThreads>
__device__ __forceinline__ typename Ops::Agg block_excl(const typename Ops::Agg& v, typename Ops::Agg* s_wave,
                                                        typename Ops::Agg* total) {
    using Agg = typename Ops::Agg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Agg incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Agg o = shfl_up_agg(incl, d);
        if (lane >= d) incl = Ops::join(o, incl);
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    Agg base = Ops::none(), sum = Ops::none();
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const Agg t = s_wave[w];
        if (w < wave) base = Ops::join(base, t);
        sum = Ops::join(sum, t);
    }
    *total = sum;
    __syncthreads();   // s_wave is reused by the caller's next round
    Agg prev = shfl_up_agg(incl, 1);
    if (lane == 0) prev = Ops::none();
    return Ops::join(base, prev);
}

// A *_blk kernel's end: blk[this block] := the join of its threads' elements.
template <class Ops>
__device__ __forceinline__ void block_total(const typename Ops::Agg& v, typename Ops::Agg* s_wave,
                                            typename Ops::Agg* blk) {
    typename Ops::Agg total;
    block_excl<Ops>(v, s_wave, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// A *_blkscan kernel (one workgroup): blk[b] := the join of the blocks before
// b; blk[nblk] := the whole batch. Thread 0 then runs `done` (what the next
// kernel expects to find set).
template <class Ops, class Done>
__device__ __forceinline__ void scan_blocks(typename Ops::Agg* blk, uint64_t nblk, typename Ops::Agg* s_wave,
                                            Done done) {
    using Agg = typename Ops::Agg;
    Agg carry = Ops::none();
    for (uint64_t b0 = 0; b0 < nblk; b0 += kCopyThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const Agg v = b < nblk ? blk[b] : Ops::none();
        Agg total;
        const Agg ex = block_excl<Ops>(v, s_wave, &total);
        if (b < nblk) blk[b] = Ops::join(carry, ex);
        carry = Ops::join(carry, total);
    }
    if (threadIdx.x == 0) {
        blk[nblk] = carry;
        done();
    }
}

// ---------------------------------------------------------------------------
// Searches of sorted positions
// ---------------------------------------------------------------------------

// Last j in [0, n) with e[j] <= x (e[0] <= x).
__device__ __forceinline__ uint64_t last_at_or_before(const uint64_t* e, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
// ... with v.pos(j) <= x (v.pos(0) <= x)
template <class View>
__device__ __forceinline__ uint64_t last_at_or_before(const View& v, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (v.pos(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The same for one x per wave (every lane calls it with the same arguments):
// the lanes probe 64 evenly spaced entries per round, so a million entries
// take 4 dependent loads instead of 20. e is sorted: the probes at or before
// x are the lowest lanes', and lane 0's (e[lo] <= x) is always one of them.
__device__ __forceinline__ uint64_t wave_last_at_or_before(const uint64_t* e, uint64_t n, uint64_t x, int lane) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t at = lo + uint64_t(lane) * step;
        const bool ok = at < hi && e[at < hi ? at : hi - 1] <= x;
        const uint64_t c = __popcll(__ballot(ok));   // >= 1
        lo += (c - 1) * step;
        hi = min(lo + step, hi);
    }
    return lo;
}

// What walk_tiles walks over: entry j's position, and the last of the entries
// [j0, j0 + n) at or before x, counted from j0. A plain sorted array, searched
// by every lane for itself or by the wave together:
struct SortedArray {
    const uint64_t* e;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return e[j]; }
    __device__ __forceinline__ uint64_t search(uint64_t j0, uint64_t n, uint64_t x) const {
        return last_at_or_before(e + j0, n, x);
    }
};
struct SortedArrayByWave {
    const uint64_t* e;
    int lane;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return e[j]; }
    __device__ __forceinline__ uint64_t search(uint64_t j0, uint64_t n, uint64_t x) const {
        return wave_last_at_or_before(e + j0, n, x, lane);
    }
};

// ---------------------------------------------------------------------------
// The walk
// ---------------------------------------------------------------------------

// What a tile handler does between staging its own columns in LDS and
// reading them (and the walk's window) back: the wave's LDS writes are done.
__device__ __forceinline__ void wave_stage_done() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The output is cut into tiles of kTile units (bytes of a stream, pieces of a
// list) and partitioned by them, never by entry count: an entry (a fragment, a
// record, a piece) may be empty or many MiB. The entries' positions
// ent.pos(0 .. N) are sorted, pos(0) <= every position asked for and pos(N) >=
// every end; an empty entry starts where the next one does, so the last entry
// starting at or before a unit holds it. Tile T is the units [T kTile,
// (T + 1) kTile) of a coordinate in which the output is [D0, D1) (bytes: from
// the 16-byte aligned address at or below the caller's buffer, so that every
// full store is aligned); unit D of it is position D + shift (mod 2^64).
//
// Every wave takes a run of consecutive tiles, so that only its first tile
// searches the entries in global memory (about 20 dependent loads: with a
// search per tile defrag_copy spent a quarter of its time there). From then
// on the tile's entries are found in a window of kCopyStage + 1 consecutive
// positions staged in LDS (`se`, the wave's own) from entry ja on, the entry
// holding the previous tile's last unit: the positions are sorted, so how many
// of them lie at or before a unit is a ballot count. With c_lo of the window
// at or before the tile's first position `lo` and c_hi before its end `hi`:
//   - c_lo = all of them: the tile starts beyond the window (a long run of
//     empty entries). Search on from the window's end and stage again.
//   - c_hi = all of them and the tile's first entry is not the window's first:
//     the window ends inside the tile. Slide it to start at that entry and
//     stage again.
//   - c_hi = all of them still: more than kCopyStage entries reach into the
//     tile. Its last entry jb is searched for and global(ja, jb - ja + 1, t0,
//     lo, hi) handles the tile from global memory; the next tile starts at jb.
//   - else window entries k = c_lo - 1 .. c_hi - 1 reach into the tile:
//     staged(se + k, ja + k, c_hi - k, t0, lo, hi) handles it. se + k holds
//     c_hi - k + 1 positions; the handler stages what else it needs per entry,
//     calls wave_stage_done() and reads both. The next tile starts at the
//     entry holding this one's last unit, which holds the next one's first or
//     comes before it.
// Both handlers get the tile's first unit t0 = T kTile and its positions
// [lo, hi) (clipped to the output, shift added).
template <uint64_t kTile, class Entries, class Staged, class Global>
__device__ __forceinline__ void walk_tiles(const Entries& ent, uint64_t N, uint64_t D0, uint64_t D1, uint64_t shift,
                                           uint64_t* se, Staged staged, Global global) {
    static_assert(kCopyStage == 128, "the window is staged and counted as two rounds of 64 lanes + 1");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t ntiles = (D1 + kTile - 1) / kTile;
    const uint64_t nw = uint64_t(gridDim.x) * (kCopyThreads / 64);
    const uint64_t per = (ntiles + nw - 1) / nw;
    const uint64_t T0 = (uint64_t(blockIdx.x) * (kCopyThreads / 64) + wv) * per;   // wave-uniform
    const uint64_t T1 = min(T0 + per, ntiles);
    if (T0 >= T1) return;
    // ja: an entry with pos(ja) <= the tile's first position (kept across tiles)
    uint64_t ja = ent.search(0, N + 1, max(T0 * kTile, D0) + shift);
    for (uint64_t T = T0; T < T1; ++T) {
        const uint64_t t0 = T * kTile;
        const uint64_t lo = max(t0, D0) + shift, hi = min(t0 + kTile, D1) + shift;
        uint32_t k, c_hi;
        for (;;) {
            __builtin_amdgcn_wave_barrier();   // the tile before may still read the stage
            // (past the last entry the window repeats pos(N) >= hi: never counted)
            const uint64_t e0 = ent.pos(min(ja + lane, N)), e1 = ent.pos(min(ja + 64 + lane, N));
            const uint64_t e2 = ent.pos(min(ja + kCopyStage, N));
            se[lane] = e0;
            se[64 + lane] = e1;
            if (lane == 0) se[kCopyStage] = e2;
            const uint32_t c_lo = __popcll(__ballot(e0 <= lo)) + __popcll(__ballot(e1 <= lo)) + (e2 <= lo ? 1u : 0u);
            c_hi = __popcll(__ballot(e0 < hi)) + __popcll(__ballot(e1 < hi)) + (e2 < hi ? 1u : 0u);
            if (c_lo == kCopyStage + 1) {      // the tile starts beyond the window: search on from its end
                ja += kCopyStage;
                ja += ent.search(ja, N + 1 - ja, lo);
                continue;
            }
            k = c_lo - 1;                      // window entry of the entry holding the tile's first unit
            if (c_hi == kCopyStage + 1 && k != 0) {   // the window ends inside the tile: start it at that entry
                ja += k;
                continue;
            }
            break;
        }
        if (c_hi == kCopyStage + 1) {
            // more than kCopyStage entries reach into the tile: in global memory
            const uint64_t jb = ja + kCopyStage + ent.search(ja + kCopyStage, N + 1 - ja - kCopyStage, hi - 1);
            global(ja, jb - ja + 1, t0, lo, hi);
            ja = jb;
            continue;
        }
        staged(se + k, ja + k, c_hi - k, t0, lo, hi);
        ja += c_hi - 1;
    }
}

// A copy launcher's grid before its maximum: the workgroups, at per_wg units
// each, that cover the capacity from `origin` on (what of it is written is
// known on the device only). The capacity is clamped so that the sum cannot
// wrap.
inline uint64_t copy_groups(uint64_t origin, uint64_t capacity, uint64_t per_wg) {
    const uint64_t cap = capacity > ~0ull - 16 - per_wg ? ~0ull - 16 - per_wg : capacity;
    return (origin + cap + per_wg - 1) / per_wg;
}

}  // namespace onc
