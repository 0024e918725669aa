// gather.hip — a piece list written as one stream on gfx950
// (onc_piece_offsets / onc_gather_pieces, include/onc_rpc.h): what a writev()
// of onc_fragment_iov's pieces sends, put into one contiguous buffer by the
// device, a window of the stream at a time.
//
// A piece is `len` bytes at byte `off` of one of three sources (the marks,
// the header buffer, the payload arena); the stream is the pieces back to
// back. Lengths, then scan, then copy, as the rest of the library:
//
//   gath_blk      per 256 pieces: the block's {stream bytes, bad pieces, first
//                 bad piece} (gather_plan.h GatherAgg)
//   gath_blkscan  one workgroup: exclusive scan of the block sums
//   gath_apply    per piece: piece_pos; the last piece: piece_pos[npieces] and
//                 result (gath_empty: the same two for a list of no pieces)
//   gather_copy   the hot path: defrag_copy (defrag.hip) with three source
//                 bases instead of one wire and no mark to synthesise. A wave
//                 per 8 KiB tile of the *window* (of `out`, so that every
//                 store is aligned), each wave a run of consecutive tiles; the
//                 pieces reaching into the tile are found by one binary
//                 search of piece_pos at the run's start and followed from
//                 there, and staged in LDS: stream position, source address
//                 and how many bytes of it may be read (0 for a bad piece).
//                 A 16-byte output chunk inside one OK piece is one unaligned
//                 16-byte load and one aligned 16-byte store; the ends of the
//                 window, chunks that span pieces and bad pieces go byte by
//                 byte, the chunk's byte loads in flight together. A piece of
//                 no bytes starts where the next one does, so the last piece
//                 starting at or before a byte holds it.
#include "common.h"
#include "gather_plan.h"
#include "kernels.h"

namespace onc {

constexpr int kGaThreads = 256;
constexpr uint64_t kGaTile = 8192;      // output bytes per wave and step
constexpr uint32_t kGaStage = 128;      // pieces of a tile kept in LDS (more: searched in global memory)
constexpr uint32_t kGaMaxBlocks = 2048; // gather_copy workgroups (the tiles are dealt out among their waves)

__device__ __forceinline__ uint64_t ga_shfl_up(uint64_t v, int d) {
    const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), d, 64));
    const uint32_t hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), d, 64));
    return uint64_t(lo) | (uint64_t(hi) << 32);
}
__device__ __forceinline__ GatherAgg ga_shfl_up(const GatherAgg& v, int d) {
    return GatherAgg{ga_shfl_up(v.bytes, d), ga_shfl_up(v.bad, d), ga_shfl_up(v.first_bad, d)};
}
// The sum of the block's elements before this thread's; *total = the block.
__device__ __forceinline__ GatherAgg ga_block_excl(const GatherAgg& v, GatherAgg* s_wave, GatherAgg* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GatherAgg incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const GatherAgg o = ga_shfl_up(incl, d);
        if (lane >= d) incl = gather_join(o, incl);
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    GatherAgg base = gather_none(), sum = gather_none();
#pragma unroll
    for (int w = 0; w < kGaThreads / 64; ++w) {
        const GatherAgg t = s_wave[w];
        if (w < wave) base = gather_join(base, t);
        sum = gather_join(sum, t);
    }
    *total = sum;
    __syncthreads();   // s_wave is reused by the caller's next round
    GatherAgg prev = ga_shfl_up(incl, 1);
    if (lane == 0) prev = gather_none();
    return gather_join(base, prev);
}

// Piece i (< npieces): one 16-byte load (onc_frag_piece: off, len, src).
struct GaPiece {
    uint64_t off;
    uint32_t len, src;
};
__device__ __forceinline__ GaPiece ga_piece(const GatherArgs& a, uint64_t i) {
    const uint4 q = *reinterpret_cast<const uint4*>(a.pieces + i);
    return GaPiece{uint64_t(q.x) | (uint64_t(q.y) << 32), q.z, q.w};
}
__device__ __forceinline__ bool ga_ok(const GatherArgs& a, const GaPiece& p) {
    return gather_ok(p.off, p.len, p.src, a.len0, a.len1, a.len2);
}
__device__ __forceinline__ GatherAgg ga_elem(const GatherArgs& a, uint64_t i) {
    if (i >= a.npieces) return gather_none();
    const GaPiece p = ga_piece(a, i);
    return gather_elem(i, p.len, ga_ok(a, p));
}

__global__ __launch_bounds__(kGaThreads) void gath_blk_kernel(GatherArgs a) {
    __shared__ GatherAgg s_wave[kGaThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kGaThreads + threadIdx.x;
    GatherAgg total;
    ga_block_excl(ga_elem(a, i), s_wave, &total);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// blk[b] := the sum of the blocks before b; blk[nblk] := the whole list.
__global__ __launch_bounds__(kGaThreads) void gath_blkscan_kernel(GatherArgs a, uint64_t nblk) {
    __shared__ GatherAgg s_wave[kGaThreads / 64];
    GatherAgg carry = gather_none();
    for (uint64_t b0 = 0; b0 < nblk; b0 += kGaThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const GatherAgg v = b < nblk ? a.blk[b] : gather_none();
        GatherAgg total;
        const GatherAgg ex = ga_block_excl(v, s_wave, &total);
        if (b < nblk) a.blk[b] = gather_join(carry, ex);
        carry = gather_join(carry, total);
    }
    if (threadIdx.x == 0) a.blk[nblk] = carry;
}

__global__ __launch_bounds__(kGaThreads) void gath_apply_kernel(GatherArgs a) {
    __shared__ GatherAgg s_wave[kGaThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kGaThreads + threadIdx.x;
    GatherAgg total;
    const GatherAgg ex = gather_join(a.blk[blockIdx.x], ga_block_excl(ga_elem(a, i), s_wave, &total));
    if (i >= a.npieces) return;
    a.piece_pos[i] = ex.bytes;      // a bad piece keeps its place in the stream
    if (i == a.npieces - 1) {
        const GatherAgg all = a.blk[(a.npieces + kGaThreads - 1) / kGaThreads];
        a.piece_pos[a.npieces] = all.bytes;
        a.result[0] = all.bytes;
        a.result[1] = all.bad;
        a.result[2] = all.first_bad < a.npieces ? all.first_bad : a.npieces;
    }
}

// A list of no pieces (a kernel and not a memset: every step of the call is a
// kernel launch, so a captured call is a chain of kernel nodes).
__global__ void gath_empty_kernel(GatherArgs a) {
    a.piece_pos[0] = 0;
    a.result[0] = 0;
    a.result[1] = 0;
    a.result[2] = 0;
}

// Where a piece's bytes are and how many of them may be read: 0 for a bad
// piece (never read; its bytes of `out` stay as they were) and for an empty
// one.
struct GaSrc {
    uint64_t addr;
    uint32_t vlen;
};
__device__ __forceinline__ GaSrc ga_src(const GatherArgs& a, const GaPiece& p) {
    if (p.len == 0 || !ga_ok(a, p)) return GaSrc{0, 0};
    const uint8_t* base = p.src == 0 ? a.base0 : p.src == 1 ? a.base1 : a.base2;
    return GaSrc{uint64_t(reinterpret_cast<uintptr_t>(base)) + p.off, p.len};
}

// The pieces reaching into a tile: pos(0 .. n) their stream positions,
// pos(0) <= the tile's first byte and pos(n) >= its end; src(0 .. n - 1).
struct GaStaged {          // in LDS
    const uint64_t* e;
    const uint64_t* s;
    const uint32_t* v;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return e[j]; }
    __device__ __forceinline__ GaSrc src(uint64_t j) const { return GaSrc{s[j], v[j]}; }
};
struct GaGlobal {          // more than kGaStage of them: from piece j0 on in global memory
    const GatherArgs& a;
    uint64_t j0;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return a.piece_pos[j0 + j]; }
    __device__ __forceinline__ GaSrc src(uint64_t j) const { return ga_src(a, ga_piece(a, j0 + j)); }
};

// Last j in [0, n) with e[j] <= x (e[0] <= x).
__device__ __forceinline__ uint64_t ga_last_at_or_before(const uint64_t* e, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
template <class View>
__device__ __forceinline__ uint64_t ga_last_at_or_before(const View& v, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (v.pos(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The chunks of tile [t0, t0 + kGaTile) within [D0, D1) (coordinates: bytes
// from the 16-byte aligned address at or below the caller's out; byte D of
// them is stream position D + shift). Among pieces starting at the same
// position only the last has bytes, so the last piece starting at or before a
// byte is the one whose non-empty extent covers it. `spare`: an address that
// may always be read (piece_pos).
template <class View>
__device__ __forceinline__ void ga_copy_tile(const View& v, uint64_t n, uint64_t shift, uint64_t spare,
                                             uint8_t* __restrict__ out, uint64_t t0, uint64_t D0, uint64_t D1, int lane) {
#pragma unroll 2
    for (uint64_t cb = t0 + 16ull * lane; cb < t0 + kGaTile; cb += 1024) {
        if (cb + 16 <= D0 || cb >= D1) continue;
        const uint64_t b0 = max(cb, D0), b1 = min(cb + 16, D1);
        uint64_t j = ga_last_at_or_before(v, n, b0 + shift);
        GaSrc s = v.src(j);
        const uint64_t o0 = b0 + shift - v.pos(j);
        if (b1 - b0 == 16 && o0 < s.vlen && s.vlen - o0 >= 16) {
            uint32_t w[4];
            load16_unaligned(uintptr_t(s.addr + o0), w);
            *reinterpret_cast<uint4*>(out + cb) = make_uint4(w[0], w[1], w[2], w[3]);
            continue;
        }
        // a seam between pieces, a bad piece or an end of the window: byte by
        // byte, but every byte's load issued before the first is waited for.
        // (One round trip per byte, as defrag_copy resolves its seams, made
        // this kernel 2.4x..2.7x slower than frag_copy on onc_fragment_iov's
        // lists, which have three seams per fragment.) A byte that is not
        // written loads from `spare` instead of branching around its load: a
        // load under a condition is waited for where it stands.
        // The walk counts in chunk bytes (32 bits): piece j holds chunk bytes
        // [i_at, i_nxt), of which `room` from i_at on may be read, at a_at.
        const uint32_t i0 = uint32_t(b0 - cb), i1 = uint32_t(b1 - cb);
        const uint64_t P0 = b0 + shift;                       // the stream position of chunk byte i0
        auto rel = [&](uint64_t pos) { return i0 + uint32_t(min(pos - P0, uint64_t(16))); };   // pos >= P0
        uint32_t i_at = i0, i_nxt = rel(v.pos(j + 1));
        uint32_t room = o0 < s.vlen ? uint32_t(s.vlen - o0) : 0u;
        uint64_t a_at = s.addr + o0;
        uint32_t got[16];
        uint32_t mask = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const bool in = i >= i0 && i < i1;
            if (in && i >= i_nxt) {                           // the next piece with bytes starts at this byte
                do i_nxt = rel(v.pos(++j + 1)); while (i >= i_nxt);
                s = v.src(j);
                i_at = i;
                room = s.vlen;
                a_at = s.addr;
            }
            const uint32_t k = i - i_at;
            const bool ok = in && k < room;
            mask |= ok ? 1u << i : 0u;
            got[i] = gload<uint8_t>(uintptr_t(ok ? a_at + k : spare));
        }
        if (mask == 0xFFFFu) {
            uint32_t w[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                w[q] = got[4 * q] | (got[4 * q + 1] << 8) | (got[4 * q + 2] << 16) | (got[4 * q + 3] << 24);
            *reinterpret_cast<uint4*>(out + cb) = make_uint4(w[0], w[1], w[2], w[3]);
            continue;
        }
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i)
            if (mask >> i & 1) out[cb + i] = uint8_t(got[i]);
    }
}

// The tiling, the run of tiles per wave and the staged window are
// defrag_copy's (defrag.hip), over piece_pos instead of E: piece_pos is
// sorted, so how many window entries lie at or before a byte is a ballot
// count. A run of equal positions (pieces of no bytes) longer than the window
// is stepped over like a tile that starts beyond it; one inside a tile sends
// the tile to global memory like any other tile of more than kGaStage pieces.
__global__ __launch_bounds__(kGaThreads) void gather_copy_kernel(GatherArgs a) {
    __shared__ uint64_t s_e[kGaThreads / 64][kGaStage + 1];
    __shared__ uint64_t s_s[kGaThreads / 64][kGaStage];
    __shared__ uint32_t s_v[kGaThreads / 64][kGaStage];
    static_assert(kGaStage == 128, "the window is staged and counted as two rounds of 64 lanes + 1");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t N = a.npieces;
    const uint64_t* E = a.piece_pos;
    const uint64_t W = gather_window(a.from, a.count, E[N]);   // stream bytes [from, from + W) exist
    if (W == 0) return;
    const uint64_t D0 = a.origin, D1 = a.origin + W;
    const uint64_t shift = a.from - a.origin;                  // (mod 2^64: D >= origin wherever it is added)
    const uint64_t ntiles = (D1 + kGaTile - 1) / kGaTile;
    const uint64_t nw = uint64_t(gridDim.x) * (kGaThreads / 64);
    const uint64_t per = (ntiles + nw - 1) / nw;
    const uint64_t T0 = (uint64_t(blockIdx.x) * (kGaThreads / 64) + wv) * per;   // wave-uniform
    const uint64_t T1 = min(T0 + per, ntiles);
    if (T0 >= T1) return;
    uint64_t* se = s_e[wv];
    const uint64_t spare = uint64_t(reinterpret_cast<uintptr_t>(E));
    // E[0] = 0 <= lo and E[N] >= from + W: every search ends below N.
    // ja: a piece with E[ja] <= the tile's first byte (kept across tiles)
    uint64_t ja = ga_last_at_or_before(E, N + 1, max(T0 * kGaTile, D0) + shift);
    for (uint64_t T = T0; T < T1; ++T) {
        const uint64_t t0 = T * kGaTile;
        const uint64_t lo = max(t0, D0) + shift, hi = min(t0 + kGaTile, D1) + shift;   // stream positions
        uint32_t k, c_hi;
        for (;;) {
            __builtin_amdgcn_wave_barrier();   // the tile before may still read the stage
            // (past the array the window repeats E[N] >= hi: never counted)
            const uint64_t e0 = E[min(ja + lane, N)], e1 = E[min(ja + 64 + lane, N)];
            const uint64_t e2 = E[min(ja + kGaStage, N)];
            se[lane] = e0;
            se[64 + lane] = e1;
            if (lane == 0) se[kGaStage] = e2;
            const uint32_t c_lo = __popcll(__ballot(e0 <= lo)) + __popcll(__ballot(e1 <= lo)) + (e2 <= lo ? 1u : 0u);
            c_hi = __popcll(__ballot(e0 < hi)) + __popcll(__ballot(e1 < hi)) + (e2 < hi ? 1u : 0u);
            if (c_lo == kGaStage + 1) {        // the tile starts beyond the window: search on from its end
                ja += kGaStage;
                ja += ga_last_at_or_before(E + ja, N + 1 - ja, lo);
                continue;
            }
            k = c_lo - 1;                      // window entry of the piece holding the tile's first byte
            if (c_hi == kGaStage + 1 && k != 0) {   // the window ends inside the tile: start it at that piece
                ja += k;
                continue;
            }
            break;
        }
        if (c_hi == kGaStage + 1) {
            // more than kGaStage pieces reach into the tile: in global memory
            const uint64_t jb = ja + kGaStage + ga_last_at_or_before(E + ja + kGaStage, N + 1 - ja - kGaStage, hi - 1);
            ga_copy_tile(GaGlobal{a, ja}, jb - ja + 1, shift, spare, a.out, t0, D0, D1, lane);
            ja = jb;
            continue;
        }
        const uint32_t n = c_hi - k;           // window entries k .. c_hi - 1 reach into the tile
        for (uint32_t i = lane; i < n; i += 64) {
            const GaSrc s = ga_src(a, ga_piece(a, ja + k + i));
            s_s[wv][i] = s.addr;
            s_v[wv][i] = s.vlen;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        ga_copy_tile(GaStaged{se + k, s_s[wv], s_v[wv]}, n, shift, spare, a.out, t0, D0, D1, lane);
        ja += c_hi - 1;                        // the piece holding the tile's last byte holds the next one's first or comes before it
    }
}

static uint32_t ga_blocks(uint64_t n) { return uint32_t((n + kGaThreads - 1) / kGaThreads); }

hipError_t launch_gath_blk(const GatherArgs& a, hipStream_t s) {
    ONC_LAUNCH(gath_blk_kernel, dim3(ga_blocks(a.npieces)), dim3(kGaThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gath_blkscan(const GatherArgs& a, hipStream_t s) {
    ONC_LAUNCH(gath_blkscan_kernel, dim3(1), dim3(kGaThreads), 0, s, a, uint64_t(ga_blocks(a.npieces)));
    return hipGetLastError();
}

hipError_t launch_gath_apply(const GatherArgs& a, hipStream_t s) {
    ONC_LAUNCH(gath_apply_kernel, dim3(ga_blocks(a.npieces)), dim3(kGaThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gath_empty(const GatherArgs& a, hipStream_t s) {
    ONC_LAUNCH(gath_empty_kernel, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

// The grid covers the window asked for (what of it exists is known on the
// device only), up to kGaMaxBlocks workgroups; the kernel deals the tiles out.
hipError_t launch_gather_copy(const GatherArgs& a, hipStream_t s, uint32_t variant) {
    const uint64_t per_wg = kGaTile * (kGaThreads / 64);
    const uint64_t cap = a.count > ~0ull - 16 - per_wg ? ~0ull - 16 - per_wg : a.count;
    const uint64_t wgs = (a.origin + cap + per_wg - 1) / per_wg;
    const uint64_t most = copy_max_groups(variant, kGaMaxBlocks);
    ONC_LAUNCH(gather_copy_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kGaThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
