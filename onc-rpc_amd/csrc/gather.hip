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
//                 store is aligned), each wave a run of consecutive tiles
//                 (tile_walk.h walk_tiles); the
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
#include "tile_walk.h"

namespace onc {

constexpr int kGaThreads = kCopyThreads;
constexpr uint64_t kGaTile = 8192;      // output bytes per wave and step
constexpr uint32_t kGaMaxBlocks = kCopyMaxBlocks;   // gather_copy workgroups

struct GatherSum {   // the block scan's aggregate
    using Agg = GatherAgg;
    static __device__ __forceinline__ Agg none() { return gather_none(); }
    static __device__ __forceinline__ Agg join(const Agg& a, const Agg& b) { return gather_join(a, b); }
};

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
    block_total<GatherSum>(ga_elem(a, i), s_wave, a.blk);
}

// blk[b] := the sum of the blocks before b; blk[nblk] := the whole list.
__global__ __launch_bounds__(kGaThreads) void gath_blkscan_kernel(GatherArgs a, uint64_t nblk) {
    __shared__ GatherAgg s_wave[kGaThreads / 64];
    scan_blocks<GatherSum>(a.blk, nblk, s_wave, [] {});
}

__global__ __launch_bounds__(kGaThreads) void gath_apply_kernel(GatherArgs a) {
    __shared__ GatherAgg s_wave[kGaThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kGaThreads + threadIdx.x;
    GatherAgg total;
    const GatherAgg ex = gather_join(a.blk[blockIdx.x], block_excl<GatherSum>(ga_elem(a, i), s_wave, &total));
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
struct GaGlobal {          // more than kCopyStage of them: from piece j0 on in global memory
    const GatherArgs& a;
    uint64_t j0;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return a.piece_pos[j0 + j]; }
    __device__ __forceinline__ GaSrc src(uint64_t j) const { return ga_src(a, ga_piece(a, j0 + j)); }
};

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
        uint64_t j = last_at_or_before(v, n, b0 + shift);
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

// The walk is walk_tiles' (tile_walk.h) over piece_pos: E[0] = 0 and E[N] >=
// from + W. A run of equal positions (pieces of no bytes) longer than the
// window is stepped over like a tile that starts beyond it; one inside a tile
// sends the tile to global memory like any other tile of more than kCopyStage
// pieces. Staged per piece of a tile: its source address and readable bytes.
__global__ __launch_bounds__(kGaThreads) void gather_copy_kernel(GatherArgs a) {
    __shared__ uint64_t s_e[kGaThreads / 64][kCopyStage + 1];
    __shared__ uint64_t s_s[kGaThreads / 64][kCopyStage];
    __shared__ uint32_t s_v[kGaThreads / 64][kCopyStage];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t N = a.npieces;
    const uint64_t* E = a.piece_pos;
    const uint64_t W = gather_window(a.from, a.count, E[N]);   // stream bytes [from, from + W) exist
    if (W == 0) return;
    const uint64_t D0 = a.origin, D1 = a.origin + W;
    const uint64_t shift = a.from - a.origin;                  // (mod 2^64: D >= origin wherever it is added)
    const uint64_t spare = uint64_t(reinterpret_cast<uintptr_t>(E));
    walk_tiles<kGaTile>(
        SortedArray{E}, N, D0, D1, shift, s_e[wv],
        [&](const uint64_t* e, uint64_t j0, uint32_t n, uint64_t t0, uint64_t, uint64_t) {
            for (uint32_t i = lane; i < n; i += 64) {
                const GaSrc s = ga_src(a, ga_piece(a, j0 + i));
                s_s[wv][i] = s.addr;
                s_v[wv][i] = s.vlen;
            }
            wave_stage_done();
            ga_copy_tile(GaStaged{e, s_s[wv], s_v[wv]}, n, shift, spare, a.out, t0, D0, D1, lane);
        },
        [&](uint64_t j0, uint64_t n, uint64_t t0, uint64_t, uint64_t) {
            ga_copy_tile(GaGlobal{a, j0}, n, shift, spare, a.out, t0, D0, D1, lane);
        });
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
    const uint64_t wgs = copy_groups(a.origin, a.count, kGaTile * (kGaThreads / 64));
    const uint64_t most = copy_max_groups(variant, kGaMaxBlocks);
    ONC_LAUNCH(gather_copy_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kGaThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
