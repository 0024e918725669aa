// fragment_iov.hip — the vectored encode's records cut into fragments without
// a byte copied (onc_fragment_iov, include/onc_rpc.h): fragment.hip for
// onc_encode_iov's list. Only the entries of `iov` are read; what is written
// is 4 bytes per fragment (its mark) and a list of 16-byte pieces naming the
// slices of the marks, the header buffer and the payload arena that make up
// the stream. fragment.hip's shape, one sum wider:
//
//   fragiov_blk      per 256 records: the block's {stream bytes, fragments,
//                    multi-fragment records, pieces} (fragment_iov_plan.h
//                    FivAgg, 64 bits)
//   fragiov_blkscan  one workgroup: exclusive scan of the block sums
//   fragiov_apply    per record: out_off, piece_off, status (both capacities),
//                    the pieces and fragments before the record for the fill
//                    (P, NF); the last record: the arrays' last entries and
//                    result
//   fragiov_fill     the hot path, partitioned by *output pieces*: a wave per
//                    tile of kFvTile pieces, each wave a run of consecutive
//                    tiles (tile_walk.h walk_tiles, as frag_copy, with the
//                    run's first tile searched for by the wave together). A
//                    lane writes whole pieces (one
//                    16-byte store; a wave's 64 stores are 1 KiB in a row) and,
//                    for a MARK piece, the mark itself (consecutive fragments:
//                    consecutive words). What is staged in LDS is the window
//                    of P over the records reaching into the tile; inside a
//                    record piece t is fragment and part by closed form
//                    (fragment_iov_plan.h fiv_at): no per-fragment table, no
//                    search among fragments.
#include "common.h"
#include "fragment_iov_plan.h"
#include "kernels.h"
#include "tile_walk.h"

namespace onc {

constexpr int kFvThreads = kCopyThreads;
constexpr uint64_t kFvTile = 512;       // pieces per wave and step (8 KiB of the piece array)
constexpr uint32_t kFvMaxBlocks = kCopyMaxBlocks;   // fragiov_fill workgroups

struct FivSum {      // the block scan's aggregate
    using Agg = FivAgg;
    static __device__ __forceinline__ Agg none() { return fiv_none(); }
    static __device__ __forceinline__ Agg join(const Agg& a, const Agg& b) { return fiv_join(a, b); }
};

// The two lengths of entry i (< n) and its limit. Nothing else is read by the
// plan, and nothing through the entry's offsets by any kernel.
__device__ __forceinline__ uint2 fv_lens(const FragmentIovArgs& a, uint64_t i) {
    return *reinterpret_cast<const uint2*>(&a.iov[i].hdr_len);
}
__device__ __forceinline__ uint32_t fv_limit(const FragmentIovArgs& a, uint64_t i) {
    return a.rec_max_frag ? a.rec_max_frag[i] : a.max_frag;
}
__device__ __forceinline__ FivRec fv_rec(const FragmentIovArgs& a, uint64_t i) {
    const uint2 l = fv_lens(a, i);
    return fiv_rec(l.x, l.y, fv_limit(a, i));
}

__global__ __launch_bounds__(kFvThreads) void fragiov_blk_kernel(FragmentIovArgs a) {
    __shared__ FivAgg s_wave[kFvThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kFvThreads + threadIdx.x;
    const FivAgg v = i < a.n ? fiv_elem(fv_rec(a, i)) : fiv_none();
    block_total<FivSum>(v, s_wave, a.blk);
}

// blk[b] := the sum of the blocks before b; blk[nblk] := the whole batch.
__global__ __launch_bounds__(kFvThreads) void fragiov_blkscan_kernel(FragmentIovArgs a, uint64_t nblk) {
    __shared__ FivAgg s_wave[kFvThreads / 64];
    scan_blocks<FivSum>(a.blk, nblk, s_wave, [&] {
        a.info[0] = ~0ull;      // the first record that does not fit starts at this piece (fragiov_apply)
    });
}

__global__ __launch_bounds__(kFvThreads) void fragiov_apply_kernel(FragmentIovArgs a) {
    __shared__ FivAgg s_wave[kFvThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kFvThreads + threadIdx.x;
    FivRec r{0, 0, 0, ONC_OK};
    if (i < a.n) r = fv_rec(a, i);
    FivAgg total;
    const FivAgg ex = fiv_join(a.blk[blockIdx.x], block_excl<FivSum>(fiv_elem(r), s_wave, &total));
    if (i >= a.n) return;
    a.out_off[i] = ex.bytes;
    a.piece_off[i] = ex.pieces;
    a.P[i] = ex.pieces;
    a.NF[i] = ex.frags;
    const int32_t st = fiv_status(r, ex.pieces, a.max_pieces, ex.frags, a.marks_cap);
    // both placements only grow and every record that can fail here takes a
    // piece and a mark: once a record has failed, every later one starts
    // beyond the capacity it failed on. The one failing record that still
    // starts within both is the first, and nothing from it on is written
    if (st == ONC_ENC_WRITE_ZERO && ex.pieces <= a.max_pieces && ex.frags <= a.marks_cap / 4) a.info[0] = ex.pieces;
    a.status[i] = st;
    if (i == a.n - 1) {
        const FivAgg all = a.blk[(a.n + kFvThreads - 1) / kFvThreads];
        a.out_off[a.n] = all.bytes;
        a.piece_off[a.n] = all.pieces;
        a.P[a.n] = all.pieces;
        a.NF[a.n] = all.frags;
        a.result[0] = all.frags;
        a.result[1] = all.bytes;
        a.result[2] = all.multi;
        a.result[3] = all.pieces;
    }
}

// The pieces [t0, hi) of one tile. e[0..n]: the first pieces of the records
// reaching into the tile, e[0] <= t0, e[n] >= hi; e[0] is record `first`'s. A
// record that takes no pieces starts where the next one does, so the last
// record starting at or before a piece holds it — and that one is a record
// with at least a mark, every capacity test passed (the tile ends before the
// first record that failed one).
__device__ __forceinline__ void fv_fill_tile(const uint64_t* e, uint64_t n, uint64_t first, const FragmentIovArgs& a,
                                             uint64_t t0, uint64_t hi, int lane) {
    // what is read never overlaps what is written: the loads of the steps
    // unrolled together are issued ahead of their stores
    const uint64_t* __restrict__ iov = reinterpret_cast<const uint64_t*>(a.iov);   // 4 words per entry
    const uint64_t* __restrict__ NF = a.NF;
    const uint32_t* __restrict__ lim = a.rec_max_frag;
    uint8_t* __restrict__ marks = a.marks;
    onc_frag_piece* __restrict__ pieces = a.pieces;
#pragma unroll 4
    for (uint64_t p = t0 + lane; p < hi; p += 64) {
        const uint64_t j = last_at_or_before(e, n, p);
        const uint64_t i = first + j;
        const uint64_t t = p - e[j];
        const uint64_t hdr_off = iov[4 * i], payload_off = iov[4 * i + 1], lens = iov[4 * i + 3], nf = NF[i];
        const uint32_t F = lim ? lim[i] : a.max_frag;
        const FivShape sh = fiv_shape(uint32_t(lens), uint32_t(lens >> 32), F);
        const FivAt at = fiv_at(sh, t);
        FivPiece pc = fiv_piece(sh, F, at);
        pc.off += pc.src == ONC_PIECE_MARK ? 4 * nf : pc.src == ONC_PIECE_HDR ? hdr_off : payload_off;
        if (pc.src == ONC_PIECE_MARK)
            *reinterpret_cast<uint32_t*>(marks + pc.off) = __builtin_bswap32(frag_mark(sh.B, at.j, F));
        uint4 v;
        v.x = uint32_t(pc.off);
        v.y = uint32_t(pc.off >> 32);
        v.z = pc.len;
        v.w = pc.src;
        *reinterpret_cast<uint4*>(pieces + p) = v;
    }
}

// The walk is walk_tiles' (tile_walk.h) over the piece prefix P instead of a
// byte prefix, with no origin: tile T is pieces [T kFvTile, (T + 1) kFvTile),
// P[0] = 0 and P[n] >= W. A run's first tile is searched for by the wave
// together. Nothing but the window is staged.
__global__ __launch_bounds__(kFvThreads) void fragiov_fill_kernel(FragmentIovArgs a) {
    __shared__ uint64_t s_e[kFvThreads / 64][kCopyStage + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t W = min(a.info[0], a.P[a.n]);   // OK records fill pieces [0, W), W <= max_pieces
    if (W == 0) return;
    walk_tiles<kFvTile>(
        SortedArrayByWave{a.P, lane}, a.n, 0, W, 0, s_e[wv],
        [&](const uint64_t* e, uint64_t j0, uint32_t n, uint64_t, uint64_t lo, uint64_t hi) {
            wave_stage_done();
            fv_fill_tile(e, n, j0, a, lo, hi, lane);
        },
        [&](uint64_t j0, uint64_t n, uint64_t, uint64_t lo, uint64_t hi) {
            fv_fill_tile(a.P + j0, n, j0, a, lo, hi, lane);
        });
}

static uint32_t fv_blocks(uint64_t n) { return uint32_t((n + kFvThreads - 1) / kFvThreads); }

hipError_t launch_fragiov_blk(const FragmentIovArgs& a, hipStream_t s) {
    ONC_LAUNCH(fragiov_blk_kernel, dim3(fv_blocks(a.n)), dim3(kFvThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fragiov_blkscan(const FragmentIovArgs& a, hipStream_t s) {
    ONC_LAUNCH(fragiov_blkscan_kernel, dim3(1), dim3(kFvThreads), 0, s, a, uint64_t(fv_blocks(a.n)));
    return hipGetLastError();
}

hipError_t launch_fragiov_apply(const FragmentIovArgs& a, hipStream_t s) {
    ONC_LAUNCH(fragiov_apply_kernel, dim3(fv_blocks(a.n)), dim3(kFvThreads), 0, s, a);
    return hipGetLastError();
}

// The grid covers the piece capacity (what is written is known on the device
// only), up to kFvMaxBlocks workgroups; the kernel deals the tiles out.
hipError_t launch_fragiov_fill(const FragmentIovArgs& a, hipStream_t s, uint32_t variant) {
    const uint64_t wgs = copy_groups(0, a.max_pieces, kFvTile * (kFvThreads / 64));
    const uint64_t most = copy_max_groups(variant, kFvMaxBlocks);
    ONC_LAUNCH(fragiov_fill_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kFvThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
