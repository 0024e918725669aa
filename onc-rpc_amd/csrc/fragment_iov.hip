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
//                    tiles, as frag_copy. A lane writes whole pieces (one
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

namespace onc {

constexpr int kFvThreads = 256;
constexpr uint64_t kFvTile = 512;       // pieces per wave and step (8 KiB of the piece array)
constexpr uint32_t kFvStage = 128;      // records of a tile kept in LDS (more: searched in global memory)
constexpr uint32_t kFvMaxBlocks = 2048; // fragiov_fill workgroups (the tiles are dealt out among their waves)

__device__ __forceinline__ uint64_t fv_shfl_up(uint64_t v, int d) {
    const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), d, 64));
    const uint32_t hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), d, 64));
    return uint64_t(lo) | (uint64_t(hi) << 32);
}
__device__ __forceinline__ FivAgg fv_shfl_up(const FivAgg& v, int d) {
    return FivAgg{fv_shfl_up(v.bytes, d), fv_shfl_up(v.frags, d), fv_shfl_up(v.multi, d), fv_shfl_up(v.pieces, d)};
}
// The sum of the block's elements before this thread's; *total = the block.
__device__ __forceinline__ FivAgg fv_block_excl(const FivAgg& v, FivAgg* s_wave, FivAgg* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    FivAgg incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const FivAgg o = fv_shfl_up(incl, d);
        if (lane >= d) incl = fiv_join(o, incl);
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    FivAgg base = fiv_none(), sum = fiv_none();
#pragma unroll
    for (int w = 0; w < kFvThreads / 64; ++w) {
        const FivAgg t = s_wave[w];
        if (w < wave) base = fiv_join(base, t);
        sum = fiv_join(sum, t);
    }
    *total = sum;
    __syncthreads();   // s_wave is reused by the caller's next round
    FivAgg prev = fv_shfl_up(incl, 1);
    if (lane == 0) prev = fiv_none();
    return fiv_join(base, prev);
}

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
    FivAgg total;
    fv_block_excl(v, s_wave, &total);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// blk[b] := the sum of the blocks before b; blk[nblk] := the whole batch.
__global__ __launch_bounds__(kFvThreads) void fragiov_blkscan_kernel(FragmentIovArgs a, uint64_t nblk) {
    __shared__ FivAgg s_wave[kFvThreads / 64];
    FivAgg carry = fiv_none();
    for (uint64_t b0 = 0; b0 < nblk; b0 += kFvThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const FivAgg v = b < nblk ? a.blk[b] : fiv_none();
        FivAgg total;
        const FivAgg ex = fv_block_excl(v, s_wave, &total);
        if (b < nblk) a.blk[b] = fiv_join(carry, ex);
        carry = fiv_join(carry, total);
    }
    if (threadIdx.x == 0) {
        a.blk[nblk] = carry;
        a.info[0] = ~0ull;      // the first record that does not fit starts at this piece (fragiov_apply)
    }
}

__global__ __launch_bounds__(kFvThreads) void fragiov_apply_kernel(FragmentIovArgs a) {
    __shared__ FivAgg s_wave[kFvThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kFvThreads + threadIdx.x;
    FivRec r{0, 0, 0, ONC_OK};
    if (i < a.n) r = fv_rec(a, i);
    FivAgg total;
    const FivAgg ex = fiv_join(a.blk[blockIdx.x], fv_block_excl(fiv_elem(r), s_wave, &total));
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

// Last j in [0, n) with e[j] <= x (e[0] <= x).
__device__ __forceinline__ uint64_t fv_last_at_or_before(const uint64_t* e, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The same for one x per wave (every lane calls it with the same arguments):
// the lanes probe 64 evenly spaced entries per round, so a million entries
// take 4 dependent loads instead of 20. e is sorted: the probes at or before
// x are the lowest lanes', and lane 0's (e[lo] <= x) is always one of them.
__device__ __forceinline__ uint64_t fv_wave_last_at_or_before(const uint64_t* e, uint64_t n, uint64_t x, int lane) {
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
        const uint64_t j = fv_last_at_or_before(e, n, p);
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

// The tiling, the run of tiles per wave and the staged window are frag_copy's
// (fragment.hip), over the piece prefix instead of the byte prefix: P is
// sorted, so how many window entries lie at or before a piece is a ballot
// count.
__global__ __launch_bounds__(kFvThreads) void fragiov_fill_kernel(FragmentIovArgs a) {
    __shared__ uint64_t s_e[kFvThreads / 64][kFvStage + 1];
    static_assert(kFvStage == 128, "the window is staged and counted as two rounds of 64 lanes + 1");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t W = min(a.info[0], a.P[a.n]);   // OK records fill pieces [0, W), W <= max_pieces
    if (W == 0) return;
    const uint64_t ntiles = (W + kFvTile - 1) / kFvTile;
    const uint64_t nw = uint64_t(gridDim.x) * (kFvThreads / 64);
    const uint64_t per = (ntiles + nw - 1) / nw;
    const uint64_t T0 = (uint64_t(blockIdx.x) * (kFvThreads / 64) + wv) * per;   // wave-uniform
    const uint64_t T1 = min(T0 + per, ntiles);
    if (T0 >= T1) return;
    uint64_t* se = s_e[wv];
    // P[0] = 0 <= lo and P[n] >= W: every search ends below n.
    // ja: a record with P[ja] <= the tile's first piece (kept across tiles)
    uint64_t ja = fv_wave_last_at_or_before(a.P, a.n + 1, T0 * kFvTile, lane);
    for (uint64_t T = T0; T < T1; ++T) {
        const uint64_t lo = T * kFvTile, hi = min(lo + kFvTile, W);
        uint32_t k, c_hi;
        for (;;) {
            __builtin_amdgcn_wave_barrier();   // the tile before may still read the stage
            // (past the array the window repeats P[n] >= W: never counted)
            const uint64_t e0 = a.P[min(ja + lane, a.n)], e1 = a.P[min(ja + 64 + lane, a.n)];
            const uint64_t e2 = a.P[min(ja + kFvStage, a.n)];
            se[lane] = e0;
            se[64 + lane] = e1;
            if (lane == 0) se[kFvStage] = e2;
            const uint32_t c_lo = __popcll(__ballot(e0 <= lo)) + __popcll(__ballot(e1 <= lo)) + (e2 <= lo ? 1u : 0u);
            c_hi = __popcll(__ballot(e0 < hi)) + __popcll(__ballot(e1 < hi)) + (e2 < hi ? 1u : 0u);
            if (c_lo == kFvStage + 1) {        // the tile starts beyond the window: search on from its end
                ja += kFvStage;
                ja += fv_wave_last_at_or_before(a.P + ja, a.n + 1 - ja, lo, lane);
                continue;
            }
            k = c_lo - 1;                      // window entry of the record holding the tile's first piece
            if (c_hi == kFvStage + 1 && k != 0) {   // the window ends inside the tile: start it at that record
                ja += k;
                continue;
            }
            break;
        }
        if (c_hi == kFvStage + 1) {
            // more than kFvStage records reach into the tile: in global memory
            const uint64_t jb = ja + kFvStage + fv_wave_last_at_or_before(a.P + ja + kFvStage, a.n + 1 - ja - kFvStage, hi - 1, lane);
            fv_fill_tile(a.P + ja, jb - ja + 1, ja, a, lo, hi, lane);
            ja = jb;
            continue;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        fv_fill_tile(se + k, c_hi - k, ja + k, a, lo, hi, lane);   // window entries k .. c_hi - 1 reach into the tile
        ja += c_hi - 1;                        // the record holding the tile's last piece holds the next one's first or comes before it
    }
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
    const uint64_t per_wg = kFvTile * (kFvThreads / 64);
    const uint64_t cap = a.max_pieces > ~0ull - per_wg ? ~0ull - per_wg : a.max_pieces;
    const uint64_t wgs = (cap + per_wg - 1) / per_wg;
    const uint64_t most = copy_max_groups(variant, kFvMaxBlocks);
    ONC_LAUNCH(fragiov_fill_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kFvThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
