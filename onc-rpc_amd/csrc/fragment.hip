// fragment.hip — records cut into fragments on the send side (onc_fragment,
// include/onc_rpc.h; RFC 5531 §11), the inverse of defrag.hip.
//
// The reference writes every record as one fragment (serialise_into,
// rpc_message.rs:146-156) and refuses a body of 2^31 bytes or more. A sender
// that flushes through a bounded buffer, or whose peer caps the fragment
// size, needs the same bytes under several marks: every max_frag body bytes a
// mark, the last one with bit 31. Lengths, then scan, then emit, as the
// encoder and the reassembly:
//
//   fragp_blk      per 256 records: the block's {output bytes, fragments,
//                  multi-fragment records} (fragment_plan.h FragAgg, 64 bits)
//   fragp_blkscan  one workgroup: exclusive scan of the block sums
//   fragp_apply    per record: out_off, status (capacity), the record's
//                  output start for the copy (E); the last record: out_off[n]
//                  and result
//   frag_copy      the hot path: a wave per 8 KiB tile of *output*, each wave
//                  a run of consecutive tiles (tile_walk.h walk_tiles, as
//                  defrag_copy). What is staged
//                  in LDS is the *records* reaching into the tile (output
//                  start and wire extent); inside a record the fragment of a
//                  byte is q / (max_frag + 4), its place in it the remainder
//                  (fragment_plan.h frag_at): no per-fragment table, no
//                  search among fragments. A 16-byte output chunk inside one
//                  fragment's body is one unaligned 16-byte load and one
//                  aligned 16-byte store; a chunk with one mark in it is one
//                  load too, the mark put in by shifts (the wire bytes on
//                  both sides of it are neighbours); chunks with several
//                  marks, records shorter than a chunk and the two ends of
//                  the batch go byte by byte.
#include "common.h"
#include "fragment_plan.h"
#include "kernels.h"
#include "tile_walk.h"

namespace onc {

constexpr int kFgThreads = kCopyThreads;
constexpr uint64_t kFgTile = 8192;      // output bytes per wave and step
constexpr uint32_t kFgMaxBlocks = kCopyMaxBlocks;   // frag_copy workgroups

struct FragSum {     // the block scan's aggregate
    using Agg = FragAgg;
    static __device__ __forceinline__ Agg none() { return frag_none(); }
    static __device__ __forceinline__ Agg join(const Agg& a, const Agg& b) { return frag_join(a, b); }
};

// Record i (< n) of the trusted offsets. The wire is not read by the plan.
__device__ __forceinline__ FragRec fg_rec(const FragmentArgs& a, uint64_t i) {
    return frag_rec(a.rec_off[i + 1] - a.rec_off[i], a.max_frag);
}

__global__ __launch_bounds__(kFgThreads) void fragp_blk_kernel(FragmentArgs a) {
    __shared__ FragAgg s_wave[kFgThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kFgThreads + threadIdx.x;
    const FragAgg v = i < a.n ? frag_elem(fg_rec(a, i)) : frag_none();
    block_total<FragSum>(v, s_wave, a.blk);
}

// blk[b] := the sum of the blocks before b; blk[nblk] := the whole batch.
__global__ __launch_bounds__(kFgThreads) void fragp_blkscan_kernel(FragmentArgs a, uint64_t nblk) {
    __shared__ FragAgg s_wave[kFgThreads / 64];
    scan_blocks<FragSum>(a.blk, nblk, s_wave, [&] {
        a.info[0] = ~0ull;      // the first record that does not fit starts here (fragp_apply)
    });
}

__global__ __launch_bounds__(kFgThreads) void fragp_apply_kernel(FragmentArgs a) {
    __shared__ FragAgg s_wave[kFgThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kFgThreads + threadIdx.x;
    FragRec r{0, 0, ONC_OK};
    if (i < a.n) r = fg_rec(a, i);
    FragAgg total;
    const FragAgg ex = frag_join(a.blk[blockIdx.x], block_excl<FragSum>(frag_elem(r), s_wave, &total));
    if (i >= a.n) return;
    const uint64_t at = ex.bytes;
    a.out_off[i] = at;
    a.E[i] = a.origin + at;
    const int32_t st = frag_status(r, at, a.out_cap);
    // placements only grow and every record that can fail here takes bytes:
    // the one failing record that still starts within the capacity is the
    // first, and nothing from it on is written
    if (st == ONC_ENC_WRITE_ZERO && at <= a.out_cap) a.info[0] = at;
    a.status[i] = st;
    if (i == a.n - 1) {
        const FragAgg all = a.blk[(a.n + kFgThreads - 1) / kFgThreads];
        a.out_off[a.n] = all.bytes;
        a.E[a.n] = a.origin + all.bytes;
        a.result[0] = all.frags;
        a.result[1] = all.bytes;
        a.result[2] = all.multi;
    }
}

// Position q of a record whose output takes rlen bytes: a single-fragment
// record needs no division, one shorter than 4 GiB a 32-bit one.
__device__ __forceinline__ FragAt fg_at(uint64_t q, uint64_t rlen, uint32_t F) {
    if (q < frag_stride(F)) return FragAt{0, uint32_t(q)};
    if (rlen <= 0xFFFFFFFFull) return frag_at32(uint32_t(q), F);
    return frag_at(q, F);
}

// A chunk with one mark in it needs no byte loop either: the body bytes on
// both sides of a synthesised mark are neighbours in the wire, and so are the
// last bytes of a record and the next record's own mark and body. v = 16
// wire bytes as little-endian dwords (load16_unaligned); the big-endian mark
// goes to chunk bytes [t, t + 4), cut at 16.
struct MarkAt {
    uint32_t d0;      // dword of chunk byte t
    uint32_t lo, hi;  // the mark's bytes in dwords d0 and d0 + 1
    uint32_t klo, khi;   // and the bytes they cover
};
__device__ __forceinline__ MarkAt fg_mark_at(uint32_t mark, uint32_t t) {
    const uint32_t sh = 8 * (t & 3);
    const uint64_t m = uint64_t(__builtin_bswap32(mark)) << sh, k = uint64_t(0xFFFFFFFFu) << sh;
    return MarkAt{t >> 2, uint32_t(m), uint32_t(m >> 32), uint32_t(k), uint32_t(k >> 32)};
}
// The mark written over bytes [t, t + 4) of v (t in 0..15): a record's own
// mark replaced by its first fragment's.
__device__ __forceinline__ void fg_put_mark(uint32_t v[4], uint32_t mark, uint32_t t) {
    const MarkAt a = fg_mark_at(mark, t);
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
        const uint32_t k = d == a.d0 ? a.klo : d == a.d0 + 1 ? a.khi : 0u;
        const uint32_t m = d == a.d0 ? a.lo : d == a.d0 + 1 ? a.hi : 0u;
        v[d] = (v[d] & ~k) | m;
    }
}
// The mark inserted at byte t of v (t in 0..15): bytes [t, 12) move up by 4.
__device__ __forceinline__ void fg_insert_mark(uint32_t v[4], uint32_t mark, uint32_t t) {
    const MarkAt a = fg_mark_at(mark, t);
    uint32_t w[4];
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
        const uint32_t below = d ? v[d - 1] : 0u;
        const uint32_t body = d < a.d0 ? v[d] : d == a.d0 ? v[d] & ~a.klo : d == a.d0 + 1 ? below & ~a.khi : below;
        const uint32_t m = d == a.d0 ? a.lo : d == a.d0 + 1 ? a.hi : 0u;
        w[d] = body | m;
    }
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) v[d] = w[d];
}
// The chunk starts at byte r (1..3) of a mark: its last 4 - r bytes, then v.
__device__ __forceinline__ void fg_after_mark(uint32_t v[4], uint32_t mark, uint32_t r) {
    const uint32_t s = 8 * (4 - r);
    const uint32_t head = __builtin_bswap32(mark) >> (8 * r);
    uint32_t w[4];
    w[0] = (v[0] << s) | head;
#pragma unroll
    for (uint32_t d = 1; d < 4; ++d) w[d] = (v[d] << s) | (v[d - 1] >> (32 - s));
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) v[d] = w[d];
}

// The chunks of tile [t0, t0 + kFgTile) within [D0, D1) (coordinates: bytes
// from the 16-byte aligned address at or below the caller's out). e[0..n]:
// the output starts of the records reaching into the tile, e[0] <= the
// tile's first byte, e[n] >= its end; ro[0..n]: their wire offsets. A record
// that takes no output starts where the next one does, so the last record
// starting at or before a byte holds it — and that one has an extent of at
// least 4 bytes.
__device__ __forceinline__ void fg_copy_tile(const uint64_t* e, const uint64_t* ro, uint64_t n, uint32_t F,
                                             uintptr_t wire, uint8_t* __restrict__ out, uint64_t t0, uint64_t D0,
                                             uint64_t D1, int lane) {
#pragma unroll 2
    for (uint64_t cb = t0 + 16ull * lane; cb < t0 + kFgTile; cb += 1024) {
        if (cb + 16 <= D0 || cb >= D1) continue;
        const uint64_t b0 = max(cb, D0), b1 = min(cb + 16, D1);
        uint64_t j = last_at_or_before(e, n, b0);
        uint64_t ej = e[j], en = e[j + 1];
        uint64_t src = ro[j] + 4, B = ro[j + 1] - ro[j] - 4;
        FragAt at = fg_at(b0 - ej, en - ej, F);
        if (b1 - b0 == 16 && en >= b1 && frag_run16(at, B, F)) {
            uint32_t v[4];
            load16_unaligned(wire + src + frag_src(at, F), v);
            *reinterpret_cast<uint4*>(out + cb) = make_uint4(v[0], v[1], v[2], v[3]);
            continue;
        }
        uint32_t mark = frag_mark(B, at.j, F), flen = frag_body_len(B, at.j, F);
        if (b1 - b0 == 16 && F >= 12) {
            // one mark in the chunk and 16 wire bytes around it that belong
            // to records: one load, the mark put in by shifts
            const uint64_t s0 = at.j * F + (at.r < 4 ? 0 : at.r - 4);   // body offset of the chunk's first body byte
            uint32_t v[4];
            bool done = false;
            if (en >= b1) {                      // inside one record
                if (B - s0 >= 16 && (at.r >= 4 || flen >= 16)) {
                    load16_unaligned(wire + src + s0, v);
                    if (at.r == 0) fg_insert_mark(v, mark, 0);
                    else if (at.r < 4) fg_after_mark(v, mark, at.r);
                    else fg_insert_mark(v, frag_mark(B, at.j + 1, F), flen + 4 - at.r);   // this fragment's last bytes first
                    done = true;
                }
            } else if (at.r >= 4 && flen + 4 - at.r == en - b0) {
                // the record's last bytes, then the next extent: a record
                // that covers the rest of the chunk with its first fragment
                const uint32_t tail = uint32_t(en - b0);
                const uint64_t Ln = ro[j + 2] - ro[j + 1];
                if (Ln >= 16 - tail && Ln >= 4) {
                    load16_unaligned(wire + ro[j + 1] - tail, v);
                    fg_put_mark(v, frag_mark(Ln - 4, 0, F), tail);
                    done = true;
                }
            }
            if (done) {
                *reinterpret_cast<uint4*>(out + cb) = make_uint4(v[0], v[1], v[2], v[3]);
                continue;
            }
        }
        // several marks, a short record, or an end of the batch: byte by
        // byte, stepping (fragment, place in it) along
        for (uint64_t p = b0; p < b1; ++p) {
            if (p >= en) {                       // the next record that takes bytes
                do ++j; while (p >= e[j + 1]);
                ej = e[j];
                en = e[j + 1];
                src = ro[j] + 4;
                B = ro[j + 1] - ro[j] - 4;
                at = FragAt{0, 0};
                mark = frag_mark(B, 0, F);
                flen = frag_body_len(B, 0, F);
            } else if (at.r == flen + 4) {       // the next fragment of this record
                at = FragAt{at.j + 1, 0};
                mark = frag_mark(B, at.j, F);
                flen = frag_body_len(B, at.j, F);
            }
            out[p] = at.r < 4 ? frag_mark_byte(mark, at.r) : gload<uint8_t>(wire + src + frag_src(at, F));
            ++at.r;
        }
    }
}

// The walk is walk_tiles' (tile_walk.h) over the records' output starts E:
// E[0] = D0 and E[n] >= D1. Staged per record of a tile: its wire offset, and
// the one after the last (a record's extent ends where the next one starts).
__global__ __launch_bounds__(kFgThreads) void frag_copy_kernel(FragmentArgs a) {
    __shared__ uint64_t s_e[kFgThreads / 64][kCopyStage + 1];
    __shared__ uint64_t s_r[kFgThreads / 64][kCopyStage + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t W = min(a.info[0], a.E[a.n] - a.origin);   // OK records fill [0, W), W <= out_cap
    if (W == 0) return;
    const uint64_t D0 = a.origin, D1 = a.origin + W;
    const uintptr_t wire = reinterpret_cast<uintptr_t>(a.wire);
    uint64_t* sr = s_r[wv];
    walk_tiles<kFgTile>(
        SortedArray{a.E}, a.n, D0, D1, 0, s_e[wv],
        [&](const uint64_t* e, uint64_t j0, uint32_t nr, uint64_t t0, uint64_t, uint64_t) {
            for (uint32_t i = lane; i <= nr; i += 64) sr[i] = a.rec_off[j0 + i];
            wave_stage_done();
            fg_copy_tile(e, sr, nr, a.max_frag, wire, a.out, t0, D0, D1, lane);
        },
        [&](uint64_t j0, uint64_t nr, uint64_t t0, uint64_t, uint64_t) {
            fg_copy_tile(a.E + j0, a.rec_off + j0, nr, a.max_frag, wire, a.out, t0, D0, D1, lane);
        });
}

static uint32_t fg_blocks(uint64_t n) { return uint32_t((n + kFgThreads - 1) / kFgThreads); }

hipError_t launch_fragp_blk(const FragmentArgs& a, hipStream_t s) {
    ONC_LAUNCH(fragp_blk_kernel, dim3(fg_blocks(a.n)), dim3(kFgThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fragp_blkscan(const FragmentArgs& a, hipStream_t s) {
    ONC_LAUNCH(fragp_blkscan_kernel, dim3(1), dim3(kFgThreads), 0, s, a, uint64_t(fg_blocks(a.n)));
    return hipGetLastError();
}

hipError_t launch_fragp_apply(const FragmentArgs& a, hipStream_t s) {
    ONC_LAUNCH(fragp_apply_kernel, dim3(fg_blocks(a.n)), dim3(kFgThreads), 0, s, a);
    return hipGetLastError();
}

// The grid covers the capacity (what is written is known on the device
// only), up to kFgMaxBlocks workgroups; the kernel deals the tiles out.
hipError_t launch_frag_copy(const FragmentArgs& a, hipStream_t s, uint32_t variant) {
    const uint64_t wgs = copy_groups(a.origin, a.out_cap, kFgTile * (kFgThreads / 64));
    const uint64_t most = copy_max_groups(variant, kFgMaxBlocks);
    ONC_LAUNCH(frag_copy_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kFgThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
