// defrag.hip — multi-fragment record reassembly on gfx950 (onc_defragment,
// include/onc_rpc.h; SURVEY §8(f) rank 1, second half).
//
// The reference rejects a record whose mark has the last-fragment bit clear
// (Error::Fragmented, rpc_message.rs:359-362; README.md:62). RFC 5531 §11
// lets a sender split a record into any number of fragments, each under its
// own mark. From the fragment offsets (onc_frame_fragments) these kernels
// rebuild the stream serialise_into would have written: per record one mark
// with the last-fragment bit and the total length (rpc_message.rs:156), then
// the fragments' bodies in order. Lengths, then scan, then emit, as the
// encoder:
//
//   defrag_blk      per 256 fragments: the plan state of the block as a run
//                   (defrag_plan.h DefragAgg: records closed, open record's
//                   fragments and body bytes); zeroes the record lengths
//   defrag_blkscan  one workgroup: exclusive scan of the block states
//   defrag_frag     per fragment: the state before it = its record index,
//                   the body bytes before it in its record, first-of-record;
//                   a last fragment closes its record: B_r -> the record's
//                   length (0: ONC_ENC_TOO_LONG)
//   (scan)          onc_scan_lengths of the record lengths: the placement
//   defrag_place    rec_off, status (capacity), result; per fragment where
//                   its bytes go in `out`, where they come from, its mark
//   defrag_copy     the hot path: a wave per 8 KiB tile of *output* (a
//                   fragment may be empty or many MiB, so never by fragment
//                   count), each wave a run of consecutive tiles: the walk
//                   written down in tile_walk.h (walk_tiles). The
//                   fragments that reach into the tile are staged in LDS
//                   (found by binary search for the wave's first tile, from
//                   the tile before after that); every 16-byte output
//                   chunk finds its fragment there by binary search: one
//                   unaligned 16-byte load and one aligned 16-byte store
//                   when the chunk lies inside one fragment's bytes, byte by
//                   byte at seams, at the synthesised marks and at the ends
//                   (compact.hip compact_gather is the precedent).
//
// onc_defragment_extents runs the same kernels on fragments that are not back
// to back (frag_start / frag_len instead of frag_off): defrag_blk, defrag_frag
// and defrag_place have an extents form (kExt); the copy works from absolute
// sources and has one form.
#include "common.h"
#include "defrag_plan.h"
#include "kernels.h"
#include "tile_walk.h"

namespace onc {

constexpr int kDfThreads = kCopyThreads;
constexpr uint64_t kDfTile = 8192;      // output bytes per wave and step
constexpr uint32_t kDfMaxBlocks = kCopyMaxBlocks;   // defrag_copy workgroups

struct DefragRun {   // the block scan's aggregate: the plan state of a run of fragments
    using Agg = DefragAgg;
    static __device__ __forceinline__ Agg none() { return defrag_none(); }
    static __device__ __forceinline__ Agg join(const Agg& a, const Agg& b) { return defrag_join(a, b); }
};

struct FragElem {
    uint64_t body;
    bool last;
};
// Fragment j (< nfrag): its mark is read only for bit 31 (the first byte).
// kExt: the extents form (onc_defragment_extents) — fragment j lies at
// frag_start[j] and is frag_len[j] bytes long, its mark included; only this
// and defrag_place look at where the fragments are.
template <bool kExt>
__device__ __forceinline__ FragElem frag_elem(const DefragArgs& a, uint64_t j) {
    if constexpr (kExt) {
        const uint64_t lo = a.frag_start[j];
        return FragElem{defrag_body(0, a.frag_len[j]), (a.wire[lo] & 0x80u) != 0};
    } else {
        const uint64_t lo = a.frag_off[j], hi = a.frag_off[j + 1];
        return FragElem{defrag_body(lo, hi), (a.wire[lo] & 0x80u) != 0};
    }
}

template <bool kExt>
__global__ __launch_bounds__(kDfThreads) void defrag_blk_kernel(DefragArgs a) {
    __shared__ DefragAgg s_wave[kDfThreads / 64];
    const uint64_t j = uint64_t(blockIdx.x) * kDfThreads + threadIdx.x;
    DefragAgg v = defrag_none();
    if (j < a.nfrag) {
        const FragElem f = frag_elem<kExt>(a, j);
        v = defrag_elem(f.body, f.last);
        // lengths past the last record scan as 0 (how many records there are
        // is known on the device only; defrag_frag sets the records'). Zeroed
        // here and not by a memset on the stream: every step of the call is a
        // kernel launch, so a captured call is a chain of kernel nodes.
        a.lens[j] = 0;
    }
    block_total<DefragRun>(v, s_wave, a.blk);
}

// blk[b] := the run of the blocks before b; blk[nblk] := the whole batch.
__global__ __launch_bounds__(kDfThreads) void defrag_blkscan_kernel(DefragArgs a, uint64_t nblk) {
    __shared__ DefragAgg s_wave[kDfThreads / 64];
    scan_blocks<DefragRun>(a.blk, nblk, s_wave, [&] {
        a.info[0] = 0;          // n_multi (defrag_frag adds)
        a.info[1] = ~0ull;      // the first record that does not fit starts here (defrag_place)
    });
}

// Between this kernel and defrag_place the per-fragment arrays hold the plan:
// E = body bytes before the fragment in its record, S = its record index,
// M = 1 for the first fragment of a record.
template <bool kExt>
__global__ __launch_bounds__(kDfThreads) void defrag_frag_kernel(DefragArgs a) {
    __shared__ DefragAgg s_wave[kDfThreads / 64];
    const uint64_t j = uint64_t(blockIdx.x) * kDfThreads + threadIdx.x;
    DefragAgg v = defrag_none();
    FragElem f{0, false};
    if (j < a.nfrag) {
        f = frag_elem<kExt>(a, j);
        v = defrag_elem(f.body, f.last);
    }
    DefragAgg total;
    const DefragAgg ex = defrag_join(a.blk[blockIdx.x], block_excl<DefragRun>(v, s_wave, &total));
    bool multi = false;
    if (j < a.nfrag) {
        a.E[j] = ex.tail;
        a.S[j] = ex.lasts;
        a.M[j] = ex.cnt == 0 ? 1u : 0u;
        if (f.last) {
            a.lens[ex.lasts] = defrag_len(ex.tail + f.body);
            multi = ex.cnt != 0;
        }
    }
    const uint64_t m = __ballot(multi);
    if (m && (threadIdx.x & 63) == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.info[0]), static_cast<unsigned long long>(__popcll(m)));
}

// Thread i: record i (rec_off, status), fragment i (its placement), and for
// i == 0 the result. off = the scan of the record lengths over nfrag entries
// (zero past the last record, so off[nfrag] = the bytes the batch needs).
// kExt: result[1] counts the fragments consumed (there is no stream offset
// to give).
template <bool kExt>
__global__ __launch_bounds__(kDfThreads) void defrag_place_kernel(DefragArgs a) {
    const uint64_t i = uint64_t(blockIdx.x) * kDfThreads + threadIdx.x;
    if (i > a.nfrag) return;
    const DefragAgg all = a.blk[(a.nfrag + kDfThreads - 1) / kDfThreads];
    const uint64_t nrec = all.lasts;
    const uint64_t need = a.off[a.nfrag];
    if (i <= nrec) a.rec_off[i] = a.off[i];
    if (i < nrec) {
        const uint64_t len = a.lens[i], at = a.off[i];
        int32_t st = ONC_ENC_TOO_LONG;
        if (len != 0) {
            st = defrag_fits(at, len, a.out_cap) ? ONC_OK : ONC_ENC_WRITE_ZERO;
            // placements only grow: the one failing record that still starts
            // within the capacity is the first, and nothing from it on is written
            if (st != ONC_OK && at <= a.out_cap) a.info[1] = at;
        }
        a.status[i] = st;
    }
    if (i < a.nfrag) {
        const uint64_t r = a.S[i], pre = a.E[i];
        const bool first = a.M[i] != 0;
        uint64_t e = need;                      // a pending fragment: no bytes, at the end
        uint32_t mark = 0;
        if (r < nrec) {
            const uint32_t len = a.lens[r];
            e = a.off[r];
            if (len != 0) {
                if (first) mark = defrag_mark(len - 4u);
                else e += 4 + pre;
            }
        }
        // the first fragment's extent starts with its mark: its four wire
        // bytes stand where the synthesised mark goes (S = the mark); a
        // continuation's extent is its body
        a.E[i] = a.origin + e;
        a.S[i] = (kExt ? a.frag_start[i] : a.frag_off[i]) + (first ? 0 : 4);
        a.M[i] = mark;
    } else {
        a.E[i] = a.origin + need;
    }
    if (i == 0) {
        a.result[0] = nrec;
        a.result[1] = kExt ? a.nfrag - all.cnt : a.frag_off[a.nfrag - all.cnt];
        a.result[2] = need;
        a.result[3] = all.cnt;
        a.result[4] = all.tail;
        a.result[5] = a.info[0];
    }
}

// The chunks of tile [t0, t0 + kDfTile) within [D0, D1) (coordinates: bytes
// from the 16-byte aligned address at or below the caller's out). e[0..n],
// s / m[0..n-1]: the fragments reaching into the tile, e[0] <= the tile's
// first byte, e[n] >= its end; an empty fragment starts where the next one
// does, so the last fragment starting at or before a byte holds it.
__device__ __forceinline__ void copy_tile(const uint64_t* e, const uint64_t* s, const uint32_t* m, uint64_t n,
                                          uintptr_t wire, uint8_t* __restrict__ out, uint64_t t0, uint64_t D0,
                                          uint64_t D1, int lane) {
#pragma unroll 2
    for (uint64_t cb = t0 + 16ull * lane; cb < t0 + kDfTile; cb += 1024) {
        if (cb + 16 <= D0 || cb >= D1) continue;
        const uint64_t b0 = max(cb, D0), b1 = min(cb + 16, D1);
        uint64_t j = last_at_or_before(e, n, b0);
        const uint64_t o0 = b0 - e[j];
        if (b1 - b0 == 16 && e[j + 1] >= b1 && !(m[j] != 0 && o0 < 4)) {
            uint32_t v[4];
            load16_unaligned(wire + s[j] + o0, v);
            *reinterpret_cast<uint4*>(out + cb) = make_uint4(v[0], v[1], v[2], v[3]);
            continue;
        }
        // a seam, a mark or an end of the batch: byte by byte. (Issuing a
        // chunk's byte loads together instead of one round trip each was
        // tried: 115 VGPRs against 69 and the same kernel time.)
        for (uint64_t p = b0; p < b1; ++p) {
            while (p >= e[j + 1]) ++j;
            const uint64_t o = p - e[j];
            const uint32_t mk = m[j];
            out[p] = (mk != 0 && o < 4) ? uint8_t(mk >> (24 - 8 * uint32_t(o)))
                                        : gload<uint8_t>(wire + s[j] + o);
        }
    }
}

// The walk is walk_tiles' (tile_walk.h) over the fragments' output starts E:
// E[0] = D0 and E[nfrag] >= D1. Staged per fragment of a tile: S and M.
__global__ __launch_bounds__(kDfThreads) void defrag_copy_kernel(DefragArgs a) {
    __shared__ uint64_t s_e[kDfThreads / 64][kCopyStage + 1];
    __shared__ uint64_t s_s[kDfThreads / 64][kCopyStage];
    __shared__ uint32_t s_m[kDfThreads / 64][kCopyStage];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t W = min(a.info[1], a.off[a.nfrag]);   // OK records fill [0, W), W <= out_cap
    if (W == 0) return;
    const uint64_t D0 = a.origin, D1 = a.origin + W;
    const uintptr_t wire = reinterpret_cast<uintptr_t>(a.wire);
    walk_tiles<kDfTile>(
        SortedArray{a.E}, a.nfrag, D0, D1, 0, s_e[wv],
        [&](const uint64_t* e, uint64_t j0, uint32_t n, uint64_t t0, uint64_t, uint64_t) {
            for (uint32_t i = lane; i < n; i += 64) {
                s_s[wv][i] = a.S[j0 + i];
                s_m[wv][i] = a.M[j0 + i];
            }
            wave_stage_done();
            copy_tile(e, s_s[wv], s_m[wv], n, wire, a.out, t0, D0, D1, lane);
        },
        [&](uint64_t j0, uint64_t n, uint64_t t0, uint64_t, uint64_t) {
            copy_tile(a.E + j0, a.S + j0, a.M + j0, n, wire, a.out, t0, D0, D1, lane);
        });
}

static uint32_t df_blocks(uint64_t n) { return uint32_t((n + kDfThreads - 1) / kDfThreads); }

hipError_t launch_defrag_blk(const DefragArgs& a, hipStream_t s) {
    if (a.frag_start) ONC_LAUNCH(defrag_blk_kernel<true>, dim3(df_blocks(a.nfrag)), dim3(kDfThreads), 0, s, a);
    else ONC_LAUNCH(defrag_blk_kernel<false>, dim3(df_blocks(a.nfrag)), dim3(kDfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_defrag_blkscan(const DefragArgs& a, hipStream_t s) {
    ONC_LAUNCH(defrag_blkscan_kernel, dim3(1), dim3(kDfThreads), 0, s, a, uint64_t(df_blocks(a.nfrag)));
    return hipGetLastError();
}

hipError_t launch_defrag_frag(const DefragArgs& a, hipStream_t s) {
    if (a.frag_start) ONC_LAUNCH(defrag_frag_kernel<true>, dim3(df_blocks(a.nfrag)), dim3(kDfThreads), 0, s, a);
    else ONC_LAUNCH(defrag_frag_kernel<false>, dim3(df_blocks(a.nfrag)), dim3(kDfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_defrag_place(const DefragArgs& a, hipStream_t s) {
    if (a.frag_start) ONC_LAUNCH(defrag_place_kernel<true>, dim3(df_blocks(a.nfrag + 1)), dim3(kDfThreads), 0, s, a);
    else ONC_LAUNCH(defrag_place_kernel<false>, dim3(df_blocks(a.nfrag + 1)), dim3(kDfThreads), 0, s, a);
    return hipGetLastError();
}

// The grid covers the capacity (what is written is known on the device
// only), up to kDfMaxBlocks workgroups; the kernel deals the tiles out.
hipError_t launch_defrag_copy(const DefragArgs& a, hipStream_t s, uint32_t variant) {
    const uint64_t wgs = copy_groups(a.origin, a.out_cap, kDfTile * (kDfThreads / 64));
    const uint64_t most = copy_max_groups(variant, kDfMaxBlocks);
    ONC_LAUNCH(defrag_copy_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kDfThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
