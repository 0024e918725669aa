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
//                   count), each wave a run of consecutive tiles. The
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

namespace onc {

constexpr int kDfThreads = 256;
constexpr uint64_t kDfTile = 8192;      // output bytes per wave and step
constexpr uint32_t kDfStage = 128;      // fragments of a tile kept in LDS (more: searched in global memory)
constexpr uint32_t kDfMaxBlocks = 2048; // defrag_copy workgroups (the tiles are dealt out among their waves)

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), d, 64));
    const uint32_t hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), d, 64));
    return uint64_t(lo) | (uint64_t(hi) << 32);
}
__device__ __forceinline__ DefragAgg shfl_up_agg(const DefragAgg& v, int d) {
    return DefragAgg{shfl_up_u64(v.tail, d), shfl_up_u64(v.lasts, d), shfl_up_u64(v.cnt, d), shfl_up_u64(v.has, d)};
}
__device__ __forceinline__ DefragAgg wave_incl_agg(DefragAgg v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const DefragAgg o = shfl_up_agg(v, d);
        if (lane >= d) v = defrag_join(o, v);
    }
    return v;
}
// The run of the block's elements before this thread's; *total = the block.
__device__ __forceinline__ DefragAgg block_excl_agg(const DefragAgg& v, DefragAgg* s_wave, DefragAgg* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DefragAgg incl = wave_incl_agg(v);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    DefragAgg base = defrag_none(), sum = defrag_none();
#pragma unroll
    for (int w = 0; w < kDfThreads / 64; ++w) {
        const DefragAgg t = s_wave[w];
        if (w < wave) base = defrag_join(base, t);
        sum = defrag_join(sum, t);
    }
    *total = sum;
    __syncthreads();   // s_wave is reused by the caller's next round
    DefragAgg prev = shfl_up_agg(incl, 1);
    if (lane == 0) prev = defrag_none();
    return defrag_join(base, prev);
}

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
    DefragAgg total;
    block_excl_agg(v, s_wave, &total);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// blk[b] := the run of the blocks before b; blk[nblk] := the whole batch.
__global__ __launch_bounds__(kDfThreads) void defrag_blkscan_kernel(DefragArgs a, uint64_t nblk) {
    __shared__ DefragAgg s_wave[kDfThreads / 64];
    DefragAgg carry = defrag_none();
    for (uint64_t b0 = 0; b0 < nblk; b0 += kDfThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const DefragAgg v = b < nblk ? a.blk[b] : defrag_none();
        DefragAgg total;
        const DefragAgg ex = block_excl_agg(v, s_wave, &total);
        if (b < nblk) a.blk[b] = defrag_join(carry, ex);
        carry = defrag_join(carry, total);
    }
    if (threadIdx.x == 0) {
        a.blk[nblk] = carry;
        a.info[0] = 0;          // n_multi (defrag_frag adds)
        a.info[1] = ~0ull;      // the first record that does not fit starts here (defrag_place)
    }
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
    const DefragAgg ex = defrag_join(a.blk[blockIdx.x], block_excl_agg(v, s_wave, &total));
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

// Every wave takes a run of consecutive tiles, so that only its first tile
// searches the fragments in global memory (about 20 dependent loads: with a
// search per tile the kernel spent a quarter of its time there). From then
// on the tile's fragments are found in a window of kDfStage + 1 consecutive
// entries of E staged in LDS from the previous tile's last fragment on: E is
// sorted, so how many entries lie at or before a byte is a ballot count.
__global__ __launch_bounds__(kDfThreads) void defrag_copy_kernel(DefragArgs a) {
    __shared__ uint64_t s_e[kDfThreads / 64][kDfStage + 1];
    __shared__ uint64_t s_s[kDfThreads / 64][kDfStage];
    __shared__ uint32_t s_m[kDfThreads / 64][kDfStage];
    static_assert(kDfStage == 128, "the window is staged and counted as two rounds of 64 lanes + 1");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t W = min(a.info[1], a.off[a.nfrag]);   // OK records fill [0, W), W <= out_cap
    if (W == 0) return;
    const uint64_t D0 = a.origin, D1 = a.origin + W;
    const uint64_t ntiles = (D1 + kDfTile - 1) / kDfTile;
    const uintptr_t wire = reinterpret_cast<uintptr_t>(a.wire);
    const uint64_t nw = uint64_t(gridDim.x) * (kDfThreads / 64);
    const uint64_t per = (ntiles + nw - 1) / nw;
    const uint64_t T0 = (uint64_t(blockIdx.x) * (kDfThreads / 64) + wv) * per;   // wave-uniform
    const uint64_t T1 = min(T0 + per, ntiles);
    if (T0 >= T1) return;
    uint64_t* se = s_e[wv];
    // E[0] = D0 <= lo and E[nfrag] >= D1: every search ends below nfrag.
    // ja: a fragment with E[ja] <= the tile's first byte (kept across tiles)
    uint64_t ja = last_at_or_before(a.E, a.nfrag + 1, max(T0 * kDfTile, D0));
    for (uint64_t T = T0; T < T1; ++T) {
        const uint64_t t0 = T * kDfTile;
        const uint64_t lo = max(t0, D0), hi = min(t0 + kDfTile, D1);
        uint32_t k, c_hi;
        for (;;) {
            __builtin_amdgcn_wave_barrier();   // the tile before may still read the stage
            // (past the array the window repeats E[nfrag] >= D1: never counted)
            const uint64_t e0 = a.E[min(ja + lane, a.nfrag)], e1 = a.E[min(ja + 64 + lane, a.nfrag)];
            const uint64_t e2 = a.E[min(ja + kDfStage, a.nfrag)];
            se[lane] = e0;
            se[64 + lane] = e1;
            if (lane == 0) se[kDfStage] = e2;
            const uint32_t c_lo = __popcll(__ballot(e0 <= lo)) + __popcll(__ballot(e1 <= lo)) + (e2 <= lo ? 1u : 0u);
            c_hi = __popcll(__ballot(e0 < hi)) + __popcll(__ballot(e1 < hi)) + (e2 < hi ? 1u : 0u);
            if (c_lo == kDfStage + 1) {        // the tile starts beyond the window: search on from its end
                ja += kDfStage;
                ja += last_at_or_before(a.E + ja, a.nfrag + 1 - ja, lo);
                continue;
            }
            k = c_lo - 1;                      // window entry of the fragment holding the tile's first byte
            if (c_hi == kDfStage + 1 && k != 0) {   // the window ends inside the tile: start it at that fragment
                ja += k;
                continue;
            }
            break;
        }
        if (c_hi == kDfStage + 1) {
            // more than kDfStage fragments reach into the tile: in global memory
            const uint64_t jb = ja + kDfStage + last_at_or_before(a.E + ja + kDfStage, a.nfrag + 1 - ja - kDfStage, hi - 1);
            copy_tile(a.E + ja, a.S + ja, a.M + ja, jb - ja + 1, wire, a.out, t0, D0, D1, lane);
            ja = jb;
            continue;
        }
        const uint32_t n = c_hi - k;           // window entries k .. c_hi - 1 reach into the tile
        for (uint32_t i = lane; i < n; i += 64) {
            s_s[wv][i] = a.S[ja + k + i];
            s_m[wv][i] = a.M[ja + k + i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        copy_tile(se + k, s_s[wv], s_m[wv], n, wire, a.out, t0, D0, D1, lane);
        ja += c_hi - 1;                        // the fragment holding the tile's last byte holds the next one's first or comes before it
    }
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
    const uint64_t per_wg = kDfTile * (kDfThreads / 64);
    const uint64_t cap = a.out_cap > ~0ull - 16 - per_wg ? ~0ull - 16 - per_wg : a.out_cap;
    const uint64_t wgs = (a.origin + cap + per_wg - 1) / per_wg;
    const uint64_t most = copy_max_groups(variant, kDfMaxBlocks);
    ONC_LAUNCH(defrag_copy_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kDfThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
