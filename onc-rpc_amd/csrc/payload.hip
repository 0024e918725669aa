// payload.hip — head-decoded payloads placed in aligned slots on gfx950
// (onc_payload_slots / onc_place_payloads, include/onc_rpc.h): the receive-side
// counterpart of gather.hip. After onc_defragment_heads + onc_decode_heads (or
// onc_frame_streams + onc_decode_extents) every payload still lies where it
// arrived, scattered over its record's fragments; here each payload byte moves
// once, into a slot of the caller's buffer.
//
//   pay_blk      per 256 records: the block's {slot bytes, records with a
//                payload, payload bytes} (payload_plan.h PayAgg)
//   pay_blkscan  one workgroup: exclusive scan of the block sums
//   pay_apply    per record: pay_pos, pay_len, slot_off and the descriptor with
//                its payload_off rebased to the slot; the last record:
//                slot_off[n] and result (pay_empty: the same two for no records)
//   place_copy   the hot path: gather_copy (gather.hip) with one more level of
//                lookup. A wave per 8 KiB tile of `dst` (counted from the
//                16-byte aligned address at or below it, so that every full
//                store is aligned), each wave a run of consecutive tiles
//                (tile_walk.h walk_tiles); the
//                records whose slots reach into the tile are found by one
//                binary search of slot_off at the run's start and followed
//                from there, and staged in LDS: slot start, body position of
//                the slice, how many bytes of it may be copied (0 for a slice
//                that is not OK), the record's fragment range, and the
//                slice's first run resolved (its address and its bytes in the
//                fragment holding its first byte). A 16-byte
//                chunk of dst inside one slice and one fragment is one
//                unaligned 16-byte load and one aligned 16-byte store; a chunk
//                that spans fragments, a slice's end or an end of dst goes
//                byte by byte: first every byte's address, then all the byte
//                loads in flight together. A chunk wholly in padding issues no
//                load. The fragment holding a body byte is heads_frag_of's:
//                the last one starting at or before it, so empty fragments in
//                a record's middle hold nothing.
//
// The copy walks "entries": entry 0 is a slice of no bytes at slot 0 (a
// caller's own slot list may start anywhere), entry j > 0 is record j - 1, and
// every entry past the last starts at 2^64 - 1. slot_off[n] is never read.
#include "common.h"
#include "defrag_heads_plan.h"
#include "kernels.h"
#include "payload_plan.h"
#include "tile_walk.h"

namespace onc {

constexpr int kPlThreads = kCopyThreads;
constexpr uint64_t kPlTile = 8192;      // dst bytes per wave and step
constexpr uint32_t kPlMaxBlocks = kCopyMaxBlocks;   // place_copy workgroups

struct PaySum {      // the block scan's aggregate
    using Agg = PayAgg;
    static __device__ __forceinline__ Agg none() { return payload_none(); }
    static __device__ __forceinline__ Agg join(const Agg& a, const Agg& b) { return payload_join(a, b); }
};

// Record i (< n): the descriptor's first and fourth 16 bytes hold every word
// the slots need (xid .. call.program, then payload_len, payload_off).
struct PlMsg {
    uint32_t payload_len;
    uint64_t payload_off;
    bool has;
};
__device__ __forceinline__ PlMsg pl_msg(const PaySlotsArgs& a, uint64_t i) {
    const onc_msg* m = a.msgs + i;
    const uint32_t plen = m->payload_len;
    const bool has = payload_has(a.status[i], m->msg_type, m->reply_stat, m->stat, plen);
    return PlMsg{plen, m->payload_off, has};
}
__device__ __forceinline__ PayAgg pl_elem(const PaySlotsArgs& a, uint64_t i) {
    if (i >= a.n) return payload_none();
    const PlMsg m = pl_msg(a, i);
    return payload_elem(m.has, m.payload_len, a.align);
}

__global__ __launch_bounds__(kPlThreads) void pay_blk_kernel(PaySlotsArgs a) {
    __shared__ PayAgg s_wave[kPlThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kPlThreads + threadIdx.x;
    block_total<PaySum>(pl_elem(a, i), s_wave, a.blk);
}

// blk[b] := the sum of the blocks before b; blk[nblk] := the whole batch.
__global__ __launch_bounds__(kPlThreads) void pay_blkscan_kernel(PaySlotsArgs a, uint64_t nblk) {
    __shared__ PayAgg s_wave[kPlThreads / 64];
    scan_blocks<PaySum>(a.blk, nblk, s_wave, [] {});
}

// (msgs_out may be msgs: a thread reads its own descriptor whole before it
// writes it.)
__global__ __launch_bounds__(kPlThreads) void pay_apply_kernel(PaySlotsArgs a) {
    __shared__ PayAgg s_wave[kPlThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kPlThreads + threadIdx.x;
    MsgRegs regs{};
    PlMsg m{0, 0, false};
    if (i < a.n) {
        regs = issue_msg(a.msgs + i);
        const onc_msg d = as_msg(regs);
        m = PlMsg{d.payload_len, d.payload_off,
                  payload_has(a.status[i], d.msg_type, d.reply_stat, d.stat, d.payload_len)};
    }
    PayAgg total;
    const PayAgg ex = payload_join(a.blk[blockIdx.x],
                                   block_excl<PaySum>(payload_elem(m.has, m.payload_len, a.align), s_wave, &total));
    if (i >= a.n) return;
    const uint64_t base = a.rec_start ? a.rec_start[i] : i * uint64_t(a.head_len);
    a.pay_pos[i] = m.has ? uint32_t(m.payload_off - base) : 0u;
    a.pay_len[i] = m.has ? m.payload_len : 0u;
    a.slot_off[i] = ex.off;
    if (a.msgs_out) {
        onc_msg d = as_msg(regs);
        if (m.has) d.payload_off = ex.off;
        MsgRegs o;
        __builtin_memcpy(&o, &d, sizeof(d));
        u32x4* q = reinterpret_cast<u32x4*>(a.msgs_out + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = o.q[k];
    }
    if (i == a.n - 1) {
        const PayAgg all = a.blk[(a.n + kPlThreads - 1) / kPlThreads];
        a.slot_off[a.n] = all.off;
        payload_result(a.result, all);
    }
}

// No records (a kernel and not a memset: every step of the call is a kernel
// launch, so a captured call is a chain of kernel nodes).
__global__ void pay_empty_kernel(PaySlotsArgs a) {
    a.slot_off[0] = 0;
    payload_result(a.result, payload_none());
}

// ---------------------------------------------------------------------------
// place_copy
// ---------------------------------------------------------------------------
// An entry's slice: body bytes [x0, x0 + vlen) of the record whose fragments
// are [lo, hi). vlen == 0: nothing is read and nothing written (an empty
// slice, one that is not OK, entry 0 and the entries past the last record).
// The slice's first run is resolved when the entry is staged: its first byte
// lies at addr0, in fragment lo (the fragments before it are never looked
// at), with room0 bytes of the slice from there on in that fragment. A chunk
// inside the first run — every chunk of a single-fragment record — needs no
// lookup of its own.
struct PlRec {
    uint64_t lo, hi;
    uint64_t addr0;
    uint32_t x0, vlen, room0;
};
__device__ __forceinline__ uint64_t pl_pos(const PlaceArgs& a, uint64_t j) {
    return j == 0 ? 0ull : j <= a.n ? a.slot_off[j - 1] : ~0ull;
}

// Where body byte x of a record lies: its address, and how many bytes from it
// on lie in the same fragment (0: none — the extents disagree with the
// record's length; nothing is read then).
struct PlRun {
    uint64_t addr;
    uint64_t room;
    uint64_t j;
};
__device__ __forceinline__ PlRun pl_run_at(const PlaceArgs& a, uint64_t j, uint64_t x) {
    const uint64_t pre = a.frag_pre ? a.frag_pre[j] : 0ull;
    const uint64_t fs = a.frag_start[j];
    const uint64_t body = uint64_t(a.frag_len[j]) - 4;      // (an extent holds its mark)
    const uint64_t at = x - pre;
    return PlRun{uint64_t(reinterpret_cast<uintptr_t>(a.wire)) + fs + 4 + at, at < body ? body - at : 0ull, j};
}
// The fragment of [lo, hi) holding body byte x (heads_frag_of). Up to four
// fragments are probed with loads that do not depend on each other: frag_pre
// is sorted inside a record, so the entries at or before x are counted.
__device__ __forceinline__ PlRun pl_locate(const PlaceArgs& a, uint64_t lo, uint64_t hi, uint64_t x) {
    if (!a.frag_pre) return pl_run_at(a, lo, x);
    const uint64_t nf = hi - lo;
    if (nf > 4) return pl_run_at(a, heads_frag_of(a.frag_pre, lo, hi, x), x);
    const uint64_t p1 = a.frag_pre[lo + min(nf - 1, uint64_t(1))];
    const uint64_t p2 = a.frag_pre[lo + min(nf - 1, uint64_t(2))];
    const uint64_t p3 = a.frag_pre[lo + min(nf - 1, uint64_t(3))];
    const uint64_t j = lo + (nf > 1 && p1 <= x) + (nf > 2 && p2 <= x) + (nf > 3 && p3 <= x);
    return pl_run_at(a, j, x);
}
__device__ __forceinline__ PlRec pl_rec(const PlaceArgs& a, uint64_t j) {
    const PlRec none{0, 0, 0, 0, 0, 0};
    if (j == 0 || j > a.n) return none;
    const uint64_t r = j - 1;
    const uint32_t len = a.pay_len[r];
    if (len == 0) return none;
    const uint32_t pos = a.pay_pos[r];
    if (!payload_ok(pos, len, a.rec_len[r], a.slot_off[r], a.dst_cap)) return none;
    uint64_t lo = r, hi = r + 1;
    if (a.rec_frag) {
        lo = a.rec_frag[r];
        hi = a.rec_frag[r + 1];
        if (lo >= hi) return none;                           // (a record of no fragments holds no byte)
    }
    const PlRun f = pl_locate(a, lo, hi, pos - 4u);
    return PlRec{f.j, hi, f.addr, pos - 4u, len, uint32_t(min(f.room, uint64_t(len)))};
}
// The run after `f` ends at body byte x (= where f's fragment ends): the next
// fragment, past the empty ones (the last fragment starting at or before x).
__device__ __forceinline__ PlRun pl_next(const PlaceArgs& a, const PlRec& s, const PlRun& f, uint64_t x) {
    uint64_t j = f.j + 1;
    if (j >= s.hi) return PlRun{0, 0, f.j};
    while (j + 1 < s.hi && a.frag_pre[j + 1] <= x) ++j;
    return pl_run_at(a, j, x);
}

// The entries reaching into a tile: pos(0 .. n) their slot starts, pos(0) <=
// the tile's first byte and pos(n) >= its end; rec(0 .. n - 1).
struct PlStaged {          // in LDS
    const uint64_t* e;
    const uint64_t* lo;
    const uint64_t* hi;
    const uint64_t* a0;
    const uint32_t* x0;
    const uint32_t* v;
    const uint32_t* r0;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return e[j]; }
    __device__ __forceinline__ PlRec rec(uint64_t j) const { return PlRec{lo[j], hi[j], a0[j], x0[j], v[j], r0[j]}; }
};
struct PlGlobal {          // more than kCopyStage of them: from entry j0 on in global memory
    const PlaceArgs& a;
    uint64_t j0;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return pl_pos(a, j0 + j); }
    __device__ __forceinline__ PlRec rec(uint64_t j) const { return pl_rec(a, j0 + j); }
};

// What the walk is over: the entries' slot starts, searched among the entries
// themselves.
struct PlEntries {
    const PlaceArgs& a;
    __device__ __forceinline__ uint64_t pos(uint64_t j) const { return pl_pos(a, j); }
    __device__ __forceinline__ uint64_t search(uint64_t j0, uint64_t n, uint64_t x) const {
        return last_at_or_before(PlGlobal{a, j0}, n, x);
    }
};

// The chunks of tile [t0, t0 + kPlTile) within [D0, D1) (coordinates: bytes
// from the 16-byte aligned address at or below the caller's dst; byte D of
// them is slot position D + shift). Among entries starting at the same
// position only the last has bytes, so the last entry starting at or before a
// byte is the one whose slice can cover it. `spare`: an address that may
// always be read (slot_off).
template <class View>
__device__ __forceinline__ void pl_copy_tile(const PlaceArgs& a, const View& v, uint64_t n, uint64_t shift,
                                             uint64_t spare, uint8_t* __restrict__ out, uint64_t t0, uint64_t D0,
                                             uint64_t D1, int lane) {
#pragma unroll 2
    for (uint64_t cb = t0 + 16ull * lane; cb < t0 + kPlTile; cb += 1024) {
        if (cb + 16 <= D0 || cb >= D1) continue;
        const uint64_t b0 = max(cb, D0), b1 = min(cb + 16, D1);
        uint64_t j = last_at_or_before(v, n, b0 + shift);
        PlRec s = v.rec(j);
        const uint64_t o0 = b0 + shift - v.pos(j);
        const uint64_t P0 = b0 + shift;                       // the slot position of chunk byte i0
        const uint64_t nxt = v.pos(j + 1);                    // >= P0
        if (o0 >= s.vlen && nxt - P0 >= b1 - b0) continue;    // wholly in padding (or in a slice that is not OK)
        PlRun f{0, 0, 0};
        if (o0 < s.vlen) {
            f = o0 < s.room0 ? PlRun{s.addr0 + o0, s.room0 - o0, s.lo} : pl_locate(a, s.lo, s.hi, uint64_t(s.x0) + o0);
            if (b1 - b0 == 16 && s.vlen - o0 >= 16 && f.room >= 16) {
                uint32_t w[4];
                load16_unaligned(uintptr_t(f.addr), w);
                *reinterpret_cast<uint4*>(out + cb) = make_uint4(w[0], w[1], w[2], w[3]);
                continue;
            }
        }
        // a seam between fragments or slices, padding or an end of dst: byte
        // by byte. First every byte's address (the lookups are loads that are
        // waited for where they stand), then all the byte loads, so that they
        // are in flight together; a byte that is not written loads from
        // `spare` instead of branching around its load.
        // The walk counts in chunk bytes (32 bits): entry j holds chunk bytes
        // [i_at, i_nxt), of which `room` from i_at on may be copied, body
        // bytes x_at on; run f holds `f.room` of them from chunk byte f_at on.
        const uint32_t i0 = uint32_t(b0 - cb), i1 = uint32_t(b1 - cb);
        auto rel = [&](uint64_t pos) { return i0 + uint32_t(min(pos - P0, uint64_t(16))); };   // pos >= P0
        uint32_t i_at = i0, i_nxt = rel(nxt);
        uint32_t room = o0 < s.vlen ? uint32_t(min(uint64_t(s.vlen) - o0, uint64_t(16))) : 0u;
        uint64_t x_at = uint64_t(s.x0) + o0;
        uint32_t f_at = i0;
        uint64_t addr[16];
        uint32_t mask = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const bool in = i >= i0 && i < i1;
            if (in && i >= i_nxt) {                           // the next entry with bytes starts at this byte
                do i_nxt = rel(v.pos(++j + 1)); while (i >= i_nxt);
                s = v.rec(j);
                i_at = i;
                room = min(s.vlen, 16u);
                x_at = s.x0;
                f = PlRun{s.addr0, s.room0, s.lo};           // (room0 is 0 where room is)
                f_at = i;
            }
            const uint32_t k = i - i_at;
            bool ok = in && k < room;
            if (ok && uint64_t(i - f_at) >= f.room) {         // the fragment ends before this byte
                f = f.room ? pl_next(a, s, f, x_at + k) : f;
                f_at = i;
                if (f.room == 0) {                            // nothing more of this record can be read
                    room = k;
                    ok = false;
                }
            }
            mask |= ok ? 1u << i : 0u;
            addr[i] = ok ? f.addr + (i - f_at) : spare;
        }
        if (mask == 0) continue;
        uint32_t got[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) got[i] = gload<uint8_t>(uintptr_t(addr[i]));
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

// The walk is walk_tiles' (tile_walk.h) over the entries' slot starts:
// pos(0) = 0 and pos(N) = 2^64 - 1 >= any end. A run of equal starts (records
// without a payload) longer than the window is stepped over like a tile that
// starts beyond it; one inside a tile sends the tile to global memory like any
// other tile of more than kCopyStage entries. Staged per entry of a tile: its
// PlRec.
__global__ __launch_bounds__(kPlThreads) void place_copy_kernel(PlaceArgs a) {
    __shared__ uint64_t s_e[kPlThreads / 64][kCopyStage + 1];
    __shared__ uint64_t s_lo[kPlThreads / 64][kCopyStage];
    __shared__ uint64_t s_hi[kPlThreads / 64][kCopyStage];
    __shared__ uint64_t s_a[kPlThreads / 64][kCopyStage];
    __shared__ uint32_t s_x[kPlThreads / 64][kCopyStage];
    __shared__ uint32_t s_v[kPlThreads / 64][kCopyStage];
    __shared__ uint32_t s_r[kPlThreads / 64][kCopyStage];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t N = a.n + 1;                                // entries; entry N (and on) starts at 2^64 - 1
    // dst bytes [0, W) may be written: up to the last record's slice
    const uint64_t W = payload_extent(a.slot_off[a.n - 1], a.pay_len[a.n - 1], a.dst_cap);
    if (W == 0) return;
    const uint64_t D0 = a.origin, D1 = a.origin + W;
    const uint64_t shift = 0 - a.origin;                       // (mod 2^64: D >= origin wherever it is added)
    const uint64_t spare = uint64_t(reinterpret_cast<uintptr_t>(a.slot_off));
    walk_tiles<kPlTile>(
        PlEntries{a}, N, D0, D1, shift, s_e[wv],
        [&](const uint64_t* e, uint64_t j0, uint32_t n, uint64_t t0, uint64_t, uint64_t) {
            for (uint32_t i = lane; i < n; i += 64) {
                const PlRec s = pl_rec(a, j0 + i);
                s_lo[wv][i] = s.lo;
                s_hi[wv][i] = s.hi;
                s_a[wv][i] = s.addr0;
                s_x[wv][i] = s.x0;
                s_v[wv][i] = s.vlen;
                s_r[wv][i] = s.room0;
            }
            wave_stage_done();
            pl_copy_tile(a, PlStaged{e, s_lo[wv], s_hi[wv], s_a[wv], s_x[wv], s_v[wv], s_r[wv]}, n, shift, spare,
                         a.out, t0, D0, D1, lane);
        },
        [&](uint64_t j0, uint64_t n, uint64_t t0, uint64_t, uint64_t) {
            pl_copy_tile(a, PlGlobal{a, j0}, n, shift, spare, a.out, t0, D0, D1, lane);
        });
}

static uint32_t pl_blocks(uint64_t n) { return uint32_t((n + kPlThreads - 1) / kPlThreads); }

hipError_t launch_pay_blk(const PaySlotsArgs& a, hipStream_t s) {
    ONC_LAUNCH(pay_blk_kernel, dim3(pl_blocks(a.n)), dim3(kPlThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pay_blkscan(const PaySlotsArgs& a, hipStream_t s) {
    ONC_LAUNCH(pay_blkscan_kernel, dim3(1), dim3(kPlThreads), 0, s, a, uint64_t(pl_blocks(a.n)));
    return hipGetLastError();
}

hipError_t launch_pay_apply(const PaySlotsArgs& a, hipStream_t s) {
    ONC_LAUNCH(pay_apply_kernel, dim3(pl_blocks(a.n)), dim3(kPlThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pay_empty(const PaySlotsArgs& a, hipStream_t s) {
    ONC_LAUNCH(pay_empty_kernel, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

// The grid covers the capacity (how much of it the slots use is known on the
// device only), up to kPlMaxBlocks workgroups; the kernel deals the tiles out.
hipError_t launch_place_copy(const PlaceArgs& a, hipStream_t s, uint32_t variant) {
    const uint64_t wgs = copy_groups(a.origin, a.dst_cap, kPlTile * (kPlThreads / 64));
    const uint64_t most = copy_max_groups(variant, kPlMaxBlocks);
    ONC_LAUNCH(place_copy_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kPlThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
