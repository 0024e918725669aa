// streams.hip — segmented framing on gfx950 (onc_frame_streams): many
// connections' receive buffers framed in one call.
//
// The reference anchor is the caller's loop of expected_message_len
// (src/rpc_message.rs:343-367) + one-message slices (rpc_message.rs:238-242),
// run once per connection. A segment's first byte is a certain record start,
// so none of frame.hip's speculation is needed (no guess, no verification, no
// walk); what is parallel here is the segments:
//
//   streams_chase  lane per segment: the exact chain from the segment's start
//                  to its end or to where it stops (frame.hip's chase<false>
//                  loop, over the segment instead of a chunk, and without a
//                  capacity: max_records does not enter it). Keeps the count,
//                  the stop and the first kStreamKeep record lengths — in LDS
//                  columns during the chase and copied out after it: a global
//                  store inside the chase would hold up the next hop's load
//                  (frame_chunks' note).
//   onc_scan_lengths  of the counts: every segment's first record index with
//                  unbounded capacity, and their total (`needed`).
//   streams_write  kStreamKeep lanes per segment: rec_start / rec_len /
//                  rec_seg and the segment's row, cut at max_records. A
//                  segment whose lengths were all kept is written from them
//                  (a 16-lane prefix sum, coalesced stores, no wire read);
//                  a longer one is chased again by its first lane, kStreamKeep
//                  hops at a time into LDS, the 16 lanes then writing those
//                  records together — again no store between two hops.
//   streams_result one workgroup: the stopped segments summed over the write
//                  workgroups, and `result`. (A ticket — the last write
//                  workgroup to finish sums up — cost more than the write
//                  itself: 29k workgroups' atomics on one word took 800 us
//                  at 470k segments, profiles/frame_streams_timing.log.)
//
// A lane follows its segment serially, however long it is: the design point
// is many segments of up to about a frame chunk each (onc_frame_stream is the
// call for one long stream).
//
// onc_frame_fragment_streams is the same machine at fragment level (RFC 5531
// §11: every mark starts a fragment, bit 31 ends a record), in kernels of its
// own below — fragstreams_chase / _write / _result — so that the ones above
// stay as they are: the chase keeps the mark words (bit 31 is needed, and a
// length can take 32 bits) and commits at every last fragment; two scans
// (fragments, records); the write pass emits whole records only.
#include "common.h"
#include "kernels.h"

namespace onc {

constexpr int kStreamsWG = 64;                   // segments (lanes) per streams_chase workgroup
constexpr int kKeepStride = kStreamsWG + 1;      // LDS column stride (the copy-out reads it transposed)
constexpr int kWriteWG = 256;
constexpr int kWriteSegs = kWriteWG / int(kStreamKeep);   // segments per streams_write workgroup

__device__ __forceinline__ uint32_t mark_at(uintptr_t seg, uint64_t p) { return bswap(load4(seg + p)); }

__global__ __launch_bounds__(kStreamsWG) void streams_chase_kernel(StreamsArgs a) {
    __shared__ uint32_t s_keep[kStreamKeep * kKeepStride];
    const int t = threadIdx.x;
    const uint64_t s0 = uint64_t(blockIdx.x) * kStreamsWG;
    const uint64_t s = s0 + t;
    if (s < a.nseg) {
        const uint64_t len = a.seg_len[s];
        const uintptr_t seg = reinterpret_cast<uintptr_t>(a.wire) + a.seg_off[s];
        uint64_t p = 0;
        uint32_t cnt = 0, aux0 = 0, aux1 = 0;
        int32_t st = ONC_OK;
        while (p < len) {
            const uint64_t left = len - p;
            if (left < 4) {                            // expected_message_len: rpc_message.rs:344-346
                st = ONC_ERR_INCOMPLETE_HEADER;
                break;
            }
            const uint32_t h = mark_at(seg, p);
            if ((h & 0x80000000u) == 0) {              // :359-362
                st = ONC_ERR_FRAGMENTED;
                break;
            }
            const uint64_t want = uint64_t(h & 0x7FFFFFFFu) + 4;
            if (left < want) {                         // the one-message slice would be short
                st = ONC_ERR_INCOMPLETE_MESSAGE;
                aux0 = uint32_t(left);
                aux1 = uint32_t(want);
                break;
            }
            if (cnt < kStreamKeep) s_keep[cnt * kKeepStride + t] = uint32_t(want);
            ++cnt;                                     // (seg_len < 2^34: fewer than 2^32 records)
            p += want;
        }
        a.x[s] = p;
        a.cnt[s] = cnt;
        a.st[s] = st;
        a.aux[2 * s] = aux0;
        a.aux[2 * s + 1] = aux1;
    }
    __syncthreads();
    // the kept lengths, copied out as whole lines: entry i of segment s0 + l
    // at keep[(s0 + l) * kStreamKeep + i] (entries at or past a segment's
    // count are never read)
    const uint64_t lim = (a.nseg - s0 < uint64_t(kStreamsWG) ? a.nseg - s0 : uint64_t(kStreamsWG)) * kStreamKeep;
    uint32_t* dst = a.keep + s0 * kStreamKeep;
#pragma unroll
    for (uint32_t r = 0; r < kStreamKeep; ++r) {
        const uint32_t q = r * kStreamsWG + uint32_t(t);
        if (q < lim) dst[q] = s_keep[(q % kStreamKeep) * kKeepStride + q / kStreamKeep];
    }
}

// Inclusive prefix sum over the kStreamKeep lanes of a segment's group.
__device__ __forceinline__ uint64_t group_incl_scan(uint64_t v, uint32_t j) {
#pragma unroll
    for (uint32_t o = 1; o < kStreamKeep; o <<= 1) {
        const uint64_t w = __shfl_up(static_cast<unsigned long long>(v), o, int(kStreamKeep));
        if (j >= o) v += w;
    }
    return v;
}

__device__ __forceinline__ void put_record(const StreamsArgs& a, uint64_t k, uint64_t start, uint32_t len, uint64_t s) {
    a.rec_start[k] = start;
    a.rec_len[k] = len;
    if (a.rec_seg) a.rec_seg[k] = uint32_t(s);
}

__device__ __forceinline__ void lds_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kWriteWG) void streams_write_kernel(StreamsArgs a) {
    static_assert(kStreamKeep == 16 && 64 % kStreamKeep == 0, "a segment's lanes lie in one wave; rows take 6 of them");
    __shared__ uint32_t s_len[kWriteSegs * kStreamKeep];
    __shared__ uint32_t s_stopped;
    const uint32_t g = threadIdx.x / kStreamKeep, j = threadIdx.x % kStreamKeep;
    const uint64_t s = uint64_t(blockIdx.x) * kWriteSegs + g;
    if (threadIdx.x == 0) s_stopped = 0;
    __syncthreads();
    if (s < a.nseg) {
        // (every value below is the same in the segment's 16 lanes)
        const uint64_t first_u = a.base[s];            // first record index with unbounded capacity
        const uint32_t cnt = a.cnt[s];
        // the caller's loop never looks at a segment once max_records is reached
        uint64_t first = a.max_records, n = 0, consumed = 0, st = 0, aux0 = 0, aux1 = 0;
        if (first_u < a.max_records) {
            const uint64_t room = a.max_records - first_u;
            const bool whole = cnt < room;             // the loop went on to see why the segment ends
            const uint32_t ce = whole ? cnt : uint32_t(room);
            const uint64_t off = a.seg_off[s];
            uint64_t p = 0;
            if (cnt <= kStreamKeep) {
                const uint64_t l = j < cnt ? a.keep[s * kStreamKeep + j] : 0u;
                const uint64_t incl = group_incl_scan(l, j);
                if (j < ce) put_record(a, first_u + j, off + incl - l, uint32_t(l), s);
                // the start of record ce (ce < cnt <= 16), or the chain's stop
                const uint64_t at_ce = __shfl(static_cast<unsigned long long>(incl - l), int(ce % kStreamKeep),
                                              int(kStreamKeep));
                p = ce == cnt ? a.x[s] : at_ce;
            } else {
                // the chain again, kStreamKeep hops at a time. The marks were
                // checked by streams_chase; a hop is still kept inside the
                // segment (a wire changed under the call must not turn into a
                // read outside it).
                const uint64_t len = a.seg_len[s];
                const uintptr_t seg = reinterpret_cast<uintptr_t>(a.wire) + off;
                uint32_t* mine = &s_len[g * kStreamKeep];
                for (uint32_t done = 0; done < ce; done += kStreamKeep) {
                    const uint32_t nb = ce - done < kStreamKeep ? ce - done : kStreamKeep;
                    if (j == 0) {
                        uint64_t q = p;
                        for (uint32_t i = 0; i < nb; ++i) {
                            const uint64_t want = len - q >= 4 ? uint64_t(mark_at(seg, q) & 0x7FFFFFFFu) + 4 : len - q;
                            mine[i] = uint32_t(want);
                            q = want < len - q ? q + want : len;
                        }
                    }
                    lds_wave_sync();
                    const uint64_t l = j < nb ? mine[j] : 0u;
                    const uint64_t incl = group_incl_scan(l, j);
                    if (j < nb) put_record(a, first_u + done + j, off + p + incl - l, uint32_t(l), s);
                    p += __shfl(static_cast<unsigned long long>(incl), int(kStreamKeep) - 1, int(kStreamKeep));
                    lds_wave_sync();                   // the next round overwrites the lengths
                }
            }
            first = first_u;
            n = ce;
            consumed = p;
            if (whole) {
                st = uint64_t(int64_t(a.st[s]));
                aux0 = a.aux[2 * s];
                aux1 = a.aux[2 * s + 1];
            }
        }
        if (j < 6) {
            const uint64_t v = j == 0 ? first : j == 1 ? n : j == 2 ? consumed : j == 3 ? st : j == 4 ? aux0 : aux1;
            a.seg_result[6 * s + j] = v;
        }
        if (j == 0 && st != 0) atomicAdd(&s_stopped, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) a.blk_stopped[blockIdx.x] = s_stopped;
}

// The write workgroups' counts summed by one workgroup of kResultWG threads.
constexpr int kResultWG = 1024;
__device__ __forceinline__ uint64_t sum_blk_stopped(const uint32_t* blk_stopped, uint64_t nblk, uint64_t* s_wave) {
    uint64_t v = 0;
    // eight loads in flight per thread (one at a time took 29 us for 29k counts)
    for (uint64_t i0 = threadIdx.x; i0 < nblk; i0 += 8ull * kResultWG) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint64_t i = i0 + uint64_t(k) * kResultWG;
            w[k] = blk_stopped[i < nblk ? i : i0];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) v += i0 + uint64_t(k) * kResultWG < nblk ? w[k] : 0u;
    }
    return block_sum_u64<kResultWG>(v, s_wave);
}

// result = {framed, needed, segments stopped}
__global__ __launch_bounds__(kResultWG) void streams_result_kernel(StreamsArgs a, uint64_t nblk) {
    __shared__ uint64_t s_wave[kResultWG / 64];
    const uint64_t stopped = sum_blk_stopped(a.blk_stopped, nblk, s_wave);
    if (threadIdx.x == 0) {
        const uint64_t needed = a.base[a.nseg];
        a.result[0] = needed < a.max_records ? needed : a.max_records;
        a.result[1] = needed;
        a.result[2] = stopped;
    }
}

hipError_t launch_streams_chase(const StreamsArgs& a, hipStream_t s) {
    const uint32_t blocks = uint32_t((a.nseg + kStreamsWG - 1) / kStreamsWG);
    ONC_LAUNCH(streams_chase_kernel, dim3(blocks), dim3(kStreamsWG), 0, s, a);
    return hipGetLastError();
}

uint64_t streams_write_groups(uint64_t nseg) { return (nseg + kWriteSegs - 1) / kWriteSegs; }

hipError_t launch_streams_result(const StreamsArgs& a, hipStream_t s) {
    ONC_LAUNCH(streams_result_kernel, dim3(1), dim3(kResultWG), 0, s, a, streams_write_groups(a.nseg));
    return hipGetLastError();
}

hipError_t launch_streams_write(const StreamsArgs& a, hipStream_t s) {
    const uint32_t blocks = uint32_t(streams_write_groups(a.nseg));
    ONC_LAUNCH(streams_write_kernel, dim3(blocks), dim3(kWriteWG), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// onc_frame_fragment_streams
// ---------------------------------------------------------------------------

// streams_chase at fragment level: the walk goes on through marks without the
// last-fragment bit, and what it has walked is committed — fragments, records,
// the position — whenever a mark has it, so that a pending run at the
// segment's end (its last fragment has not arrived, or a stop cut it) counts
// for nothing. The commit is three selects: the hop loop has no branch and no
// store that streams_chase's has not.
__global__ __launch_bounds__(kStreamsWG) void fragstreams_chase_kernel(FragStreamsArgs a) {
    __shared__ uint32_t s_keep[kStreamKeep * kKeepStride];
    const int t = threadIdx.x;
    const uint64_t s0 = uint64_t(blockIdx.x) * kStreamsWG;
    const uint64_t s = s0 + t;
    if (s < a.nseg) {
        const uint64_t len = a.seg_len[s];
        const uintptr_t seg = reinterpret_cast<uintptr_t>(a.wire) + a.seg_off[s];
        uint64_t p = 0, x = 0;
        uint32_t cnt = 0, fcnt = 0, rcnt = 0, aux0 = 0, aux1 = 0;
        int32_t st = ONC_OK;
        while (p < len) {
            const uint64_t left = len - p;
            if (left < 4) {
                st = ONC_ERR_INCOMPLETE_HEADER;
                break;
            }
            const uint32_t h = mark_at(seg, p);
            const uint64_t want = uint64_t(h & 0x7FFFFFFFu) + 4;
            if (left < want) {
                st = ONC_ERR_INCOMPLETE_MESSAGE;
                aux0 = uint32_t(left);
                aux1 = uint32_t(want);
                break;
            }
            if (cnt < kStreamKeep) s_keep[cnt * kKeepStride + t] = h;   // the word: `want` can take 32 bits
            ++cnt;                                     // (seg_len < 2^34: fewer than 2^32 fragments)
            p += want;
            const bool last = (h & 0x80000000u) != 0;
            fcnt = last ? cnt : fcnt;
            rcnt += last ? 1u : 0u;
            x = last ? p : x;
        }
        a.x[s] = x;
        a.fcnt[s] = fcnt;
        a.rcnt[s] = rcnt;
        a.st[s] = st;
        a.aux[2 * s] = aux0;
        a.aux[2 * s + 1] = aux1;
    }
    __syncthreads();
    // the kept marks, copied out as whole lines (as streams_chase's lengths);
    // the first fcnt <= cnt of a segment's entries are the ones read later
    const uint64_t lim = (a.nseg - s0 < uint64_t(kStreamsWG) ? a.nseg - s0 : uint64_t(kStreamsWG)) * kStreamKeep;
    uint32_t* dst = a.keep + s0 * kStreamKeep;
#pragma unroll
    for (uint32_t r = 0; r < kStreamKeep; ++r) {
        const uint32_t q = r * kStreamsWG + uint32_t(t);
        if (q < lim) dst[q] = s_keep[(q % kStreamKeep) * kKeepStride + q / kStreamKeep];
    }
}

__device__ __forceinline__ void put_fragment(const FragStreamsArgs& a, uint64_t k, uint64_t start, uint32_t len,
                                             uint64_t s) {
    a.frag_start[k] = start;
    a.frag_len[k] = len;
    if (a.frag_seg) a.frag_seg[k] = uint32_t(s);
}

// A mark of segment [seg, seg + len) at q, as the write pass follows a chain
// again: streams_chase checked it, and the hop is still kept inside the
// segment (streams_write's note). *q moves past the fragment.
__device__ __forceinline__ uint32_t rehop(uintptr_t seg, uint64_t len, uint64_t* q) {
    const uint64_t left = len - *q;
    const uint32_t h = left >= 4 ? mark_at(seg, *q) : 0u;
    const uint64_t want = left >= 4 ? uint64_t(h & 0x7FFFFFFFu) + 4 : left;
    *q = want < left ? *q + want : len;
    return h;
}

// streams_write at fragment level. fbase[s] = the fragments before segment s
// with unbounded capacity, so (fbase only grows) the segments with
// fbase[s + 1] <= max_frags are emitted whole, the one with fbase[s] <=
// max_frags < fbase[s + 1] is cut — it emits its records while they fit
// whole — and every later one has fbase[s] > max_frags: the caller's loop
// never looked at it.
__global__ __launch_bounds__(kWriteWG) void fragstreams_write_kernel(FragStreamsArgs a) {
    static_assert(kStreamKeep == 16 && 64 % kStreamKeep == 0, "a segment's lanes lie in one wave; rows take 8 of them");
    __shared__ uint32_t s_mark[kWriteSegs * kStreamKeep];
    __shared__ uint32_t s_stopped;
    const uint32_t g = threadIdx.x / kStreamKeep, j = threadIdx.x % kStreamKeep;
    const uint64_t s = uint64_t(blockIdx.x) * kWriteSegs + g;
    if (threadIdx.x == 0) s_stopped = 0;
    __syncthreads();
    if (s < a.nseg) {
        // (every value below is the same in the segment's 16 lanes)
        const uint64_t first_u = a.fbase[s];
        const uint32_t cnt = a.fcnt[s];                // fragments of its complete records
        uint64_t first = a.max_frags, n = 0, consumed = 0, st = 0, aux0 = 0, aux1 = 0, first_rec = 0, n_rec = 0;
        if (first_u <= a.max_frags) {
            const uint64_t room = a.max_frags - first_u;
            const bool whole = cnt <= room;
            const uint64_t off = a.seg_off[s];
            uint32_t ce = cnt, nr = a.rcnt[s];         // fragments and records emitted
            uint64_t p = 0;
            if (cnt <= kStreamKeep) {
                // every fragment to emit was kept (a pending run past them may not have been: it is not read)
                const uint32_t h = j < cnt ? a.keep[s * kStreamKeep + j] : 0u;
                const uint64_t l = j < cnt ? uint64_t(h & 0x7FFFFFFFu) + 4 : 0u;
                const uint64_t incl = group_incl_scan(l, j);
                p = a.x[s];
                if (!whole) {
                    // the last fragments among the first `room` (< cnt <= 16): the records that fit
                    const uint64_t b = __ballot(j < room && (h & 0x80000000u) != 0);
                    const uint32_t lasts = uint32_t(b >> (threadIdx.x & 63u & ~(kStreamKeep - 1u))) & 0xFFFFu;
                    ce = lasts ? 32u - uint32_t(__clz(int(lasts))) : 0u;
                    nr = uint32_t(__popc(lasts));
                    // the end of fragment ce - 1
                    const uint64_t end = __shfl(static_cast<unsigned long long>(incl), int((ce + kStreamKeep - 1) % kStreamKeep),
                                                int(kStreamKeep));
                    p = ce ? end : 0;
                }
                if (j < ce) put_fragment(a, first_u + j, off + incl - l, uint32_t(l), s);
            } else {
                const uint64_t len = a.seg_len[s];
                const uintptr_t seg = reinterpret_cast<uintptr_t>(a.wire) + off;
                if (!whole) {
                    // the one segment of a call that the capacity cuts: how far
                    // its whole records go within the room, by a chain of its own
                    // (the same in all 16 lanes)
                    ce = 0;
                    nr = 0;
                    uint64_t q = 0;
                    for (uint32_t i = 0; i < uint32_t(room); ++i) {   // room < cnt
                        const bool last = (rehop(seg, len, &q) & 0x80000000u) != 0;
                        ce = last ? i + 1 : ce;
                        nr += last ? 1u : 0u;
                    }
                }
                // the chain again, kStreamKeep hops at a time (streams_write)
                uint32_t* mine = &s_mark[g * kStreamKeep];
                for (uint32_t done = 0; done < ce; done += kStreamKeep) {
                    const uint32_t nb = ce - done < kStreamKeep ? ce - done : kStreamKeep;
                    if (j == 0) {
                        uint64_t q = p;
                        for (uint32_t i = 0; i < nb; ++i) {
                            const uint64_t q0 = q;
                            (void)rehop(seg, len, &q);
                            mine[i] = uint32_t(q - q0);    // < 2^32: inside the segment
                        }
                    }
                    lds_wave_sync();
                    const uint64_t l = j < nb ? mine[j] : 0u;
                    const uint64_t incl = group_incl_scan(l, j);
                    if (j < nb) put_fragment(a, first_u + done + j, off + p + incl - l, uint32_t(l), s);
                    p += __shfl(static_cast<unsigned long long>(incl), int(kStreamKeep) - 1, int(kStreamKeep));
                    lds_wave_sync();                   // the next round overwrites the lengths
                }
            }
            first = first_u;
            n = ce;
            consumed = p;
            first_rec = a.rbase[s];
            n_rec = nr;
            if (whole) {
                st = uint64_t(int64_t(a.st[s]));
                aux0 = a.aux[2 * s];
                aux1 = a.aux[2 * s + 1];
            } else if (j == 0) {
                a.cut[0] = first_u + ce;
                a.cut[1] = first_rec + nr;
            }
        }
        if (j < 8) {
            const uint64_t v = j == 0 ? first : j == 1 ? n : j == 2 ? consumed : j == 3 ? st : j == 4 ? aux0
                             : j == 5 ? aux1 : j == 6 ? first_rec : n_rec;
            a.seg_result[8 * s + j] = v;
        }
        if (j == 0 && st != 0) atomicAdd(&s_stopped, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) a.blk_stopped[blockIdx.x] = s_stopped;
}

// result = {fragments emitted, needed, records emitted, segments stopped}
__global__ __launch_bounds__(kResultWG) void fragstreams_result_kernel(FragStreamsArgs a, uint64_t nblk) {
    __shared__ uint64_t s_wave[kResultWG / 64];
    const uint64_t stopped = sum_blk_stopped(a.blk_stopped, nblk, s_wave);
    if (threadIdx.x == 0) {
        const uint64_t needed = a.fbase[a.nseg];
        const bool cut = needed > a.max_frags;         // then, and only then, a segment was cut and wrote a.cut
        a.result[0] = cut ? a.cut[0] : needed;
        a.result[1] = needed;
        a.result[2] = cut ? a.cut[1] : a.rbase[a.nseg];
        a.result[3] = stopped;
    }
}

hipError_t launch_fragstreams_chase(const FragStreamsArgs& a, hipStream_t s) {
    const uint32_t blocks = uint32_t((a.nseg + kStreamsWG - 1) / kStreamsWG);
    ONC_LAUNCH(fragstreams_chase_kernel, dim3(blocks), dim3(kStreamsWG), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fragstreams_write(const FragStreamsArgs& a, hipStream_t s) {
    const uint32_t blocks = uint32_t(streams_write_groups(a.nseg));
    ONC_LAUNCH(fragstreams_write_kernel, dim3(blocks), dim3(kWriteWG), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fragstreams_result(const FragStreamsArgs& a, hipStream_t s) {
    ONC_LAUNCH(fragstreams_result_kernel, dim3(1), dim3(kResultWG), 0, s, a, streams_write_groups(a.nseg));
    return hipGetLastError();
}

}  // namespace onc
