// defrag_heads.hip — the heads of fragmented records on gfx950
// (onc_defragment_heads, include/onc_rpc.h): what a decoder needs from a
// reassembled record — its synthesised mark and its first head_len bytes,
// contiguous, and its true length — without moving the payload, which stays
// where it arrived and is described by rec_frag / frag_pre.
//
// The plan is onc_defragment_extents' (defrag.hip): defrag_blk<true>,
// defrag_blkscan and defrag_frag<true> give every fragment its record index
// (S), the body bytes before it in its record (written straight into the
// caller's frag_pre) and first-of-record (M), and every record its length.
// Slots have a fixed stride, so there is no placement scan. Then:
//
//   heads_place   rec_len, status (the capacity cut is by record index),
//                 rec_frag (a record's first fragment stores its own index),
//                 result
//   heads_gather  the hot path, partitioned by output: a lane owns one
//                 16-byte chunk of one slot. The fragment holding the chunk's
//                 first body byte is found by binary search of frag_pre
//                 inside the record's fragments (a head may be spread over
//                 any number of fragments, runs of empty ones included); a
//                 chunk inside one fragment's body is one unaligned 16-byte
//                 load and one aligned 16-byte store — the first chunk too,
//                 loaded from the fragment's own mark on and its first word
//                 replaced by the record's mark; byte by byte at seams and at
//                 the record's end. No LDS and no barrier: a lane that has
//                 nothing to write just takes its next chunk.
#include "common.h"
#include "defrag_heads_plan.h"
#include "kernels.h"

namespace onc {

constexpr int kDhThreads = 256;
constexpr uint64_t kDhMaxBlocks = 1ull << 16;   // heads_gather workgroups (the chunks are dealt out among them)

__global__ __launch_bounds__(kDhThreads) void heads_empty_kernel(HeadsArgs a) {
    if (threadIdx.x == 0) a.rec_frag[0] = 0;
    if (threadIdx.x < 6) a.result[threadIdx.x] = 0;
}

// Thread i: fragment i (its record's rec_frag entry when it is the first),
// record i (rec_len, status), and for i == 0 the result.
__global__ __launch_bounds__(kDhThreads) void heads_place_kernel(HeadsArgs a) {
    const uint64_t i = uint64_t(blockIdx.x) * kDhThreads + threadIdx.x;
    if (i > a.nfrag) return;
    const DefragAgg all = a.blk[(a.nfrag + kDhThreads - 1) / kDhThreads];
    const uint64_t nrec = all.lasts;
    if (i < a.nfrag && a.M[i] != 0) {
        const uint64_t r = a.S[i];
        if (r < nrec) a.rec_frag[r] = i;
    }
    if (i == a.nfrag) a.rec_frag[nrec] = a.nfrag - all.cnt;     // the first pending fragment, or nfrag
    if (i < nrec) {
        const uint32_t len = a.lens[i];
        a.rec_len[i] = len;
        a.status[i] = heads_status_len(len, i, a.max_records);
    }
    if (i == 0) heads_result(a.result, nrec, a.nfrag, all.cnt, all.tail, a.info[0], a.head_len);
}

__global__ __launch_bounds__(kDhThreads) void heads_gather_kernel(HeadsArgs a) {
    const uint64_t nrec = min(a.result[0], a.max_records);      // records past the capacity have no slot
    const uint32_t H = a.head_len, cpr = H >> 4;
    const uint64_t total = nrec * cpr;
    const uintptr_t wire = reinterpret_cast<uintptr_t>(a.wire);
    const uint64_t stride = uint64_t(gridDim.x) * kDhThreads;
    for (uint64_t c = uint64_t(blockIdx.x) * kDhThreads + threadIdx.x; c < total; c += stride) {
        const uint64_t r = c / cpr;
        const uint32_t b0 = 16u * uint32_t(c - r * cpr);
        const uint32_t len = a.rec_len[r];
        if (len == 0) continue;                                 // ONC_ENC_TOO_LONG: its slot stays as it is
        const uint32_t P = heads_present(len, H);
        if (b0 >= P) continue;
        const uint32_t b1 = min(b0 + 16u, P);
        const uint32_t B = len - 4u;
        const uint32_t mark = defrag_mark(B);
        uint8_t* dst = a.heads + r * H;
        if (b1 <= 4u) {                                         // an empty record: the mark alone
            for (uint32_t p = b0; p < b1; ++p) dst[p] = uint8_t(mark >> (24u - 8u * p));
            continue;
        }
        // body bytes [x0, x1) of the record, x0 < x1 <= B
        const uint32_t x0 = b0 < 4u ? 0u : b0 - 4u, x1 = b1 - 4u;
        const uint64_t hi = a.rec_frag[r + 1];
        uint64_t j = heads_frag_of(a.frag_pre, a.rec_frag[r], hi, x0);
        uint64_t pre = a.frag_pre[j];
        uint64_t end = j + 1 < hi ? a.frag_pre[j + 1] : B;      // where fragment j's body ends in the record's
        if (b1 - b0 == 16u && end >= x1) {
            // the chunk lies inside fragment j (the first chunk: from the
            // fragment's own mark on, pre == 0 there)
            uint32_t v[4];
            load16_unaligned(wire + a.frag_start[j] + (x0 - pre) + (b0 == 0 ? 0u : 4u), v);
            if (b0 == 0) v[0] = bswap(mark);
            *reinterpret_cast<uint4*>(dst + b0) = make_uint4(v[0], v[1], v[2], v[3]);
            continue;
        }
        // a seam or the record's end: byte by byte
        uintptr_t src = wire + a.frag_start[j] + 4u;
        for (uint32_t p = b0; p < b1; ++p) {
            if (p < 4u) {
                dst[p] = uint8_t(mark >> (24u - 8u * p));
                continue;
            }
            const uint32_t x = p - 4u;
            if (x >= end) {                                     // the next fragment that is not empty
                j = heads_frag_of(a.frag_pre, j, hi, x);
                pre = a.frag_pre[j];
                end = j + 1 < hi ? a.frag_pre[j + 1] : B;
                src = wire + a.frag_start[j] + 4u;
            }
            dst[p] = gload<uint8_t>(src + (x - pre));
        }
    }
}

static uint32_t dh_blocks(uint64_t n) { return uint32_t((n + kDhThreads - 1) / kDhThreads); }

hipError_t launch_heads_empty(const HeadsArgs& a, hipStream_t s) {
    ONC_LAUNCH(heads_empty_kernel, dim3(1), dim3(kDhThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_heads_place(const HeadsArgs& a, hipStream_t s) {
    ONC_LAUNCH(heads_place_kernel, dim3(dh_blocks(a.nfrag + 1)), dim3(kDhThreads), 0, s, a);
    return hipGetLastError();
}

// The grid covers the slots there can be (how many records the fragments
// close is known on the device only), up to kDhMaxBlocks workgroups.
hipError_t launch_heads_gather(const HeadsArgs& a, hipStream_t s, uint32_t variant) {
    const uint64_t slots = a.nfrag < a.max_records ? a.nfrag : a.max_records;
    const uint64_t wgs = (slots * (a.head_len >> 4) + kDhThreads - 1) / kDhThreads;
    const uint64_t most = copy_max_groups(variant, kDhMaxBlocks);
    ONC_LAUNCH(heads_gather_kernel, dim3(uint32_t(wgs < most ? wgs : most)), dim3(kDhThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace onc
