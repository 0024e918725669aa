// xdr.hip — Call arguments decoded into columns on gfx950 (onc_xdr_unpack,
// include/onc_rpc.h): every payload of a slice of descriptors parsed against
// one flat XDR schema, a column per field.
//
//   xdr_unpack   a workgroup per tile of kXdrTile records, a lane per record.
//                The schema travels by value in the kernel arguments, so the
//                loop over its fields (xdr_plan.h xdr_parse) is wave-uniform:
//                the field is read with scalar loads, the branches on its type
//                and flags are uniform, and only the IF test and the failures
//                diverge. A lane loads its status and, for an OK record only,
//                the descriptor's first two 16-byte granules (kinds |
//                payload_len, payload_off). Wire bytes come as whole aligned
//                16-byte granules that hold a byte of the payload inside the
//                readable window: the granules as far as the schema's word
//                reads can reach (xdr_reach; at most kXdrPre) are issued
//                together before the parse, the rest on demand, one cached. A word at any byte address is put
//                together from one or two granules (v_alignbyte). Nothing is
//                read for a record that is SKIPPED or BAD_EXTENT, and of an
//                opaque or array body only what shares those first granules
//                with the words. A column store writes the records of
//                consecutive lanes to consecutive addresses. The tile's
//                records per outcome class are counted with ballots and go to
//                the scratch.
//   xdr_result   one workgroup: the tiles' counts summed into result.
//
// No atomics, and no workgroup waits for another.
#include "common.h"
#include "kernels.h"
#include "xdr_plan.h"

namespace onc {

constexpr int kXdrThreads = int(kXdrTile);
constexpr int kXdrWaves = kXdrThreads / 64;
static_assert(kXdrTile == ONC_XDR_TILE, "the tile the header names");
static_assert(sizeof(onc_xdr_field) == 24, "the schema by value: 1.5 KiB of kernel arguments");
static_assert(offsetof(onc_msg, stat) == 6 && offsetof(onc_msg, payload_len) == 20 &&
                  offsetof(onc_msg, payload_off) == 24,
              "the descriptor words read and the one byte patched");

__device__ __forceinline__ uint32_t xdr_pick(const u32x4& q, uint32_t w) {
    return w == 0 ? q.x : (w == 1 ? q.y : (w == 2 ? q.z : q.w));
}

// The words of one payload. Every granule it loads holds a byte the parse has
// checked to lie inside the payload and the window (xdr_parse reads a word
// only after both tests), or — the ones issued up front — a byte below
// `readable`, the end of that range.
struct XdrReader {
    uintptr_t pay;          // address of payload byte 0
    uintptr_t g0;           // its granule
    u32x4 p0, p1, p2, p3, p4;   // granules g0 + 16 k, k < npre (named, not an array: a select among them
                            // must not become an indexed load from scratch)
    uint32_t npre;
    uintptr_t cg;           // the granule fetched on demand last (0: none)
    u32x4 cq;

    // readable: the payload bytes inside the window; want: how many of them to fetch now
    __device__ __forceinline__ void issue(uintptr_t payload, uint64_t readable, uint32_t want) {
        pay = payload;
        g0 = payload & ~uintptr_t(15);
        cg = 0;
        cq = u32x4{0u, 0u, 0u, 0u};
        const uint64_t bytes = readable < want ? readable : want;
        npre = bytes ? uint32_t((payload + bytes - g0 + 15) >> 4) : 0u;     // (<= kXdrPre: want <= 16 kXdrPre - 15)
        static_assert(kXdrPre == 5, "p0 .. p4");
        p0 = p1 = p2 = p3 = p4 = cq;
        if (npre > 0) p0 = gload<u32x4>(g0);
        if (npre > 1) p1 = gload<u32x4>(g0 + 16);
        if (npre > 2) p2 = gload<u32x4>(g0 + 32);
        if (npre > 3) p3 = gload<u32x4>(g0 + 48);
        if (npre > 4) p4 = gload<u32x4>(g0 + 64);
    }
    __device__ __forceinline__ u32x4 granule(uintptr_t ga) {
        const uint64_t k = (ga - g0) >> 4;
        if (k < npre) {
            // (all four read before the choice: a choice among their addresses would keep them in memory)
            const u32x4 a0 = p0, a1 = p1, a2 = p2, a3 = p3, a4 = p4;
            u32x4 q = a4;
            q = k == 3 ? a3 : q;
            q = k == 2 ? a2 : q;
            q = k == 1 ? a1 : q;
            q = k == 0 ? a0 : q;
            return q;
        }
        if (ga != cg) {
            cq = gload<u32x4>(ga);
            cg = ga;
        }
        return cq;
    }
    __device__ __forceinline__ uint32_t word(uint64_t p) {
        const uintptr_t a = pay + p, ga = a & ~uintptr_t(15);
        const uint32_t w = uint32_t(a & 15) >> 2, b = uint32_t(a & 3);
        const u32x4 q = granule(ga);
        const uint32_t lo = xdr_pick(q, w);
        if (b == 0) return bswap(lo);
        // (the word's last byte lies in the next granule when w == 3)
        const uint32_t hi = w < 3 ? xdr_pick(q, w + 1) : granule(ga + 16).x;
        return bswap(funnel(lo, hi, b));
    }
};

struct XdrSink {
    uint8_t* cols;
    uint64_t r, n;
    bool active;            // r < n

    __device__ __forceinline__ void put32(const onc_xdr_field& f, uint32_t v) const {
        if (active && xdr_has_column(f.type_flags)) *reinterpret_cast<uint32_t*>(cols + f.col_off + 4ull * r) = v;
    }
    __device__ __forceinline__ void put64(const onc_xdr_field& f, uint64_t v) const {
        if (active && xdr_has_column(f.type_flags)) *reinterpret_cast<uint64_t*>(cols + f.col_off + 8ull * r) = v;
    }
    __device__ __forceinline__ void put_pair(const onc_xdr_field& f, uint32_t pos, uint32_t len) const {
        if (active && xdr_has_column(f.type_flags)) {
            *reinterpret_cast<uint32_t*>(cols + f.col_off + 4ull * r) = pos;
            *reinterpret_cast<uint32_t*>(cols + f.col_off + 4ull * n + 4ull * r) = len;
        }
    }
};

__global__ __launch_bounds__(kXdrThreads) void xdr_unpack_kernel(XdrArgs a) {
    __shared__ uint32_t s_cnt[kXdrWaves][3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t r = uint64_t(blockIdx.x) * kXdrTile + tid;
    const bool active = r < a.n;
    const bool heads = a.rec_start == nullptr && a.head_len != 0;
    uint32_t code = ONC_XDR_SKIPPED, kinds = 0;
    uint64_t o = 0, L = 0;
    XdrExtent e{false, 0, 0};
    if (active) {
        // (the record's start with its status, not behind the descriptor: one round trip fewer)
        const uint64_t start = a.rec_start ? a.rec_start[r] : 0ull;
        const int32_t st = a.status[r];
        if (st == ONC_OK) {
            const uintptr_t m = reinterpret_cast<uintptr_t>(a.msgs + r);
            const u32x4 q0 = gload<u32x4>(m), q1 = gload<u32x4>(m + 16);
            kinds = q0.y;
            if (xdr_carries(st, kinds)) {
                L = q1.y;
                o = uint64_t(q1.z) | (uint64_t(q1.w) << 32);
                e = xdr_extent(o, L, r, heads, a.head_len, a.rec_start != nullptr, start, a.wire_len);
                code = e.bad ? ONC_XDR_BAD_EXTENT : ONC_XDR_OK;
            }
        }
    }
    XdrReader rd;
    {
        // the payload bytes inside the window: all of them, or in the heads form those of the head slot
        uint64_t readable = 0;
        if (code == ONC_XDR_OK) readable = (heads && e.hi - o < L) ? e.hi - o : L;
        rd.issue(reinterpret_cast<uintptr_t>(a.wire) + o, readable, a.pre_bytes);
    }
    const XdrSink sink{a.cols, r, a.n, active};
    const XdrParsed out = xdr_parse(a.fields, a.nf, a.flags, code, o, L, e, heads, rd, sink);
    const bool ok = out.code == ONC_XDR_OK;
    const bool garbage = out.code >= ONC_XDR_SHORT && out.code <= ONC_XDR_TRAILING;
    if (active) {
        a.xstat[r] = out.code | (out.fail << 8);
        if (a.present) a.present[r] = out.present;
        if (a.rest_pos) {
            a.rest_pos[r] = ok ? uint32_t(e.base + out.p) : 0u;
            a.rest_len[r] = ok ? uint32_t(L - out.p) : 0u;
        }
        if (a.replies && garbage && (kinds & 0xFFu) == ONC_MSG_CALL)
            reinterpret_cast<uint8_t*>(a.replies + r)[offsetof(onc_msg, stat)] = uint8_t(ONC_ACCEPT_GARBAGE_ARGS);
    }
    const uint32_t n_ok = uint32_t(__popcll(__ballot(active && ok)));
    const uint32_t n_garbage = uint32_t(__popcll(__ballot(active && garbage)));
    const uint32_t n_other = uint32_t(__popcll(__ballot(active && !ok && !garbage)));
    if (lane == 0) {
        s_cnt[wave][0] = n_ok;
        s_cnt[wave][1] = n_garbage;
        s_cnt[wave][2] = n_other;
    }
    __syncthreads();
    if (tid < 3) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < kXdrWaves; ++w) c += s_cnt[w][tid];
        a.counts[3ull * blockIdx.x + tid] = c;
    }
}

// result = {OK, codes 3..6, every other code, 0}
__global__ __launch_bounds__(kXdrThreads) void xdr_result_kernel(const uint32_t* counts, uint64_t tiles,
                                                                 uint64_t* result) {
    __shared__ uint64_t s_wave[kXdrWaves];
    uint64_t sum[3] = {0, 0, 0};
    for (uint64_t t = threadIdx.x; t < tiles; t += kXdrThreads)
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += counts[3ull * t + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t total = block_sum_u64<kXdrThreads>(sum[k], s_wave);
        if (threadIdx.x == 0) result[k] = total;
    }
    if (threadIdx.x == 0) result[3] = 0;
}

hipError_t launch_xdr_unpack(const XdrArgs& a, hipStream_t s) {
    ONC_LAUNCH(xdr_unpack_kernel, dim3(uint32_t(a.tiles)), dim3(kXdrThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_xdr_result(const XdrArgs& a, hipStream_t s) {
    ONC_LAUNCH(xdr_result_kernel, dim3(1), dim3(kXdrThreads), 0, s, a.counts, a.tiles, a.result);
    return hipGetLastError();
}

}  // namespace onc
