// kernels.h — host-side launchers of the gfx950 kernels (internal to the
// shared library; the public surface is include/onc_rpc.h).
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/onc_rpc.h"
#include "common.h"
#include "defrag_heads_plan.h"
#include "defrag_plan.h"
#include "fragment_iov_plan.h"
#include "fragment_plan.h"
#include "gather_plan.h"
#include "group_plan.h"
#include "match_plan.h"
#include "payload_plan.h"
#include "route_plan.h"
#include "xdr_plan.h"

namespace onc {

// Per-kernel timing (onc_codec_enable_timing): codec.hip's run() hands the
// start/stop events to the next launch, which then goes through
// hipExtLaunchKernelGGL — the events take the dispatch packet's own
// timestamps instead of marker packets recorded around it (each marker
// pair serialised the stream: ~7 us per timed launch on gfx950).
struct LaunchEvents {
    hipEvent_t start, stop;
};
extern thread_local LaunchEvents t_launch_events;
inline LaunchEvents take_launch_events() {
    const LaunchEvents e = t_launch_events;
    t_launch_events = LaunchEvents{nullptr, nullptr};
    return e;
}
#define ONC_LAUNCH(K, G, B, L, S, ...)                                                               \
    do {                                                                                             \
        const ::onc::LaunchEvents ev_ = ::onc::take_launch_events();                                 \
        if (ev_.start)                                                                               \
            hipExtLaunchKernelGGL(K, G, B, L, S, ev_.start, ev_.stop, 0, __VA_ARGS__);               \
        else                                                                                         \
            hipLaunchKernelGGL(K, G, B, L, S, __VA_ARGS__);                                          \
    } while (0)

struct EncArgs {
    uint64_t n;
    const onc_msg* msgs;
    const onc_unix_params* unix;
    const uint8_t* auth_arena;
    const uint8_t* payload_arena;
    Bounds bounds;          // arena sizes (onc_batch)
    uint8_t* out;           // 16-byte aligned base of the output chunks
    uint64_t origin;        // byte offset of the caller's `out` from `out` here (0..15)
    uint64_t out_cap;       // origin + the caller's capacity
    uint64_t* rec_off;      // n + 1
    int32_t* status;        // n
    uint32_t* rec_len;      // n, optional
    uint32_t* len_out;      // enc_len: optional codec-owned copy of the lengths (what the emit reads back)
    uint64_t* tile_sum;     // tiles
    uint64_t* block_sum;    // enc_len workgroups (kLenRecs records): byte totals
    uint64_t* block_base;   // exclusive scan of block_sum (unused when fused_base)
    uint64_t* block_pay;    // optional: enc_len workgroups' streamed payload bytes (the wave-specialised
                            // enc_emit's header-heavy test); NULL = not computed
    uint32_t fused_base;    // enc_emit sums block_sum itself (<= kFusedBlocks workgroups; no scan launch)
    uint32_t variant;       // ONC_VARIANT_* bits (onc_codec_options; A/B experiments, tests)
    uint32_t ws;            // enc_emit: the wave-specialised kernel (codec.hip enc_args decides)
    uint32_t root;          // ONC_ROOT_* (onc_encode_body); ONC_ROOT_RPC_MESSAGE for onc_encode
    uint32_t decl;          // enc_len, RpcMessage root: 1 = an emit's plan (declared AUTH_UNIX lengths taken
                            // as given, the emit runs the deferred parameter-block checks); 2 = onc_encode_lengths
                            // (the same extents, every check up front for the statuses); 0 = every check (roots)
    const uint64_t* base_dev;   // optional: output bytes before this launch's first record (chunked encode)
    const uint32_t* len_in;     // optional (wave-per-tile enc_emit): the plan's record lengths, read instead
                                // of re-planning (no dependent AUTH_UNIX parameter load in the prologue)
    uint32_t small;             // the one-launch small batch (enc_emit_single_kernel: one workgroup, the
                                // tiles planned and placed inside it; <= kSpWaves tiles)
#ifdef ONC_EMIT_PROF
    uint64_t* prof;         // lab builds only (tools/emit_prof.hip): per-tile phase timestamps
#endif
};

// Batches of at most this many enc_len workgroups (1M records) skip the
// scan launch: every enc_emit wave sums the block totals before its own
// (16 coalesced u64 loads per lane, issued with its tile-total load).
constexpr uint64_t kFusedBlocks = 1024;

struct IovArgs {
    uint64_t n;
    // (extents follow the declared AUTH_UNIX lengths as onc_encode places them; a record failing only a
    // deferred block check takes its extent with the placeholder header, include/onc_rpc.h onc_auth)
    const onc_msg* msgs;
    const onc_unix_params* unix;
    const uint8_t* auth_arena;
    const uint8_t* payload_arena;
    Bounds bounds;
    uint8_t* hdr_out;
    uint64_t hdr_cap;
    onc_iov_rec* iov;
    int32_t* status;
    uint64_t* totals;          // optional [2]
    uint64_t* tile_sum;        // per 64 records: (wire bytes << 16) | header bytes
    uint64_t* block_len;       // per iov_len workgroup (kLenRecs records)
    uint64_t* block_hdr;
    uint64_t* block_len_base;  // exclusive scans
    uint64_t* block_hdr_base;
};

constexpr uint64_t kFrameChunkDefault = 65536;  // stream bytes per framing lane (FrameArgs::chunk)

struct FrameArgs {
    const uint8_t* wire;
    uint64_t len;
    uint64_t chunk;         // stream bytes per framing lane
    uint64_t nchunks;
    uint64_t max_records;
    uint64_t* rec_off;      // max_records + 1
    uint64_t* starts;       // per chunk: its first record starts (frame.hip kStartsCap)
    uint64_t* result;       // [5] n, consumed, status, aux0, aux1
    // per chunk
    uint64_t* g;            // guessed / verified first record start (~0 = none)
    uint64_t* x;            // exit or stop position of the chain
    uint32_t* cnt;          // records started in the chunk
    int32_t* st;            // -1 = left the chunk, else the stop status
    uint32_t* aux;          // 2 per chunk
    uint8_t* fail;          // chunk's check failed
    uint8_t* stop;          // chunk's chain ends in it
    uint8_t* fail2;         // per 256 chunks
    uint8_t* stop2;
    uint8_t* fail3;         // per 65536 chunks
    uint8_t* stop3;
    uint32_t* cnt_eff;      // records framed from this chunk
    uint64_t* cnt_base;     // exclusive scan of cnt_eff
    uint64_t* first_fail;
    uint64_t* first_stop;
};

// onc_defragment (defrag.hip). Scratch per fragment: E, S, off (8 bytes
// each), M and the codec's record lengths (4 each): 32 bytes.
struct DefragArgs {
    const uint8_t* wire;
    const uint64_t* frag_off;   // nfrag + 1
    uint64_t nfrag;
    uint8_t* out;           // the 16-byte aligned address at or below the caller's out
    uint64_t origin;        // the caller's out from there (0..15)
    uint64_t out_cap;       // the caller's capacity
    uint64_t* rec_off;      // nfrag + 1
    int32_t* status;        // nfrag
    uint64_t* result;       // [6]
    uint64_t* E;            // nfrag + 1: where a fragment's bytes start in `out` (origin included)
    uint64_t* S;            // nfrag: where they start in `wire`
    uint32_t* M;            // nfrag: the record's mark for its first fragment, else 0
    uint32_t* lens;         // nfrag: record lengths, 0 past the last record
    uint64_t* off;          // nfrag + 1: their scan
    DefragAgg* blk;         // per 256 fragments (+ 1: the whole batch)
    uint64_t* info;         // [0] n_multi, [1] start of the first record beyond the capacity
    // onc_defragment_extents (appended: the fields above keep their kernarg
    // offsets): fragment j is wire[frag_start[j], frag_start[j] + frag_len[j])
    // and frag_off is not read (the defrag_* kernels' extents form)
    const uint64_t* frag_start; // nfrag
    const uint32_t* frag_len;   // nfrag
};

// onc_defragment_heads (defrag_heads.hip). The plan kernels are
// onc_defragment_extents' (a DefragArgs whose E is the caller's frag_pre);
// scratch per fragment in onc_defragment's buffer: S (8 bytes), M and the
// codec's record lengths (4 each).
struct HeadsArgs {
    const uint8_t* wire;
    const uint64_t* frag_start; // nfrag
    const uint32_t* frag_len;   // nfrag
    uint64_t nfrag;
    uint32_t head_len;          // a multiple of 16 in [64, 4096]
    uint8_t* heads;             // 16-byte aligned: slot r at r * head_len
    uint64_t max_records;       // slots
    uint32_t* rec_len;          // nfrag
    uint64_t* rec_frag;         // nfrag + 1
    uint64_t* frag_pre;         // nfrag (the plan's E)
    int32_t* status;            // nfrag
    uint64_t* result;           // [6]
    const uint64_t* S;          // nfrag: the fragment's record index
    const uint32_t* M;          // nfrag: 1 for the first fragment of a record
    const uint32_t* lens;       // nfrag: record lengths (0: ONC_ENC_TOO_LONG)
    const DefragAgg* blk;       // per 256 fragments (+ 1: the whole batch)
    const uint64_t* info;       // [0] n_multi
};

// onc_fragment (fragment.hip). Scratch per record: E (8 bytes) and the block
// sums (24 per 256 records), in onc_defragment's buffer; the copy takes a
// record's source and body length from the caller's rec_off.
struct FragmentArgs {
    const uint8_t* wire;
    const uint64_t* rec_off;    // n + 1
    uint64_t n;
    uint32_t max_frag;      // 1 .. 0x7FFFFFFF
    uint8_t* out;           // the 16-byte aligned address at or below the caller's out
    uint64_t origin;        // the caller's out from there (0..15)
    uint64_t out_cap;       // the caller's capacity
    uint64_t* out_off;      // n + 1
    int32_t* status;        // n
    uint64_t* result;       // [3]
    uint64_t* E;            // n + 1: where a record's fragments start in `out` (origin included)
    FragAgg* blk;           // per 256 records (+ 1: the whole batch)
    uint64_t* info;         // [0] start of the first record beyond the capacity
};

// onc_fragment_iov (fragment_iov.hip). Scratch per record: P and NF (8 bytes
// each) and the block sums (32 per 256 records), in onc_defragment's buffer;
// the fill takes a record's lengths and sources from the caller's iov.
struct FragmentIovArgs {
    const onc_iov_rec* iov;     // n
    uint64_t n;
    uint32_t max_frag;          // 1 .. 0x7FFFFFFF
    const uint32_t* rec_max_frag;   // n, or NULL: max_frag for every record
    uint8_t* marks;             // 4-byte aligned
    uint64_t marks_cap;         // bytes
    onc_frag_piece* pieces;     // 16-byte aligned
    uint64_t max_pieces;
    uint64_t* out_off;          // n + 1
    uint64_t* piece_off;        // n + 1
    int32_t* status;            // n
    uint64_t* result;           // [4]
    uint64_t* P;                // n + 1: the pieces before a record (piece_off, read back by the fill)
    uint64_t* NF;               // n + 1: the fragments before a record
    FivAgg* blk;                // per 256 records (+ 1: the whole batch)
    uint64_t* info;             // [0] first piece of the first record beyond a capacity
};

// onc_piece_offsets / onc_gather_pieces (gather.hip). Scratch: the block
// sums of the offsets (24 bytes per 256 pieces), in onc_defragment's buffer;
// the copy uses none.
struct GatherArgs {
    const onc_frag_piece* pieces;   // npieces, 16-byte aligned
    uint64_t npieces;
    const uint8_t* base0;       // the sources, by ONC_PIECE_*: never indexed, so they stay in scalar registers
    const uint8_t* base1;
    const uint8_t* base2;
    uint64_t len0, len1, len2;  // their lengths in bytes
    uint64_t* piece_pos;        // npieces + 1: written by the offsets, read by the copy
    uint64_t* result;           // [3] (the offsets)
    GatherAgg* blk;             // per 256 pieces (+ 1: the whole list) (the offsets)
    uint64_t from, count;       // the window of the stream (the copy)
    uint8_t* out;               // the 16-byte aligned address at or below the caller's out
    uint64_t origin;            // the caller's out from there (0..15)
};

// onc_payload_slots (payload.hip). Scratch: the block sums of the slots (24
// bytes per 256 records), in onc_defragment's buffer.
struct PaySlotsArgs {
    const onc_msg* msgs;        // n, 16-byte aligned
    const int32_t* status;      // n
    uint64_t n;
    uint32_t head_len;          // the heads form: record r's offsets count from r * head_len
    const uint64_t* rec_start;  // n, or NULL: the heads form
    uint32_t align;             // a power of two in [1, 2^20]
    uint32_t* pay_pos;          // n
    uint32_t* pay_len;          // n
    uint64_t* slot_off;         // n + 1
    onc_msg* msgs_out;          // n, optional; may be msgs
    uint64_t* result;           // [3]
    PayAgg* blk;                // per 256 records (+ 1: the whole batch)
};

// onc_place_payloads (payload.hip). No scratch.
struct PlaceArgs {
    const uint8_t* wire;
    const uint64_t* frag_start; // nfrag
    const uint32_t* frag_len;   // nfrag
    const uint64_t* rec_frag;   // n + 1, or NULL: record r is fragment r
    const uint64_t* frag_pre;   // nfrag, or NULL with rec_frag
    const uint32_t* rec_len;    // n
    const uint32_t* pay_pos;    // n
    const uint32_t* pay_len;    // n
    const uint64_t* slot_off;   // n
    uint64_t n;
    uint8_t* out;               // the 16-byte aligned address at or below the caller's dst
    uint64_t origin;            // the caller's dst from there (0..15)
    uint64_t dst_cap;           // the caller's capacity
};

// onc_route_calls (route.hip). Scratch: the tiles' bin counts, bin-major
// (partition.h), and a total per bin (4 bytes each), in onc_defragment's buffer.
struct RouteArgs {
    const onc_msg* msgs;        // n, 16-byte aligned
    const int32_t* status;      // n
    uint64_t n;                 // < 2^32
    const onc_route* table;     // ntab, 4-byte aligned
    uint32_t ntab;              // <= ONC_ROUTE_TABLE_MAX
    uint32_t nh;                // <= ONC_ROUTE_HANDLERS_MAX
    uint32_t* route;            // n
    uint32_t* order;            // n
    uint64_t* bin_first;        // nh + 4
    onc_msg* calls_out;         // n, optional
    onc_msg* replies;           // n, optional
    uint64_t* result;           // [4]
    uint64_t tiles;             // tile_count(n, kRouteTile)
    uint32_t* counts;           // (nh + 3) * tiles (bin_count_at)
    uint32_t* totals;           // nh + 3
};

// onc_match_replies (match.hip). Scratch, in onc_defragment's buffer
// (match_plan.h MatchLayout): the slot table (S words, S a power of two >=
// 2 np), first_rec (np words), five class counts per tile of records and one
// unanswered count per tile of pending entries.
struct MatchArgs {
    const onc_msg* msgs;        // n, 16-byte aligned
    const int32_t* status;      // n
    const uint32_t* rec_conn;   // n, or NULL: connection 0
    uint64_t n;                 // < ONC_MATCH_MAX
    const onc_pending* pending; // np, 16-byte aligned
    uint64_t np;                // < ONC_MATCH_MAX
    uint32_t* match;            // n
    uint32_t* hit;              // np
    uint64_t* tag_out;          // n, optional
    onc_pending* still;         // np, optional
    uint64_t* result;           // [6]
    uint32_t variant;           // ONC_VARIANT_MATCH_ONE_CHAIN
    uint64_t slots;             // S
    uint64_t clear_words;       // S + np rounded up to 4: what match_clear fills from `table`
    uint64_t rtiles, ptiles;    // match_tiles(n), match_tiles(np)
    uint32_t* table;            // S: a pending index, or kMatchEmpty
    uint32_t* first_rec;        // np: the lowest record that found the entry, or kMatchEmpty
    uint32_t* rec_counts;       // kMatchClasses * rtiles (bin_count_at)
    uint32_t* pend_counts;      // ptiles: counted by match_resolve, scanned by match_scan
};

// onc_group_by_conn (group.hip). Scratch, in onc_defragment's buffer
// (group_plan.h GroupLayout): the tiles' digit counts (partition.h), a total and a first
// position per digit, the bounds kernel's partial counts and two (key, index)
// buffers — 17 bytes per item.
struct GroupArgs {
    const uint32_t* rec_conn;   // nsrc
    uint64_t nsrc;
    const uint32_t* via;        // n, or NULL: item k is rec_conn[k]
    uint64_t n;                 // < 2^32
    uint32_t nconn;             // <= ONC_GROUP_CONN_MAX
    uint32_t passes;            // group_passes(nconn)
    uint32_t pass;              // the launch's pass
    uint32_t digit_bits;        // bits of its digit that can be set
    uint32_t* order;            // n
    uint64_t* conn_first;       // nconn + 2
    const onc_msg* msgs;        // n, optional
    onc_msg* msgs_out;          // n, optional
    uint64_t* result;           // [3]
    uint64_t tiles;             // tile_count(n, kGroupTile)
    uint32_t* counts;           // kGroupDigits * tiles (bin_count_at)
    uint32_t* totals;           // kGroupDigits
    uint32_t* first;            // kGroupDigits
    uint32_t* partial;          // bounds_groups
    uint32_t bounds_groups;     // workgroups of group_bounds
    const uint32_t* src_key;    // n: what a pass after the first reads
    const uint32_t* src_idx;
    uint32_t* dst_key;          // n: what the pass writes
    uint32_t* dst_idx;          // (the last pass: order)
    const uint32_t* sorted_key; // n: the last pass's keys
};

// onc_xdr_unpack (xdr.hip). Scratch: three counts per tile (OK, codes 3..6,
// the other codes; 4 bytes each), in onc_defragment's buffer.
struct XdrArgs {
    const uint8_t* wire;
    uint64_t wire_len;
    const onc_msg* msgs;        // n, 16-byte aligned
    const int32_t* status;      // n
    uint64_t n;
    const uint64_t* rec_start;  // n, or NULL
    uint32_t head_len;          // != 0 (with rec_start NULL): the heads form
    uint32_t nf;                // <= ONC_XDR_FIELDS_MAX
    uint32_t flags;             // ONC_XDR_EXACT
    uint32_t pre_bytes;         // payload bytes a lane fetches before the parse (xdr_reach: how far the schema's
                                // word reads can reach, at most 16 kXdrPre - 15: kXdrPre granules at any alignment)
    uint8_t* cols;
    uint32_t* xstat;            // n
    uint64_t* present;          // n, optional
    uint32_t* rest_pos;         // n, optional
    uint32_t* rest_len;         // n, with rest_pos
    onc_msg* replies;           // n, optional
    uint64_t* result;           // [4]
    uint64_t tiles;             // xdr_tiles(n)
    uint32_t* counts;           // 3 * tiles
    onc_xdr_field fields[ONC_XDR_FIELDS_MAX];   // by value: the field loop reads it with scalar loads
};
constexpr int kXdrPre = 5;      // granules a lane issues up front at most

struct DecArgs {
    uint64_t n;
    const uint8_t* wire;
    const uint64_t* rec_off;
    onc_decoded out;
    uint32_t variant;       // ONC_VARIANT_* bits (onc_codec_options)
    // onc_decode_lengths: offsets from the lengths inside the decode
    const uint32_t* rec_len;
    const uint64_t* tile_sum;   // per decode workgroup (kDecTile records): byte total
    const uint64_t* blk_sum;    // per 4096 records: byte total (summed in the kernel) ...
    const uint64_t* blk_base;   // ... or their exclusive scan (beyond kDecLenFusedBlocks blocks)
    uint64_t nblk;
    uint64_t base;              // offset of record 0
    uint64_t* rec_off_out;      // optional: the offsets (n + 1)
    // onc_decode_body
    uint32_t body;              // 1: the root kernel (decode_kernel<..., kRoot>)
    uint32_t root;              // ONC_ROOT_*; ONC_ROOT_RPC_MESSAGE = the product decode
    const uint32_t* param;      // per record: expected_len / max_len (or NULL)
    uint32_t* consumed;         // optional: bytes the decoded value occupies
    uint32_t* hint;             // the codec's policy word (mapped host memory; decode.hip kLine) or NULL
    uint32_t line;              // message decode: the line policy (decode.hip kLine)
    // onc_decode*_bounded (last, so the fields above keep their kernarg offsets)
    uint32_t bounded;           // 1: the wire-length checked kernels (decode_kernel<..., kBound>)
    uint64_t wire_len;          // readable bytes from `wire`
    // onc_decode_extents (appended: the fields above keep their kernarg offsets)
    const uint64_t* ext_start;  // per record: its first byte's wire offset
    const uint32_t* ext_len;    // per record: its length
    uint32_t extents;           // 1: the extents kernels (decode_kernel<..., kExtents>; always bounded)
    // onc_decode_heads (appended: the fields above keep their kernarg offsets):
    // `wire` is the heads buffer, record i's first min(rec_len[i], head_len)
    // bytes at i * head_len
    uint32_t head_len;          // != 0: the heads kernels (decode_kernel<..., kHeads>)
};

// onc_frame_streams (streams.hip). Scratch per segment: base and x (8 bytes
// each), cnt, st and two aux words (4 each), kStreamKeep record lengths (4
// each): 96 bytes; and 4 per write workgroup (kStreamKeep segments).
constexpr uint32_t kStreamKeep = 16;   // record lengths the chase keeps per segment (= write lanes per segment)
struct StreamsArgs {
    const uint8_t* wire;
    const uint64_t* seg_off;    // nseg
    const uint64_t* seg_len;    // nseg
    uint64_t nseg;
    uint64_t max_records;
    uint64_t* rec_start;        // max_records
    uint32_t* rec_len;          // max_records
    uint32_t* rec_seg;          // max_records, optional
    uint64_t* seg_result;       // 6 * nseg
    uint64_t* result;           // [3] framed, needed, segments stopped
    // per segment, the unbounded chase (max_records does not enter it)
    uint64_t* base;             // nseg + 1: exclusive scan of cnt (onc_scan_lengths); base[nseg] = needed
    uint64_t* x;                // where the chain stops, relative to the segment
    uint32_t* cnt;              // records of the segment
    int32_t* st;                // why it stops (ONC_OK: at the segment's end)
    uint32_t* aux;              // 2 per segment
    uint32_t* keep;             // kStreamKeep per segment: its first records' lengths
    uint32_t* blk_stopped;      // per streams_write workgroup: its segments that stopped
};
// onc_frame_fragment_streams (streams.hip). Scratch per segment: fbase, rbase
// and x (8 bytes each), fcnt, rcnt, st and two aux words (4 each), kStreamKeep
// marks (4 each): 108 bytes; 4 per write workgroup (kStreamKeep segments) and
// two words for the segment the capacity cuts.
struct FragStreamsArgs {
    const uint8_t* wire;
    const uint64_t* seg_off;    // nseg
    const uint64_t* seg_len;    // nseg
    uint64_t nseg;
    uint64_t max_frags;
    uint64_t* frag_start;       // max_frags
    uint32_t* frag_len;         // max_frags
    uint32_t* frag_seg;         // max_frags, optional
    uint64_t* seg_result;       // 8 * nseg
    uint64_t* result;           // [4] fragments emitted, needed, records emitted, segments stopped
    // per segment, the unbounded chase (max_frags does not enter it)
    uint64_t* fbase;            // nseg + 1: exclusive scan of fcnt; fbase[nseg] = needed
    uint64_t* rbase;            // nseg + 1: exclusive scan of rcnt
    uint64_t* x;                // the end of the last complete record, relative to the segment
    uint32_t* fcnt;             // fragments of the segment's complete records
    uint32_t* rcnt;             // its complete records
    int32_t* st;                // why the walk stops (ONC_OK: at the segment's end)
    uint32_t* aux;              // 2 per segment
    uint32_t* keep;             // kStreamKeep per segment: its first marks (the words: bit 31 says last)
    uint32_t* blk_stopped;      // per fragstreams_write workgroup: its segments that stopped
    uint64_t* cut;              // [2] fragments and records emitted up to and with the segment the capacity cuts
};
// the line policy when at least this many of a sampled workgroup's 64
// records needed a second first-round window under the standard one
constexpr uint32_t kLine1Min = 24;
constexpr uint64_t kDecLenBlk = 4096;          // records per length block
constexpr uint64_t kDecLenFusedBlocks = 512;   // up to 2M records: block totals summed in the decode

// encode.hip
hipError_t launch_enc_len(const EncArgs& a, hipStream_t s);
hipError_t launch_enc_emit(const EncArgs& a, hipStream_t s);
// iov.hip
hipError_t launch_iov_len(const IovArgs& a, hipStream_t s);
hipError_t launch_iov_emit(const IovArgs& a, hipStream_t s);
// frame.hip
hipError_t launch_frame_walk(const FrameArgs& a, hipStream_t s, bool frag = false);
hipError_t launch_frame_counts(const FrameArgs& a, hipStream_t s);
hipError_t launch_frame_guess(const FrameArgs& a, hipStream_t s, bool frag = false);
hipError_t launch_frame_chunks(const FrameArgs& a, hipStream_t s, bool frag = false);
hipError_t launch_frame_write(const FrameArgs& a, hipStream_t s);
bool frame_fused_scan_ok(uint64_t nchunks);
hipError_t launch_frame_cblk(const FrameArgs& a, uint64_t* blk_sum, hipStream_t s);
hipError_t launch_frame_write_slots(const FrameArgs& a, const uint64_t* blk_sum, hipStream_t s);
// scan.hip
hipError_t launch_scan_tiles(const uint64_t* in, uint64_t* out_excl, uint64_t count, uint64_t base,
                             uint64_t* total_out, hipStream_t s);
hipError_t launch_len_tiles(const uint32_t* len, uint64_t n, uint64_t* tile_sum, hipStream_t s);
hipError_t launch_len_apply(const uint32_t* len, uint64_t n, const uint64_t* tile_base, uint64_t* rec_off,
                            hipStream_t s);
bool scan_lengths_fused_ok(uint64_t n);
hipError_t launch_store_u64(uint64_t* p, uint64_t v, hipStream_t s);
hipError_t launch_lenblk(const uint32_t* len, uint64_t n, uint64_t* blk_sum, hipStream_t s);
hipError_t launch_lenoff(const uint32_t* len, uint64_t n, const uint64_t* blk_sum, uint64_t base, uint64_t* rec_off,
                         hipStream_t s);
// compact.hip
hipError_t launch_compact_lens(const uint64_t* rec_off, const int32_t* status, uint64_t n, uint32_t* lens,
                               uint64_t* first_drop, hipStream_t s);
hipError_t launch_compact_info(const uint64_t* rec_off, const uint64_t* new_off, uint64_t n,
                               const uint64_t* first_drop, uint64_t* info, hipStream_t s);
hipError_t launch_compact_gather(const uint8_t* out, const uint64_t* rec_off, const uint64_t* new_off, uint64_t fb,
                                 uint64_t n, uint64_t base, uint64_t lo, uint8_t* scratch, hipStream_t s);
hipError_t launch_compact_offsets(uint64_t* rec_off, const uint64_t* new_off, uint64_t fb, uint64_t n, uint64_t base,
                                  hipStream_t s);
hipError_t launch_compact_iov_lens(const onc_iov_rec* iov, const int32_t* status, uint64_t n, uint32_t* lens,
                                   hipStream_t s);
hipError_t launch_compact_iov_apply(onc_iov_rec* iov, const int32_t* status, uint64_t n, const uint64_t* new_off,
                                    uint64_t* totals, hipStream_t s);
// The copy launchers below that take `variant` (the codec's ONC_VARIANT_*
// bits) launch one workgroup under ONC_VARIANT_COPY_ONE_GROUP instead of up
// to their kernel's maximum: the kernels deal their tiles (heads_gather: its
// chunks) out by gridDim.x, so the same code then walks runs of tiles at
// sizes a test can afford.
inline uint64_t copy_max_groups(uint32_t variant, uint64_t max_blocks) {
    return (variant & ONC_VARIANT_COPY_ONE_GROUP) ? 1 : max_blocks;
}
// defrag.hip
// (blk, frag, place: the extents form when a.frag_start is set)
hipError_t launch_defrag_blk(const DefragArgs& a, hipStream_t s);
hipError_t launch_defrag_blkscan(const DefragArgs& a, hipStream_t s);
hipError_t launch_defrag_frag(const DefragArgs& a, hipStream_t s);
hipError_t launch_defrag_place(const DefragArgs& a, hipStream_t s);
hipError_t launch_defrag_copy(const DefragArgs& a, hipStream_t s, uint32_t variant = 0);
// defrag_heads.hip
hipError_t launch_heads_empty(const HeadsArgs& a, hipStream_t s);
hipError_t launch_heads_place(const HeadsArgs& a, hipStream_t s);
hipError_t launch_heads_gather(const HeadsArgs& a, hipStream_t s, uint32_t variant = 0);
// fragment.hip
hipError_t launch_fragp_blk(const FragmentArgs& a, hipStream_t s);
hipError_t launch_fragp_blkscan(const FragmentArgs& a, hipStream_t s);
hipError_t launch_fragp_apply(const FragmentArgs& a, hipStream_t s);
hipError_t launch_frag_copy(const FragmentArgs& a, hipStream_t s, uint32_t variant = 0);
// fragment_iov.hip
hipError_t launch_fragiov_blk(const FragmentIovArgs& a, hipStream_t s);
hipError_t launch_fragiov_blkscan(const FragmentIovArgs& a, hipStream_t s);
hipError_t launch_fragiov_apply(const FragmentIovArgs& a, hipStream_t s);
hipError_t launch_fragiov_fill(const FragmentIovArgs& a, hipStream_t s, uint32_t variant = 0);
// gather.hip
hipError_t launch_gath_blk(const GatherArgs& a, hipStream_t s);
hipError_t launch_gath_blkscan(const GatherArgs& a, hipStream_t s);
hipError_t launch_gath_apply(const GatherArgs& a, hipStream_t s);
hipError_t launch_gath_empty(const GatherArgs& a, hipStream_t s);
hipError_t launch_gather_copy(const GatherArgs& a, hipStream_t s, uint32_t variant = 0);
// payload.hip
hipError_t launch_pay_blk(const PaySlotsArgs& a, hipStream_t s);
hipError_t launch_pay_blkscan(const PaySlotsArgs& a, hipStream_t s);
hipError_t launch_pay_apply(const PaySlotsArgs& a, hipStream_t s);
hipError_t launch_pay_empty(const PaySlotsArgs& a, hipStream_t s);
hipError_t launch_place_copy(const PlaceArgs& a, hipStream_t s, uint32_t variant = 0);
// route.hip
hipError_t launch_route_classify(const RouteArgs& a, hipStream_t s);
hipError_t launch_route_scan_bins(const RouteArgs& a, hipStream_t s);
hipError_t launch_route_scan_total(const RouteArgs& a, hipStream_t s);
hipError_t launch_route_scatter(const RouteArgs& a, hipStream_t s);
// xdr.hip
hipError_t launch_xdr_unpack(const XdrArgs& a, hipStream_t s);
hipError_t launch_xdr_result(const XdrArgs& a, hipStream_t s);
// group.hip
uint32_t group_bounds_groups(uint32_t nconn);
hipError_t launch_group_identity(const GroupArgs& a, hipStream_t s);
hipError_t launch_group_count(const GroupArgs& a, hipStream_t s);
hipError_t launch_group_scan_digits(const GroupArgs& a, hipStream_t s);
hipError_t launch_group_scan_total(const GroupArgs& a, hipStream_t s);
hipError_t launch_group_scatter(const GroupArgs& a, hipStream_t s);
hipError_t launch_group_bounds(const GroupArgs& a, hipStream_t s);
hipError_t launch_group_result(const GroupArgs& a, hipStream_t s);
hipError_t launch_group_gather(const GroupArgs& a, hipStream_t s);
hipError_t launch_conn_extents(const uint64_t* rec_off, uint64_t nrec, const uint64_t* conn_first, uint32_t nconn,
                               uint64_t* conn_off, hipStream_t s);
// match.hip
hipError_t launch_match_clear(const MatchArgs& a, hipStream_t s);
hipError_t launch_match_insert(const MatchArgs& a, hipStream_t s);
hipError_t launch_match_probe(const MatchArgs& a, hipStream_t s);
hipError_t launch_match_resolve(const MatchArgs& a, hipStream_t s);
hipError_t launch_match_scan(const MatchArgs& a, hipStream_t s);
hipError_t launch_match_compact(const MatchArgs& a, hipStream_t s);
// streams.hip
hipError_t launch_streams_chase(const StreamsArgs& a, hipStream_t s);
hipError_t launch_streams_write(const StreamsArgs& a, hipStream_t s);
hipError_t launch_streams_result(const StreamsArgs& a, hipStream_t s);
uint64_t streams_write_groups(uint64_t nseg);
hipError_t launch_fragstreams_chase(const FragStreamsArgs& a, hipStream_t s);
hipError_t launch_fragstreams_write(const FragStreamsArgs& a, hipStream_t s);
hipError_t launch_fragstreams_result(const FragStreamsArgs& a, hipStream_t s);
// decode.hip
hipError_t launch_decode(const DecArgs& a, int mode, hipStream_t s);
hipError_t launch_dlen_tiles(const uint32_t* rec_len, uint64_t n, uint64_t* tile_sum, uint64_t* blk_sum, hipStream_t s);

__host__ __device__ inline uint64_t num_tiles(uint64_t n) { return (n + 255) / 256; }
__host__ __device__ inline uint64_t num_len_blocks(uint64_t n) { return (n + kLenRecs - 1) / kLenRecs; }
__host__ __device__ inline uint64_t num_emit_tiles(uint64_t n) { return (n + kEmitRecs - 1) / kEmitRecs; }
// enc_emit_single_kernel: tiles (waves) of its one workgroup — the largest
// one-launch small-batch encode is kSpWaves * kEmitRecs records
#ifndef ONC_SP_WAVES
#define ONC_SP_WAVES 8
#endif
constexpr int kSpWaves = ONC_SP_WAVES;

}  // namespace onc
