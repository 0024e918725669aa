/*
 * onc_rpc.h — C ABI of the MI355X (gfx950) batch ONC-RPC / XDR codec.
 *
 * This is the drop-in boundary for the reference crate's hot path
 * (domodwyer/onc-rpc v0.3.3, read at /root/reference). Every entry point
 * below names the reference interface it replaces. The reference is a Rust
 * crate whose API is one message per call:
 *
 *   RpcMessage::serialise_into(&self, W: Write)  src/rpc_message.rs:136-164
 *   RpcMessage::serialised_len(&self) -> u32      src/rpc_message.rs:201-204
 *   RpcMessage::try_from(&[u8])                   src/rpc_message.rs:235-271
 *   RpcMessage::try_from(Bytes)                   src/rpc_message.rs:273-314
 *   expected_message_len(&[u8])                   src/rpc_message.rs:343-367
 *
 * Here the caller's per-message loop is replaced by one batch call over N
 * independent records, executed by hand-written HIP kernels on one GPU.
 *
 * Conventions
 *  - Every pointer marked [dev] is device-accessible memory on the codec's
 *    device: device memory (hipMalloc / torch CUDA tensor), or host memory
 *    mapped for the device (onc_host_register, hipHostMalloc / torch pinned
 *    memory), which the kernels then read and write in place over PCIe — a
 *    decode of a socket buffer moves only the header granules it parses.
 *    Nothing is copied to or from the host by these calls; all calls are
 *    asynchronous on the codec's stream.
 *  - The caller owns every buffer (the reference never allocates on decode
 *    and reuses caller buffers on encode, README.md:10-14). The codec only
 *    keeps a small scratch area for the record-offset scan.
 *  - Messages are described by fixed 64-byte descriptors (onc_msg). Opaque
 *    bodies (auth bodies, machine names) and payloads are (offset, length)
 *    references into caller arenas, mirroring the borrowed slices of the
 *    reference's generic `T, P: AsRef<[u8]>` (src/call_body.rs:18-30).
 *  - Per-record results are status codes equal to the reference's Error
 *    variants in declaration order (src/errors.rs:6-97), plus encode-only
 *    codes for the reference's panics and io::Errors.
 */
#ifndef ONC_RPC_H
#define ONC_RPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: onc_batch carries arena sizes (bounds-checked descriptors), onc_encode
 *    accepts any output address, retired kernel id ONC_K_ENC_FIXUP removed.
 * 3: timing id 10 is ONC_K_FRAME_OFFSETS (the framer's chunk verification
 *    now runs inside frame_chunks; ONC_K_FRAME_VERIFY is gone).
 * 4: body-level roots (ONC_ROOT_*, onc_decode_body, onc_encode_body,
 *    onc_encode_body_lengths); timing id 10 retired (ONC_K_FRAME_OFFSETS
 *    gone, the framer ids after it move down by one).
 * 5: decoded AUTH_UNIX slots compacted per 64-record group (onc_decoded):
 *    a slot's index is only what onc_auth.ref says, no longer 2i / 2i + 1.
 * 6: onc_codec_create_ex + onc_codec_options (kernel choices, chunk sizes and
 *    the decode policy are explicit options; the library reads no
 *    environment variable), onc_codec_set_decode_policy, calls refuse to grow
 *    scratch while the stream is being captured (ONC_RC_ECAPTURE); an
 *    AUTH_UNIX onc_auth carries its declared serialised length (kind_len
 *    bits 0..23, written by the decoder; 0 = not declared). */
/* 7: a record whose declared AUTH_UNIX credential fails a deferred block
 *    check keeps its extent with a placeholder header — the record mark of
 *    the extent, then zeros — instead of zeros alone, so that the stream
 *    stays framable (onc_encode_iov emits the same placeholder as its header
 *    iovec); onc_host_register / onc_host_unregister map a caller's host
 *    buffer (a socket buffer) for the kernels to read and write in place. */
/* 8: onc_compact / onc_compact_iov (a failing record's extent dropped from an
 *    encoded batch: the stream the reference's per-message loop writes);
 *    timing id ONC_K_COMPACT; onc_host_unregister takes a NULL codec and
 *    registrations are counted per range (a pinned range belongs to the
 *    process); the rejected-experiment variant bits (EMIT_PRELOAD,
 *    DEC_AUX_SPARSE, SINGLE_PASS, SP_*) are gone.
 *    Added without a version change (nothing existing moved; a caller finds
 *    them by linking): onc_decode_bounded, onc_decode_lengths_bounded,
 *    onc_decode_body_bounded and the status ONC_DEC_BAD_EXTENT;
 *    onc_frame_fragments and onc_defragment (multi-fragment record streams)
 *    with the timing ids ONC_K_DEFRAG_PLAN / ONC_K_DEFRAG_COPY appended
 *    (ONC_K_COUNT 16: onc_codec_kernel_stats writes that many entries);
 *    onc_frame_streams (many connections' buffers framed in one call) and
 *    onc_decode_extents (records that are not back to back), which add no
 *    status code and no timing id; onc_fragment (records cut into fragments
 *    on the send side), which reuses the existing status codes and
 *    onc_defragment's timing ids; onc_frame_fragment_streams and
 *    onc_defragment_extents (fragmented records of many connections
 *    reassembled in one call), which add no status code and no timing id;
 *    onc_defragment_heads and onc_decode_heads (fragmented records decoded
 *    without copying their payloads), which add no status code and no timing
 *    id: the one new outcome is a reason of ONC_DEC_BAD_EXTENT,
 *    ONC_EXTENT_HEAD_SHORT; onc_piece_offsets and onc_gather_pieces with
 *    onc_gather_src (a piece list written as one stream on the device), which
 *    add no status code and reuse onc_defragment's timing ids;
 *    onc_payload_slots and onc_place_payloads (decoded payloads placed in
 *    aligned slots on the device), which add no status code and reuse
 *    onc_defragment's timing ids; onc_route_calls with onc_route (decoded
 *    Calls dispatched to handlers on the device), which adds no status code
 *    and reuses onc_defragment's timing ids; onc_match_replies with
 *    onc_pending (decoded Replies paired with pending Calls on the device),
 *    which adds no status code and reuses onc_defragment's timing ids;
 *    onc_group_by_conn and onc_conn_extents (a send batch grouped by
 *    connection on the device), which add no status code and reuse
 *    onc_defragment's timing ids; onc_xdr_unpack and onc_xdr_schema_check
 *    with onc_xdr_field (Call arguments decoded into columns on the device),
 *    which add no status code (the parse outcomes are the ONC_XDR_* codes of
 *    their own array) and report under ONC_K_DEC_PARSE. */
#define ONC_RPC_ABI_VERSION 8

/* ------------------------------------------------------------------------ */
/* Wire discriminants (values are the on-wire u32s)                          */
/* ------------------------------------------------------------------------ */

/* msg_type — src/rpc_message.rs:16-17 */
#define ONC_MSG_CALL  0u
#define ONC_MSG_REPLY 1u

/* reply_stat — src/reply/reply_body.rs:11-12 */
#define ONC_REPLY_ACCEPTED 0u
#define ONC_REPLY_DENIED   1u

/* accept_stat — src/reply/accepted_reply.rs:10-15 */
#define ONC_ACCEPT_SUCCESS       0u
#define ONC_ACCEPT_PROG_UNAVAIL  1u
#define ONC_ACCEPT_PROG_MISMATCH 2u
#define ONC_ACCEPT_PROC_UNAVAIL  3u
#define ONC_ACCEPT_GARBAGE_ARGS  4u
#define ONC_ACCEPT_SYSTEM_ERR    5u

/* reject_stat — src/reply/rejected_reply.rs:10-11 */
#define ONC_REJECT_RPC_MISMATCH 0u
#define ONC_REJECT_AUTH_ERROR   1u

/* auth_stat — src/reply/rejected_reply.rs:13-20 (AUTH_OK .. AUTH_FAILED = 0..7) */
#define ONC_AUTH_STAT_MAX 7u

/* Auth flavor ids — src/auth/flavor.rs:10-12 */
#define ONC_AUTH_NONE  0u
#define ONC_AUTH_UNIX  1u
#define ONC_AUTH_SHORT 2u

/* AuthFlavor variant (descriptor "kind") — src/auth/flavor.rs:18-49.
 * NONE with length 0 is AuthNone(None); with length > 0 AuthNone(Some(_)).
 * UNKNOWN writes/reads `id` as the wire discriminant. */
#define ONC_KIND_NONE    0u
#define ONC_KIND_UNIX    1u
#define ONC_KIND_SHORT   2u
#define ONC_KIND_UNKNOWN 3u

/* Limits — src/auth/flavor.rs:110 (encode), :83 / opaque 200 (decode);
 * src/auth/unix_params.rs:11-12 */
#define ONC_MAX_AUTH_LEN         200u
#define ONC_MAX_MACHINE_NAME_LEN 255u
#define ONC_MAX_GIDS             16u

/* Decode modes: the two reference decoders */
#define ONC_DECODE_SLICE 0 /* TryFrom<&[u8]>  src/rpc_message.rs:235-271 */
#define ONC_DECODE_BYTES 1 /* TryFrom<Bytes>  src/rpc_message.rs:273-314 */

/* Roots: the reference type a body-level call decodes each record as, or
 * serialises each descriptor as (onc_decode_body / onc_encode_body). The
 * reference has TryFrom / serialise_into / serialised_len on every type of
 * a message, not only on RpcMessage; each root is one of
 * them. `param` is a per-record u32 the root needs (else ignored).
 *                               decode (slice | Bytes)              encode (serialise_into)
 *  RPC_MESSAGE      RpcMessage  rpc_message.rs:235-271 | :273-314   :136-164
 *  MESSAGE_TYPE     MessageType from_cursor :39-45 | TryFrom :80-93 :55-68
 *  CALL_BODY        CallBody    call_body.rs:168-175 | :177-210     :98-108
 *  REPLY_BODY       ReplyBody   reply_body.rs:76-83 | :85-98        :45-56
 *  ACCEPTED_REPLY   AcceptedReply accepted_reply.rs:79-86 | :88-105 :58-61
 *  ACCEPTED_STATUS  AcceptedStatus :234-241 | :243-265              :195-211
 *  REJECTED_REPLY   RejectedReply rejected_reply.rs:98-105 | :107-125 :61-73
 *  AUTH_ERROR       AuthError   from_cursor :176-190 | TryFrom :215-236 :194-207
 *  AUTH_FLAVOR      AuthFlavor  flavor.rs:177-184 | :186-222       :106-129
 *  AUTH_UNIX_PARAMS AuthUnixParams from_cursor(r, expected_len = param)
 *                               unix_params.rs:90-129 | TryFrom :248-276  :162-176
 *  OPAQUE           Opaque (crate-private) from_wire(r, max_len = param)
 *                               opaque.rs:72-98 | try_array bytes_ext.rs:25-42  :38-56
 * Descriptor shape of a root's value (decode writes it, encode reads it;
 * fields outside it are zero on decode and ignored on encode):
 *  MESSAGE_TYPE     as RPC_MESSAGE without xid
 *  CALL_BODY        msg_type CALL, u.call, cred, verf, payload
 *  REPLY_BODY       msg_type REPLY, reply_stat, stat, auth_stat, u.mismatch,
 *                   verf and payload (accepted)
 *  ACCEPTED_REPLY   the same with reply_stat ACCEPTED
 *  ACCEPTED_STATUS  msg_type REPLY, reply_stat ACCEPTED, stat, u.mismatch,
 *                   payload (no verifier)
 *  REJECTED_REPLY   msg_type REPLY, reply_stat DENIED, stat, u.mismatch / auth_stat
 *  AUTH_ERROR       msg_type REPLY, reply_stat DENIED, stat AUTH_ERROR, auth_stat
 *  AUTH_FLAVOR      msg_type CALL, the value in cred (AUTH_UNIX: slot cred.ref)
 *  AUTH_UNIX_PARAMS msg_type CALL, cred kind UNIX (slot cred.ref)
 *  OPAQUE           msg_type CALL, cred kind NONE, its body = the opaque's
 * A descriptor of another shape encodes as ONC_ENC_BAD_DESCRIPTOR. */
#define ONC_ROOT_RPC_MESSAGE      0
#define ONC_ROOT_MESSAGE_TYPE     1
#define ONC_ROOT_CALL_BODY        2
#define ONC_ROOT_REPLY_BODY       3
#define ONC_ROOT_ACCEPTED_REPLY   4
#define ONC_ROOT_ACCEPTED_STATUS  5
#define ONC_ROOT_REJECTED_REPLY   6
#define ONC_ROOT_AUTH_ERROR       7
#define ONC_ROOT_AUTH_FLAVOR      8
#define ONC_ROOT_AUTH_UNIX_PARAMS 9
#define ONC_ROOT_OPAQUE           10
#define ONC_ROOT_COUNT            11
/* Largest opaque body the OPAQUE root encodes: the crate serialises Opaque
 * only for auth bodies (<= 200, flavor.rs:110) and machine names (<= 255,
 * unix_params.rs:149); a longer one is ONC_ENC_BAD_DESCRIPTOR. Decode takes
 * max_len up to ONC_OPAQUE_MAX_LEN (the descriptor's 24-bit length field;
 * the reference calls from_wire with 200 and 255 only): a larger param acts
 * as ONC_OPAQUE_MAX_LEN. */
#define ONC_OPAQUE_ENCODE_MAX 255u
#define ONC_OPAQUE_MAX_LEN    0xFFFFFFu

/* ------------------------------------------------------------------------ */
/* Per-record status codes                                                   */
/* ------------------------------------------------------------------------ */
/* 1..13 are src/errors.rs:6-97 in declaration order.                        */
#define ONC_OK                               0
#define ONC_ERR_INCOMPLETE_MESSAGE           1  /* aux0 = buffer_len, aux1 = expected   errors.rs:14-21 */
#define ONC_ERR_INCOMPLETE_HEADER            2  /* errors.rs:24-25 */
#define ONC_ERR_FRAGMENTED                   3  /* errors.rs:32-33 */
#define ONC_ERR_INVALID_MESSAGE_TYPE         4  /* aux0 = value   errors.rs:42-43 */
#define ONC_ERR_INVALID_REPLY_TYPE           5  /* aux0 = value   errors.rs:52-53 */
#define ONC_ERR_INVALID_REPLY_STATUS         6  /* aux0 = value   errors.rs:59-60 */
#define ONC_ERR_INVALID_AUTH_DATA            7  /* errors.rs:63-64 */
#define ONC_ERR_INVALID_AUTH_ERROR           8  /* aux0 = value   errors.rs:70-71 */
#define ONC_ERR_INVALID_REJECTED_REPLY_TYPE  9  /* aux0 = value   errors.rs:77-78 */
#define ONC_ERR_INVALID_LENGTH              10  /* errors.rs:82-83 */
#define ONC_ERR_INVALID_RPC_VERSION         11  /* aux0 = value   errors.rs:86-87 */
#define ONC_ERR_INVALID_MACHINE_NAME        12  /* errors.rs:91-92 — never produced by a decoder */
#define ONC_ERR_IO_UNEXPECTED_EOF           13  /* IOError(UnexpectedEof, "failed to fill whole buffer")
                                                   errors.rs:95-103 (slice-mode short read) */
/* Encode-only codes (the reference panics or returns io::Error here). */
#define ONC_ENC_TOO_LONG        100 /* io::Error InvalidInput "message length exceeds maximum"
                                       rpc_message.rs:146-151 */
#define ONC_ENC_AUTH_GT_200     101 /* panic: assert!(associated_data_len() <= 200) flavor.rs:110 */
#define ONC_ENC_NAME_GT_255     102 /* panic: AuthUnixParams::new unix_params.rs:149 */
#define ONC_ENC_GIDS_GT_16      103 /* panic: Gids::from_iter unix_params.rs:47 */
#define ONC_ENC_BAD_DESCRIPTOR  104 /* a descriptor the Rust enums cannot represent */
#define ONC_ENC_WRITE_ZERO      105 /* io::Error WriteZero: output capacity exhausted */
/* Bounded-decode-only code (onc_decode_bounded and its siblings). */
#define ONC_DEC_BAD_EXTENT      106 /* panic: slice index out of range: the caller's
                                       `&wire[off..off + len]`. aux0 = why (ONC_EXTENT_*), aux1 = 0 */
#define ONC_EXTENT_START_PAST_WIRE 1 /* the record starts past wire_len */
#define ONC_EXTENT_END_PAST_WIRE   2 /* the record ends past wire_len */
#define ONC_EXTENT_NOT_MONOTONIC   3 /* rec_off[i+1] < rec_off[i] (offset forms) */
#define ONC_EXTENT_HEAD_SHORT      4 /* onc_decode_heads: the record's header does not fit its head */
/* The furthest the message parse reaches into a record (slice mode, the
 * longer one): 4 for the mark, 24 for xid, message type and the four Call
 * words, and two auths of 8 (flavor, length) + 4 + 4 (stamp, name length) +
 * 256 (name) + 12 (uid, gid, gid count) + 64 (gids) each — unix_params.rs:
 * 96-113 reads the block before its length is compared, and flavor.rs:83
 * bounds only the declared length. A head of ONC_HEAD_SPAN_MAX rounded up to
 * 16 (736) holds every header. */
#define ONC_HEAD_SPAN_MAX 724

/* Batch-level return codes of the API functions */
#define ONC_RC_OK        0
#define ONC_RC_EINVAL   -1
#define ONC_RC_EHIP     -2
#define ONC_RC_ENOMEM   -3
#define ONC_RC_EALIGN   -4
#define ONC_RC_ECAPTURE -5   /* the call would allocate scratch while its stream is being captured
                                into a hipGraph: call onc_codec_reserve before the capture */

/* ------------------------------------------------------------------------ */
/* Descriptors                                                               */
/* ------------------------------------------------------------------------ */

/* opaque_auth — AuthFlavor<T> (src/auth/flavor.rs:18-49). 16 bytes.
 *  id       : wire flavor discriminant. Encode writes 0/1/2 for kinds
 *             NONE/UNIX/SHORT and `id` for UNKNOWN; decode stores the value read.
 *  kind_len : bits 0..23 opaque body length (NONE/SHORT/UNKNOWN),
 *             bits 24..31 ONC_KIND_*.
 *             UNIX (ABI 6): the declared length — AuthUnixParams::serialised_len
 *             (unix_params.rs:219-230: 20 + 4 * ceil(name_len / 4) + 4 * ngids)
 *             — or 0 (not declared). The decoder always declares it. On
 *             encode a declared length lets the length pass (onc_encode,
 *             onc_encode_plan) size the record from the descriptor alone,
 *             without reading the 96-byte parameter block; the emit checks
 *             the block when it serialises it (the AuthUnixParams::new / Gids
 *             panics, the machine name inside the auth arena, and declared ==
 *             serialised length — a mismatch is ONC_ENC_BAD_DESCRIPTOR).
 *             Statuses are the reference order's either way. One placement
 *             difference: a record whose only failure is such a block check
 *             keeps the extent its descriptor declares in the output (every
 *             other failing record takes 0 bytes), so that the records after
 *             it stay where the length pass placed them. Its bytes there are a
 *             placeholder that keeps the stream framable (ABI 7): the record
 *             mark of the extent, BE32((extent - 4) | 1 << 31) as
 *             rpc_message.rs:156 writes it — a receiver's expected_message_len
 *             (:343-367) and onc_frame_stream cut it as one record and go on
 *             to the next — then zero bytes up to the payload, which is in
 *             place (a receiver's decode of it fails: InvalidRpcVersion(0)).
 *             onc_encode_lengths reports the same extents (with every check's
 *             status) and onc_encode_iov places records by them (such a
 *             record: its placeholder as the header iovec, its payload
 *             slice); the body roots check every block up front.
 *  ref      : NONE/SHORT/UNKNOWN: byte offset of the body in the auth arena
 *             (decode: in the wire buffer). UNIX: index into the unix table. */
typedef struct onc_auth {
    uint32_t id;
    uint32_t kind_len;
    uint64_t ref;
} onc_auth;

#define ONC_AUTH_KIND(a)        ((uint32_t)((a).kind_len >> 24))
#define ONC_AUTH_LEN(a)         ((uint32_t)((a).kind_len & 0xFFFFFFu))
#define ONC_AUTH_PACK(kind, len) ((uint32_t)(((uint32_t)(kind) << 24) | ((uint32_t)(len) & 0xFFFFFFu)))

/* RpcMessage<T, P> (src/rpc_message.rs:97-105) with its MessageType,
 * CallBody (src/call_body.rs:17-30) / ReplyBody (src/reply/ *.rs). 64 bytes.
 *
 *  msg_type    ONC_MSG_CALL | ONC_MSG_REPLY
 *  reply_stat  reply: ONC_REPLY_ACCEPTED | ONC_REPLY_DENIED
 *  stat        accepted: ONC_ACCEPT_*; denied: ONC_REJECT_*
 *  auth_stat   denied AUTH_ERROR: AuthError (0..7)
 *  call        program / program_version / procedure (CallBody)
 *  mismatch    low / high of ProgramMismatch or RpcVersionMismatch
 *  payload_*   Call payload or Success payload (raw, unpadded; call_body.rs:107,
 *              accepted_reply.rs:199): encode = payload arena offset,
 *              decode = wire offset
 *  cred        call credentials (unused for replies)
 *  verf        call verifier or accepted-reply verifier */
typedef struct onc_msg {
    uint32_t xid;
    uint8_t  msg_type;
    uint8_t  reply_stat;
    uint8_t  stat;
    uint8_t  auth_stat;
    union {
        struct { uint32_t program, program_version, procedure; } call;
        struct { uint32_t low, high, reserved; } mismatch;
    } u;
    uint32_t payload_len;
    uint64_t payload_off;
    onc_auth cred;
    onc_auth verf;
} onc_msg;

/* AuthUnixParams<T> (src/auth/unix_params.rs:72-82). 96 bytes.
 * name_off is an auth-arena offset (decode: wire offset). */
typedef struct onc_unix_params {
    uint32_t stamp;
    uint32_t uid;
    uint32_t gid;
    uint32_t ngids;
    uint64_t name_off;
    uint32_t name_len;
    uint32_t reserved;
    uint32_t gids[16];
} onc_unix_params;

/* A batch of messages to encode. [dev] pointers. auth_arena and
 * payload_arena may alias (e.g. both = the wire buffer of a decoded batch).
 * The three sizes bound every reference a descriptor makes: a unix-table
 * index >= unix_count, an auth body / machine name [off, off + len) beyond
 * auth_len or a payload beyond payload_len makes that record
 * ONC_ENC_BAD_DESCRIPTOR (checked before anything is read through it), so a
 * malformed descriptor can never make a kernel read outside the arenas.
 * Zero-length bodies and payloads are not checked (their offsets are never
 * dereferenced). The reference's owned types cannot express such a
 * reference; the check replaces an out-of-bounds read, not a reference
 * behaviour. The sizes must be true: the encoder may read any byte of
 * [payload_arena, payload_arena + payload_len) (it loads whole 16-byte
 * windows at each output chunk's own source bytes when they all lie in the
 * arena), never a byte outside it. */
typedef struct onc_batch {
    uint64_t               n;
    const onc_msg*         msgs;          /* [dev] n descriptors */
    const onc_unix_params* unix_params;   /* [dev] AUTH_UNIX table (may be NULL if unix_count == 0) */
    const uint8_t*         auth_arena;    /* [dev] auth bodies + machine names */
    const uint8_t*         payload_arena; /* [dev] payloads */
    uint64_t               unix_count;    /* entries in unix_params */
    uint64_t               auth_len;      /* bytes in auth_arena */
    uint64_t               payload_len;   /* bytes in payload_arena */
} onc_batch;

/* Decode outputs. [dev] pointers.
 * unix_params has 2*n slots. The AUTH_UNIX parameter sets of the OK records
 * of each 64-record group [64g, 64g + 64) (counted from the call's first
 * record) take consecutive slots from 128g, in record order, credential
 * before verifier; onc_auth.ref holds the slot index. Slots past a group's
 * last set are not written. (Packed, the sets of a group are written as
 * whole contiguous lines: a slot pair per record, 2i / 2i + 1, scattered
 * them 192 bytes apart.)
 * Offsets in the decoded descriptors are wire-buffer offsets, so a decoded
 * batch can be re-encoded with auth_arena = payload_arena = wire and
 * unix_params as the AUTH_UNIX table (unix_count = 2n).
 * For a record with status != ONC_OK the descriptor is all zero and it takes
 * no slot. */
typedef struct onc_decoded {
    onc_msg*         msgs;        /* n */
    onc_unix_params* unix_params; /* 2n */
    int32_t*         status;      /* n */
    uint32_t*        aux0;        /* n: buffer_len or the offending value */
    uint32_t*        aux1;        /* n: expected (IncompleteMessage) */
} onc_decoded;

/* ------------------------------------------------------------------------ */
/* Codec handle                                                              */
/* ------------------------------------------------------------------------ */

typedef struct onc_codec onc_codec;

/* Decode first-round policy (decode.hip): how much of each record's header
 * the decode's first load round fetches. Results never depend on it, only
 * the time. AUTO picks it per launch from the records the previous decode
 * launch on the handle sampled (a word the kernel writes to mapped host
 * memory, read at the next launch without a synchronisation); STANDARD
 * fetches the first 44 bytes (short headers: AUTH_NONE calls, replies);
 * LINE the rest of the record's first 128-byte line (long AUTH_UNIX
 * headers). A hipGraph captures the policy in force when it is captured. */
#define ONC_DECODE_POLICY_AUTO     0
#define ONC_DECODE_POLICY_STANDARD 1
#define ONC_DECODE_POLICY_LINE     2

/* Kernel-variant bits (onc_codec_options.variant): measurement and test
 * switches that force a kernel the codec would otherwise choose per batch.
 * Results are bit-identical under every combination; production leaves 0.
 * ONC_VARIANT_COPY_ONE_GROUP changes no kernel: the copy kernels of
 * onc_defragment(_extents), onc_fragment, onc_gather_pieces,
 * onc_place_payloads, onc_fragment_iov and onc_defragment_heads are launched
 * as one workgroup instead of one per 32 KiB of capacity. They deal their
 * output tiles out by gridDim.x, so each of the four waves then walks a run
 * of ceil(tiles / 4) consecutive tiles, which the default grid does only
 * beyond 64 MiB of output (tests of that walk; slow on anything large). */
#define ONC_VARIANT_EMIT_WS          0x200u    /* force the wave-specialised enc_emit */
#define ONC_VARIANT_EMIT_TILE        0x400u    /* force the wave-per-tile enc_emit */
#define ONC_VARIANT_WS_NO_INTERIOR   0x4000u   /* wave-specialised: no interior spans */
#define ONC_VARIANT_WS_NO_FULL       0x8000u   /* wave-specialised: no full-interior spans */
#define ONC_VARIANT_WS_PIPELINE      0x10000u  /* wave-specialised: the pipeline on header-heavy batches too */
#define ONC_VARIANT_EMIT_REPLAN      0x20000u  /* wave-per-tile enc_emit re-plans instead of reading the plan's lengths */
#define ONC_VARIANT_WHOLE_PLAN       0x40000u  /* plan a large batch whole instead of in chunks */
#define ONC_VARIANT_MATCH_ONE_CHAIN  0x80000u  /* onc_match_replies: every key hashes to slot S - 2 (one wrapping chain) */
#define ONC_VARIANT_COPY_ONE_GROUP   0x100000u /* the copy kernels run in one workgroup (runs of tiles per wave at test sizes) */

#define ONC_OPT_FORCE_SCAN 0x1u   /* always launch the separate block-scan kernels (tests of that path) */

/* Options of onc_codec_create_ex; all-zero (or a NULL pointer) = the
 * defaults, which are what onc_codec_create uses. The library reads nothing
 * from the environment. */
typedef struct onc_codec_options {
    uint32_t size;           /* sizeof(onc_codec_options), or 0 */
    uint32_t flags;          /* ONC_OPT_* */
    int32_t  decode_policy;  /* ONC_DECODE_POLICY_* */
    uint32_t variant;        /* ONC_VARIANT_* bits (A/B measurements and tests; 0 in production) */
    uint64_t enc_chunk;      /* records per plan + emit chunk of a large encode (rounded down to a
                                multiple of 1024; 0 = 1M) */
    uint64_t frame_chunk;    /* bytes per onc_frame_stream chunk (>= 64; 0 = 64 KiB) */
} onc_codec_options;

/* One handle per device: a HIP stream + scan scratch. `hip_stream` may be
 * NULL (the device's null stream) or a hipStream_t owned by the caller. */
int onc_codec_create(onc_codec** out, int device, void* hip_stream);
int onc_codec_create_ex(onc_codec** out, int device, void* hip_stream, const onc_codec_options* options);
int onc_codec_destroy(onc_codec* codec);
int onc_codec_set_stream(onc_codec* codec, void* hip_stream);
int onc_codec_set_decode_policy(onc_codec* codec, int policy);
int onc_codec_sync(onc_codec* codec);
/* Pre-size the scratch for batches of up to max_records (scan totals, the
 * plan's record lengths), so that later encode / decode / scan calls of up
 * to that many records perform no allocation. Required before capturing
 * calls into a hipGraph: a call that would grow the scratch while its
 * stream is capturing returns ONC_RC_ECAPTURE (outside a capture the
 * scratch grows on demand with a synchronous hipMalloc). onc_frame_stream
 * keeps its own per-chunk scratch, sized by its first call on a stream that
 * long or longer (growing it inside a capture is ONC_RC_ECAPTURE too);
 * onc_frame_fragments shares it. onc_defragment of up to max_records
 * fragments is covered too (32 bytes of scratch per fragment; onc_fragment
 * and onc_fragment_iov of up to max_records records use the same buffer,
 * under 32 bytes per record), and so is onc_frame_streams of up to max_records segments (under 100 bytes per
 * segment). onc_defragment_extents is covered as onc_defragment is, and
 * onc_frame_fragment_streams of up to max_records segments as
 * onc_frame_streams is (the two share one buffer of under 112 bytes per
 * segment). onc_payload_slots of up to max_records records keeps its block
 * sums in onc_defragment's buffer (under 1 byte per record) and is covered
 * too; onc_place_payloads needs no scratch. onc_route_calls of up to
 * max_records records keeps its bin counts there as well (about 1 byte per
 * record at 256 bins, and 2 KiB of them however few the records): that buffer
 * is never smaller than 65536 fragments' worth (1.8 MB), so a reserve for a
 * handful of records covers the call at any table and handler count.
 * onc_match_replies of up to max_records records against up to max_records
 * pending entries builds its slot table, first_rec and tile counts there too
 * (under 32 bytes per pending entry plus under 1 byte per 32 records): a
 * reserve of max(n, np) covers the call. onc_group_by_conn of up to
 * max_records items keeps its digit counts and two (key, index) buffers there
 * (17 bytes per item and 7 KiB); onc_conn_extents needs no scratch.
 * onc_xdr_unpack of up to max_records records keeps three counts per
 * ONC_XDR_TILE records there (under 0.05 bytes per record). */
int onc_codec_reserve(onc_codec* codec, uint64_t max_records);
/* Map a caller's host buffer (a socket buffer: any malloc'd or mmap'd
 * range) for the kernels, so that an encode / decode reads and writes it in
 * place instead of through a staging copy: pins its pages
 * (hipHostRegister, mapped and portable) and returns the device address of
 * `host` in *dev_ptr, usable as any [dev] pointer of this header. The
 * zero-copy counterpart of the reference's borrowed slices
 * (call_body.rs:53-59, opaque.rs:92-97): onc_decode of a registered wire
 * fetches only the 16-byte granules holding the header bytes it parses over
 * the link, never the payloads. Synchronous. A pinned range belongs to the
 * process, not to the codec (destroying the codec leaves it pinned): a
 * register of a range inside one this library pinned maps it and counts one
 * more registration of that range; each onc_host_unregister counts one
 * down and the last unpins it. A range already pinned by its owner
 * (hipHostMalloc, torch's pin_memory) needs no registration: its device
 * address is returned and nothing is recorded (onc_host_unregister of it is
 * then a no-op). The address is for the codec's device. Returns
 * ONC_RC_EINVAL for a NULL pointer or length, or for a range that starts in
 * pinned memory but runs past that pinned allocation; ONC_RC_EHIP if the
 * runtime refuses the range (onc_codec_last_error says why). */
int onc_host_register(onc_codec* codec, void* host, uint64_t len, void** dev_ptr);
/* Undo one onc_host_register of a range this library pinned (`host`: any
 * address inside it; the kernels must be done with it); the last one unpins
 * the range. `codec` may be NULL (it is only where an error is reported):
 * a registration may outlive the codec that made it. */
int onc_host_unregister(onc_codec* codec, void* host);

/* Last HIP error string seen by this handle ("" if none). */
const char* onc_codec_last_error(const onc_codec* codec);
const char* onc_status_str(int32_t status);
int onc_abi_version(void);

/* Per-kernel event timing (for the bench's roofline). `enable` is a bitmask
 * of kernel ids (1 << ONC_K_*; ONC_TIMING_ALL = every kernel, 0 = off): each
 * launch of a selected kernel carries start/stop hipEvents on the codec
 * stream (hipExtLaunchKernelGGL: the dispatch's own timestamps); the
 * accumulated device time and launch count per kernel id are returned by
 * onc_codec_kernel_stats after a sync. Timing only the kernel of interest
 * keeps the event overhead off the other launches. An id names a launch
 * site: ONC_K_ENC_EMIT is either enc_emit kernel; ONC_K_LEN_TILES /
 * ONC_K_LEN_APPLY are onc_scan_lengths' first and second launch (lenblk /
 * lenoff up to 8M records); ONC_K_FRAME_COUNTS the framer's count pass
 * (frame_cblk, or frame_counts ahead of the three-launch scan beyond 512k
 * chunks); ONC_K_FRAME_WRITE its start copy, which up to 512k chunks also
 * sums each chunk's first record index. The body-level calls use the ids of
 * the kernels they launch (ONC_K_ENC_LEN / _ENC_EMIT / _DEC_PARSE).
 * onc_frame_fragments launches at onc_frame_stream's sites (ONC_K_FRAME_*);
 * ONC_K_DEFRAG_PLAN is every planning launch of onc_defragment (its length
 * scan counts as onc_scan_lengths'), ONC_K_DEFRAG_COPY the byte copy.
 * onc_frame_streams and onc_decode_extents have no ids of their own: the
 * per-segment chase (streams_chase) reports under ONC_K_FRAME, the scan of
 * the segments' record counts under onc_scan_lengths' ids (ONC_K_LEN_TILES /
 * ONC_K_LEN_APPLY, with ONC_K_SCAN_TILES beyond 8M segments), the write pass
 * (streams_write) under ONC_K_FRAME_WRITE, the count of stopped segments
 * (streams_result) under ONC_K_FRAME_COUNTS, and the extents decode under
 * ONC_K_DEC_PARSE. onc_fragment has none either: its three plan launches
 * report under ONC_K_DEFRAG_PLAN and its copy under ONC_K_DEFRAG_COPY (it
 * launches no onc_scan_lengths kernel: its scan is 64 bits wide), and so do
 * onc_fragment_iov's three plan launches and its fill.
 * onc_frame_fragment_streams reports under the ids onc_frame_streams uses:
 * its chase (fragstreams_chase) under ONC_K_FRAME, its two scans (fragment
 * counts, record counts) under onc_scan_lengths' ids, its write pass
 * (fragstreams_write) under ONC_K_FRAME_WRITE and its result
 * (fragstreams_result) under ONC_K_FRAME_COUNTS. onc_defragment_extents
 * reports as onc_defragment does (ONC_K_DEFRAG_PLAN / ONC_K_DEFRAG_COPY).
 * onc_defragment_heads reports its plan launches (defrag_blk, defrag_blkscan,
 * defrag_frag, heads_place) under ONC_K_DEFRAG_PLAN and its gather
 * (heads_gather) under ONC_K_DEFRAG_COPY; it launches no onc_scan_lengths
 * kernel. onc_decode_heads reports under ONC_K_DEC_PARSE. onc_payload_slots
 * reports its launches (pay_blk, pay_blkscan, pay_apply; pay_empty) under
 * ONC_K_DEFRAG_PLAN and onc_place_payloads its copy (place_copy) under
 * ONC_K_DEFRAG_COPY. onc_route_calls reports its classify and scan launches
 * (route_classify, route_scan_bins, route_scan_total) under
 * ONC_K_DEFRAG_PLAN and its scatter (route_scatter) under ONC_K_DEFRAG_COPY.
 * onc_match_replies reports its clear, insert, probe, resolve and scan
 * launches (match_clear, match_insert, match_probe, match_resolve,
 * match_scan) under ONC_K_DEFRAG_PLAN and its compaction (match_compact)
 * under ONC_K_DEFRAG_COPY. onc_group_by_conn reports its counts, scans,
 * bounds and result (group_count, group_scan_digits, group_scan_total,
 * group_bounds, group_result) under ONC_K_DEFRAG_PLAN and its scatters and
 * gather (group_identity, group_scatter, group_gather) under
 * ONC_K_DEFRAG_COPY; onc_conn_extents' one launch reports under
 * ONC_K_DEFRAG_PLAN. onc_xdr_unpack reports its two launches (xdr_unpack,
 * xdr_result) under ONC_K_DEC_PARSE. */
#define ONC_K_ENC_LEN      0
#define ONC_K_SCAN_TILES   1
#define ONC_K_ENC_EMIT     2
#define ONC_K_DEC_PARSE    3
#define ONC_K_LEN_TILES    4
#define ONC_K_LEN_APPLY    5
#define ONC_K_IOV_LEN      6
#define ONC_K_IOV_EMIT     7
#define ONC_K_FRAME        8
#define ONC_K_FRAME_WRITE  9
#define ONC_K_FRAME_WALK   10
#define ONC_K_FRAME_COUNTS 11
#define ONC_K_FRAME_GUESS  12
#define ONC_K_COMPACT      13
#define ONC_K_DEFRAG_PLAN  14
#define ONC_K_DEFRAG_COPY  15
#define ONC_K_COUNT        16
#define ONC_TIMING_ALL    (-1)
int onc_codec_enable_timing(onc_codec* codec, int enable);
int onc_codec_kernel_stats(onc_codec* codec, double* ms_total /*[ONC_K_COUNT]*/,
                           uint64_t* launches /*[ONC_K_COUNT]*/);
int onc_codec_reset_stats(onc_codec* codec);
const char* onc_kernel_name(int kernel_id);

/* ------------------------------------------------------------------------ */
/* Encode — RpcMessage::serialise_into (src/rpc_message.rs:136-164)          */
/* ------------------------------------------------------------------------ */

/* serialised_len() of every record (src/rpc_message.rs:201-204) plus the
 * encode-time validation of serialise_into (oversize, panics).
 * rec_len[dev,n] receives the length (0 for a record whose status != OK,
 * except a declared AUTH_UNIX record failing only a parameter-block check:
 * its declared extent, as onc_encode places it — onc_auth), so the sum is
 * the size of onc_encode's output; status[dev,n] receives ONC_OK or an
 * ONC_ENC_* code. */
int onc_encode_lengths(onc_codec* codec, const onc_batch* batch,
                       uint32_t* rec_len, int32_t* status);

/* Encode every record back to back into out[dev] (out_cap bytes): the
 * batch equivalent of calling serialise_into for each message in order on
 * one Cursor<Vec<u8>> (a TCP send buffer). `out` may be any byte address —
 * the cursor's current position in a partly filled buffer — and bytes
 * before `out` or at/after out + out_cap are never written (the reference
 * writes at the writer's position, rpc_message.rs:136, and reuses buffers,
 * README.md:11). Whole 16-byte-aligned chunks are written with one store;
 * the chunks at either end of the batch are written byte by byte.
 *   rec_off[dev, n+1]: record i occupies out[rec_off[i], rec_off[i+1]);
 *                      rec_off[n] is the total byte count.
 *   status[dev, n]   : ONC_OK or ONC_ENC_*. Records that fail validation
 *                      occupy 0 bytes — except a declared AUTH_UNIX record
 *                      failing only its deferred parameter-block check, which
 *                      keeps its declared extent as a framable placeholder
 *                      (onc_auth). Bytes at or beyond out_cap are never
 *                      written; records ending beyond it get ONC_ENC_WRITE_ZERO.
 *   rec_len[dev, n]  : optional (may be NULL) serialised lengths.
 * Launches: a length pass and the emit per 1M-record chunk; a batch of at
 * most 512 records is planned and emitted in one launch (the results are the
 * same). */
int onc_encode(onc_codec* codec, const onc_batch* batch,
               uint8_t* out, uint64_t out_cap,
               uint64_t* rec_off, int32_t* status, uint32_t* rec_len);

/* onc_encode in two phases on the handle's stream, so that the length pass
 * of one batch can run while other work (the decode of the previous batch,
 * on another stream) is in flight:
 *   onc_encode_plan : serialised_len() + validation of every record
 *                     (status, optional rec_len) and the placement totals,
 *                     kept in this handle's scratch (enc_len);
 *   onc_encode_emit : the bytes, placed by that plan (enc_emit) — same
 *                     arguments and results as onc_encode.
 * The plan belongs to the handle: emit must name the batch last planned on
 * it (same msgs pointer and n) with the status array the plan filled (the
 * plan's statuses stand; emit adds ONC_ENC_WRITE_ZERO and the status of a
 * declared AUTH_UNIX auth's parameter-block check, onc_auth), else
 * ONC_RC_EINVAL; any other call on the handle in between that uses its
 * scratch (every encode, decode_lengths and scan_lengths call) discards the
 * plan (then ONC_RC_EINVAL too). The descriptors must not change in between,
 * nor the plan's rec_len array when one was given (for a batch with an
 * AUTH_UNIX table the emit reads the record lengths back from it instead of
 * re-planning). onc_encode = plan + emit (for more than 512 records; a
 * smaller batch it encodes in one launch). */
int onc_encode_plan(onc_codec* codec, const onc_batch* batch, int32_t* status, uint32_t* rec_len);
int onc_encode_emit(onc_codec* codec, const onc_batch* batch, uint8_t* out, uint64_t out_cap,
                    uint64_t* rec_off, int32_t* status);

/* Vectored encode (the zero-copy writer the reference
 * plans in README.md:71-75 and rpc_message.rs:19): only the header part of
 * every record (everything before the raw payload) is serialised, into
 * hdr_out[dev] back to back; payloads stay where they are in the batch's
 * payload arena. Record i on the wire is
 *     hdr_out[iov[i].hdr_off, +hdr_len) ++ payload_arena[iov[i].payload_off, +payload_len)
 * and starts at iov[i].wire_off of the equivalent packed send buffer, i.e.
 * the bytes onc_encode would produce, for a writev()/scatter-gather sender.
 *   iov[dev, n]    : one entry per record; all zero lengths for a record
 *                    whose status != ONC_OK (except a declared AUTH_UNIX
 *                    record failing only its deferred block check: its
 *                    placeholder header and payload slice, as onc_encode
 *                    writes them, onc_auth).
 *   status[dev, n] : ONC_OK or ONC_ENC_*; a record whose header would end
 *                    beyond hdr_cap gets ONC_ENC_WRITE_ZERO and none of its
 *                    header bytes are written.
 *   totals[dev, 2] : optional: {header bytes, wire bytes} of the batch. */
typedef struct onc_iov_rec {
    uint64_t hdr_off;
    uint64_t payload_off;
    uint64_t wire_off;
    uint32_t hdr_len;
    uint32_t payload_len;
} onc_iov_rec;

int onc_encode_iov(onc_codec* codec, const onc_batch* batch,
                   uint8_t* hdr_out, uint64_t hdr_cap,
                   onc_iov_rec* iov, int32_t* status, uint64_t* totals);

/* Drop the extent of every record whose status != ONC_OK from a buffer
 * onc_encode wrote, in place: afterwards out[rec_off[i], rec_off[i+1]) is
 * record i for an OK record and empty for any other, the OK records back to
 * back from rec_off[0] (unchanged) on — the bytes the reference's loop of
 * serialise_into calls on one Cursor<Vec<u8>> writes for the same messages,
 * since a message that panics (unix_params.rs:47,149, flavor.rs:110) or
 * fails writes nothing. Only placeholders (a declared AUTH_UNIX credential
 * failing its deferred block check, onc_auth) have an extent to drop; every
 * other failing record already takes 0 bytes, so a batch without a
 * placeholder moves nothing. `status` is onc_encode's. Bytes from the new
 * rec_off[n] up to the old one are left as they were. *total (host,
 * optional) receives the new rec_off[n]. Synchronous: it sizes its scratch
 * by the moved bytes, which it reads back, and returns with the buffer and
 * rec_off final (ONC_RC_ECAPTURE inside a stream capture). For the rare
 * path: call it only after seeing a failing status. */
int onc_compact(onc_codec* codec, uint8_t* out, uint64_t* rec_off, const int32_t* status, uint64_t n,
                uint64_t* total);

/* The same for onc_encode_iov's list: every entry whose status != ONC_OK
 * gets hdr_len = payload_len = 0 and every wire_off is the kept bytes before
 * it (rec_off[0] = 0); hdr_off / payload_off are kept. totals[dev, 2]
 * (optional): {kept header bytes, kept wire bytes}. Asynchronous. */
int onc_compact_iov(onc_codec* codec, onc_iov_rec* iov, const int32_t* status, uint64_t n, uint64_t* totals);

/* ------------------------------------------------------------------------ */
/* Decode — RpcMessage::try_from(&[u8]) / try_from(Bytes)                    */
/* ------------------------------------------------------------------------ */

/* Decode record i = wire[rec_off[i] .. rec_off[i+1]) for i < n, each
 * exactly as the reference decodes one buffer that must hold exactly one
 * message (src/rpc_message.rs:238-242). mode = ONC_DECODE_SLICE | _BYTES.
 * Memory access: the decoder reads its records' header bytes as whole
 * 16-byte-aligned granules (one dwordx4 per granule), so it may read up to
 * 15 bytes before rec_off[i] / after rec_off[i+1] — never outside the
 * aligned 16-byte granules that hold record bytes, so never across a page
 * or allocation boundary of a hipMalloc'd buffer. Those bytes never affect
 * the result; no byte of the wire is written. */
int onc_decode(onc_codec* codec, const uint8_t* wire, const uint64_t* rec_off,
               uint64_t n, int mode, const onc_decoded* out);

/* expected_message_len (src/rpc_message.rs:343-367) of one host buffer: the
 * record-marking header's length + 4. Returns ONC_OK, or
 * ONC_ERR_INCOMPLETE_HEADER (len < 4) / ONC_ERR_FRAGMENTED (last-fragment
 * bit clear). Host memory, synchronous; the framing helper a caller uses to
 * cut one message out of a socket buffer. */
int32_t onc_expected_message_len(const uint8_t* data, uint64_t len, uint32_t* out);

/* Framing of a stream buffer of back-to-back record-marked messages (a
 * socket read buffer): the caller's loop of expected_message_len
 * (src/rpc_message.rs:343-367) + one-message slices
 * (rpc_message.rs:238-242), in parallel on the device with the same result.
 * From offset 0, records are framed while the remaining bytes hold a whole
 * record and fewer than max_records were framed.
 *   rec_off[dev, max_records + 1]: starts of the framed records, then the
 *                     end of the last one (= bytes consumed).
 *   result[dev, 5]  : {n, consumed, status, aux0, aux1}; status is ONC_OK when
 *                     the buffer ends on a record boundary or max_records
 *                     were framed, else why the next record cannot be cut:
 *                     ONC_ERR_INCOMPLETE_HEADER (< 4 bytes left),
 *                     ONC_ERR_FRAGMENTED (last-fragment bit clear) or
 *                     ONC_ERR_INCOMPLETE_MESSAGE {aux0 = bytes left,
 *                     aux1 = record length} (wait for more data).
 * The stream is cut into 64 KiB chunks framed speculatively in parallel and
 * verified (frame.hip); onc_codec_options.frame_chunk overrides the chunk
 * size (tests use small chunks to exercise the multi-chunk logic).
 * SURVEY §8(f) rank 1. */
int onc_frame_stream(onc_codec* codec, const uint8_t* wire, uint64_t len,
                     uint64_t* rec_off, uint64_t max_records, uint64_t* result);

/* onc_frame_stream at fragment level (RFC 5531 §11: a record is one or more
 * fragments, the last one marked by bit 31 of its mark — streams the
 * reference rejects: Error::Fragmented, rpc_message.rs:359-362, "No support
 * for fragmented messages", README.md:62). Every mark starts a fragment,
 * whatever its last-fragment bit; the result is that of
 *
 *   p = 0; n = 0; st = ONC_OK
 *   while p < len and n < max_frags:
 *       if len - p < 4:     st = ONC_ERR_INCOMPLETE_HEADER; break
 *       h = be32(wire, p); want = (h & 0x7FFFFFFF) + 4        (rpc_message.rs:343-367 without :359-362)
 *       if len - p < want:  st = ONC_ERR_INCOMPLETE_MESSAGE; aux0 = len - p; aux1 = want; break
 *       frag_off[n++] = p; p += want
 *   frag_off[n] = p; result = {n, p, st, aux0, aux1}
 *
 * so ONC_ERR_FRAGMENTED is never reported; len == 0 or max_frags == 0 gives
 * all zeros. Arguments, scratch, ONC_RC_ECAPTURE, frame_chunk and the timing
 * ids are onc_frame_stream's: the same speculative machine in its fragment
 * mode (frame.hip), where a chunk's chain runs on through continuation
 * fragments — which carry no RPC header to guess by — up to the next guess.
 * When onc_frame_stream stops with ONC_ERR_FRAGMENTED at `consumed`, call
 * this and onc_defragment on the rest of the buffer, then go on as usual on
 * onc_defragment's output. */
int onc_frame_fragments(onc_codec* codec, const uint8_t* wire, uint64_t len,
                        uint64_t* frag_off /*[dev, max_frags + 1]*/, uint64_t max_frags,
                        uint64_t* result /*[dev, 5]: n, consumed, status, aux0, aux1*/);

/* Segmented framing: onc_frame_stream for many independent buffers at once —
 * a server's per-connection receive buffers, usually slots of one pinned
 * slab, each filled to its own level and holding a few whole records and
 * often a cut one at the end. The reference anchor is the caller's loop of
 * expected_message_len (src/rpc_message.rs:343-367) + one-message slices
 * (rpc_message.rs:238-242), run once per connection. Segment s is
 * wire[seg_off[s], seg_off[s] + seg_len[s]); segments may lie in any address
 * order, start at any byte alignment and overlap (the wire is only read).
 * seg_off / seg_len are trusted, as `len` is in onc_frame_stream;
 * seg_len[s] < 2^34 (so a segment holds fewer than 2^32 records) and
 * nseg < 2^32 are preconditions (nseg >= 2^32 is ONC_RC_EINVAL). The result
 * is exactly that of
 *
 *   k = 0; needed = 0
 *   for s in 0 .. nseg-1:
 *       first = k; p = 0; st = ONC_OK; aux0 = aux1 = 0
 *       while p < seg_len[s] and k < max_records:
 *           left = seg_len[s] - p
 *           if left < 4:  st = ONC_ERR_INCOMPLETE_HEADER; break
 *           h = be32(wire, seg_off[s] + p)
 *           if !(h >> 31): st = ONC_ERR_FRAGMENTED; break
 *           want = (h & 0x7FFFFFFF) + 4
 *           if left < want: st = ONC_ERR_INCOMPLETE_MESSAGE; aux0 = u32(left); aux1 = u32(want); break
 *           rec_start[k] = seg_off[s] + p; rec_len[k] = want; rec_seg[k] = s; k++; p += want
 *       seg_result[6s ..] = {first, k - first, p, st, aux0, aux1}
 *       needed += records this segment frames when max_records is unbounded
 *   result = {k, needed, number of segments whose st != ONC_OK}
 *
 *   rec_start[dev, max_records], rec_len[dev, max_records]: record k is
 *                     wire[rec_start[k], rec_start[k] + rec_len[k]) — the
 *                     extents onc_decode_extents takes. Records are ordered by
 *                     segment index, then by position in the segment.
 *   rec_seg[dev, max_records]: optional (may be NULL): the record's segment.
 *   seg_result[dev, 6 * nseg]: per segment {first, n, consumed, status, aux0,
 *                     aux1}: its records are [first, first + n), `consumed`
 *                     bytes of it are framed (the caller memmoves the rest to
 *                     the slot's start), and status says why it stopped there,
 *                     as onc_frame_stream's does. An empty segment gives
 *                     {first, 0, 0, ONC_OK, 0, 0}. A stopped segment (cut tail,
 *                     fragmented mark, short header) affects nothing outside
 *                     its own row.
 *   result[dev, 3]  : {records framed, needed, segments whose status != ONC_OK}.
 *                     `needed` = the records framed with unbounded
 *                     max_records: the capacity a retry needs.
 * Once max_records is reached, the segment being framed ends with status
 * ONC_OK and its `consumed` is the start of its first unframed record; every
 * later segment is {max_records, 0, 0, ONC_OK, 0, 0} (the caller's loop never
 * looked at it). nseg == 0 or max_records == 0 writes a zero `result` and
 * zeroes every seg_result row (first = 0). Entries of rec_start / rec_len /
 * rec_seg at or past result[0] are not written. Asynchronous on the codec's
 * stream.
 * Memory access: only record marks are read — the aligned dwords holding the
 * 4 bytes at each record start of a segment, never a byte of a payload and
 * never an aligned dword without a segment byte — so framing a mapped host
 * slab costs one small read per record (two for a segment of more than 16
 * records, whose chain the write pass follows again).
 * Kernels (streams.hip): every segment start is a certain record start, so
 * there is no guess, no verification and no walk: a lane follows each
 * segment's exact chain (onc_frame_stream's chase), the segments' record
 * counts are scanned by onc_scan_lengths' launches, and a write pass fills
 * the outputs — coalesced from the record lengths the chase kept (segments of
 * up to 16 records), by a second chase otherwise. The design point is many
 * segments of up to about a frame chunk (64 KiB) each; a longer segment is
 * still exact but is followed serially by one lane: for one long stream use
 * onc_frame_stream. A fragmented segment only reports ONC_ERR_FRAGMENTED in
 * its row: the rests {seg_off + consumed, seg_len - consumed} of all such
 * rows go through onc_frame_fragment_streams + onc_defragment_extents in one
 * call each (or one segment's rest through onc_frame_fragments +
 * onc_defragment).
 * Scratch: 96 bytes per segment (and 4 per 16 segments), covered by
 * onc_codec_reserve(max_records >= nseg) — after it the call allocates
 * nothing; growing it while the stream is capturing is ONC_RC_ECAPTURE. */
int onc_frame_streams(onc_codec* codec, const uint8_t* wire,
                      const uint64_t* seg_off, const uint64_t* seg_len, uint64_t nseg, /* [dev, nseg] each */
                      uint64_t* rec_start, uint32_t* rec_len, uint32_t* rec_seg,       /* [dev, max_records]; rec_seg optional */
                      uint64_t max_records,
                      uint64_t* seg_result /* [dev, 6 * nseg] */, uint64_t* result /* [dev, 3] */);

/* Rebuild framed fragments as the packed stream of single-fragment records
 * that RpcMessage::serialise_into writes (one mark with the last-fragment bit
 * and the total length, rpc_message.rs:156, then the body), so that
 * onc_frame_stream, onc_decode and everything after them apply unchanged.
 * Fragment j is wire[frag_off[j], frag_off[j+1]): a 4-byte mark, read only
 * for bit 31, and a body. The offsets are trusted, as in onc_decode (they
 * come from onc_frame_fragments). Record r is the run of fragments ending at
 * the r-th fragment with bit 31 set; B_r = the sum of its bodies' lengths.
 *   rec_off[dev, nfrag + 1]: rec_off[0] = 0; a record takes 4 + B_r bytes; a
 *                     record with B_r >= 2^31 takes none and gets
 *                     ONC_ENC_TOO_LONG (the mark cannot say it:
 *                     rpc_message.rs:146-151). Placement ignores out_cap, so
 *                     rec_off[n_records] is the capacity the batch needs.
 *   out[dev]        : an OK record is BE32(0x80000000 | B_r), then its
 *                     fragments' bodies in order. A record that would end
 *                     beyond out_cap gets ONC_ENC_WRITE_ZERO and none of its
 *                     bytes are written. Any byte address (as onc_encode);
 *                     no byte before out, at or after out + out_cap, or
 *                     outside an OK record's extent is written. out must not
 *                     overlap wire.
 *   status[dev, nfrag]: per record, ONC_OK / ONC_ENC_TOO_LONG / ONC_ENC_WRITE_ZERO.
 *   result[dev, 6]  : {n_records, wire_consumed, out_bytes, pending_frags,
 *                     pending_body_bytes, n_multi}. Fragments after the last
 *                     one with bit 31 set belong to no complete record: they
 *                     are not emitted, only counted (pending_*);
 *                     wire_consumed = frag_off[first pending fragment], or
 *                     frag_off[nfrag]; out_bytes = rec_off[n_records];
 *                     n_multi = records of more than one fragment.
 * Entries of rec_off past n_records and of status from n_records on are not
 * written. nfrag == 0 gives rec_off[0] = 0 and a zero result. Zero-length
 * fragments are legal anywhere; an empty record is the bare mark 80 00 00 00.
 * Wire reads follow onc_decode's rule: only whole aligned 16-byte granules
 * that hold fragment bytes. Asynchronous on the codec's stream. Scratch: 32
 * bytes per fragment, covered by onc_codec_reserve(max_records >= nfrag);
 * growing it inside a capture is ONC_RC_ECAPTURE.
 * Kernels (defrag.hip): a plan over fragments (a scan of body bytes and
 * last-fragment bits, then onc_scan_lengths of the record lengths) and a
 * copy partitioned by output bytes. SURVEY §8(f) rank 1. */
int onc_defragment(onc_codec* codec, const uint8_t* wire, const uint64_t* frag_off, uint64_t nfrag,
                   uint8_t* out, uint64_t out_cap,
                   uint64_t* rec_off /*[dev, nfrag + 1]*/, int32_t* status /*[dev, nfrag]*/,
                   uint64_t* result /*[dev, 6]*/);

/* onc_frame_streams at fragment level: the fragments of many connections'
 * buffers in one call (RFC 5531 §11; the reference rejects such records:
 * Error::Fragmented, rpc_message.rs:359-362). Per segment the fragment chain
 * is followed as onc_frame_fragments follows it, and the fragments of the
 * segment's complete records come out as scattered extents — what
 * onc_defragment_extents takes. The segments are onc_frame_streams': any
 * order, any alignment, overlapping allowed, trusted; seg_len[s] < 2^34 and
 * nseg < 2^32 are preconditions (nseg >= 2^32 is ONC_RC_EINVAL). Fragment k
 * is wire[frag_start[k], frag_start[k] + frag_len[k]), its mark included
 * (frag_len >= 4; the largest value, 0x80000003, fits 32 bits). Only
 * fragments of complete records are emitted — a record is complete when its
 * run of fragments ends inside the segment with a mark whose bit 31 is set —
 * so every emitted run ends with a last fragment and no record spans two
 * segments. The result is exactly that of
 *
 *   k = r = needed = stopped = 0; full = false
 *   for s in 0 .. nseg-1:
 *       if full: seg_result[8s ..] = {max_frags, 0, 0, ONC_OK, 0, 0, 0, 0}
 *                (still add this segment's complete-record fragments to needed); continue
 *       # the walk: max_frags does not enter it
 *       p = 0; st = ONC_OK; aux0 = aux1 = 0; open = []; recs = []
 *       while p < seg_len[s]:
 *           left = seg_len[s] - p
 *           if left < 4: st = ONC_ERR_INCOMPLETE_HEADER; break
 *           h = be32(wire, seg_off[s] + p); want = (h & 0x7FFFFFFF) + 4
 *           if left < want: st = ONC_ERR_INCOMPLETE_MESSAGE; aux0 = u32(left); aux1 = u32(want); break
 *           open.append((p, want)); p += want
 *           if h >> 31: recs.append(open); open = []
 *       needed += fragments in recs                 # `open` (the pending run) is never emitted nor counted
 *       # the commit: whole records while they fit
 *       first = k; first_rec = r; consumed = 0; cut = false
 *       for R in recs:
 *           if len(R) > max_frags - k: cut = full = true; break
 *           for (fp, fl) in R: frag_start[k] = seg_off[s] + fp; frag_len[k] = fl; frag_seg[k] = s; k++
 *           r++; consumed = end of R
 *       seg_result[8s ..] = {first, k - first, consumed, cut ? ONC_OK : st, cut ? 0 : aux0, cut ? 0 : aux1, first_rec, r - first_rec}
 *       stopped += (row status != ONC_OK)
 *   result = {k, needed, r, stopped}
 *
 *   frag_start[dev, max_frags], frag_len[dev, max_frags]: the extents, ordered
 *                     by segment index, then by position in the segment.
 *   frag_seg[dev, max_frags]: optional (may be NULL): the fragment's segment.
 *   seg_result[dev, 8 * nseg]: per segment {first, n, consumed, status, aux0,
 *                     aux1, first_rec, n_rec}: its fragments are [first,
 *                     first + n), they make the records [first_rec, first_rec +
 *                     n_rec) of onc_defragment_extents' output, and `consumed`
 *                     bytes of it are done with: the end of its last emitted
 *                     record.
 *   result[dev, 4]  : {fragments emitted, needed, records emitted, segments
 *                     whose status != ONC_OK}. `needed` = the fragments emitted
 *                     with unbounded max_frags: the capacity a retry needs.
 * ONC_ERR_FRAGMENTED is never reported. A segment that ends on a fragment
 * boundary in the middle of a record has status ONC_OK and consumed <
 * seg_len: the caller moves [consumed, seg_len) down and waits for the rest,
 * as it does for a cut tail (INCOMPLETE_MESSAGE / INCOMPLETE_HEADER, whose
 * pending run is not emitted either). A stopped or pending segment affects
 * nothing outside its own row. The segment at which the capacity runs out
 * emits its records while they fit whole and has status ONC_OK; the segments
 * after it get the row {max_frags, 0, 0, ONC_OK, 0, 0, 0, 0}, because the
 * caller's loop never looked at them. nseg == 0 or max_frags == 0 writes a
 * zero `result` and zero rows. Entries of frag_start / frag_len / frag_seg at
 * or past result[0] are not written. Zero-length fragments and bare last
 * marks (80 00 00 00: an empty record) are legal anywhere. Asynchronous on
 * the codec's stream.
 * Memory access follows onc_frame_streams' rule: only the aligned dwords
 * holding a mark are read — no fragment body byte, and no dword without a
 * segment byte (two reads per mark for a segment with more than 16 fragments
 * in complete records, whose chain the write pass follows again).
 * Use: onc_frame_streams on the slab first — single-fragment peers stay on
 * the in-place path, nothing copied; for every row with ONC_ERR_FRAGMENTED put
 * {seg_off + consumed, seg_len - consumed} into a second segment list, run
 * this call and onc_defragment_extents on that list, then onc_decode on the
 * rebuilt stream. A list of all connections is legal too: a single-fragment
 * record is a one-fragment record.
 * Kernels (streams.hip): onc_frame_streams' structure, every segment start
 * being a certain fragment start — a lane follows each segment's chain and
 * commits at every last fragment, the segments' fragment and record counts
 * are scanned by onc_scan_lengths' launches (twice), and a write pass fills
 * the outputs, coalesced from the marks the chase kept or by a second chase.
 * The argument checks and ONC_RC_ECAPTURE are onc_frame_streams'. Scratch:
 * 108 bytes per segment (and 4 per 16 segments), in onc_frame_streams'
 * buffer, covered by onc_codec_reserve(max_records >= nseg). */
int onc_frame_fragment_streams(onc_codec* codec, const uint8_t* wire,
                               const uint64_t* seg_off, const uint64_t* seg_len, uint64_t nseg, /* [dev, nseg] each */
                               uint64_t* frag_start, uint32_t* frag_len, uint32_t* frag_seg,    /* [dev, max_frags]; frag_seg optional */
                               uint64_t max_frags,
                               uint64_t* seg_result /* [dev, 8 * nseg] */, uint64_t* result /* [dev, 4] */);

/* onc_defragment for fragments that are not back to back (it relates to
 * onc_defragment as onc_decode_extents relates to onc_decode): fragment j is
 * wire[frag_start[j], frag_start[j] + frag_len[j]), its mark included —
 * onc_frame_fragment_streams' outputs, in any address order. With C = the
 * concatenation of the fragments in order and frag_off = the prefix sums of
 * frag_len, `out`, rec_off and status are those of onc_defragment(C,
 * frag_off, nfrag, ...), and so is result, except that result[1] is the
 * number of fragments consumed (nfrag - pending_frags) instead of a byte
 * offset. Everything else is onc_defragment's: the extents are trusted
 * (frag_len >= 4 is a precondition); trailing fragments without a last mark
 * are counted, not emitted; out may be any byte address and must not overlap
 * the fragments; nothing is written outside the OK records' extents;
 * ONC_ENC_TOO_LONG and ONC_ENC_WRITE_ZERO apply as there; wire reads are
 * limited to the whole aligned 16-byte granules that hold fragment bytes;
 * nfrag == 0 gives rec_off[0] = 0 and a zero result. Scratch: 32 bytes per
 * fragment, covered by onc_codec_reserve(max_records >= nfrag); timing ids
 * ONC_K_DEFRAG_PLAN / ONC_K_DEFRAG_COPY. The output is the packed stream plus
 * rec_off: onc_decode and everything after it apply unchanged. */
int onc_defragment_extents(onc_codec* codec, const uint8_t* wire,
                           const uint64_t* frag_start, const uint32_t* frag_len, uint64_t nfrag,
                           uint8_t* out, uint64_t out_cap,
                           uint64_t* rec_off /*[dev, nfrag + 1]*/, int32_t* status /*[dev, nfrag]*/,
                           uint64_t* result /*[dev, 6]*/);

/* The heads of fragmented records: what a decoder needs from a reassembled
 * record — its synthesised mark and its first bytes, contiguous, and its
 * true length — without moving a payload byte (the receive-side counterpart
 * of onc_fragment_iov; the reference's decode borrows the payload,
 * call_body.rs:53-59). The fragments are onc_defragment_extents': fragment j
 * is wire[frag_start[j], frag_start[j] + frag_len[j]), mark included,
 * frag_len >= 4, in any address order, overlaps allowed; the extents are
 * trusted and the mark is read only for bit 31. Record r's head goes to the
 * fixed-stride slot heads + r * head_len; the rest of the record stays where
 * it arrived and is located by rec_frag / frag_pre. The result is exactly
 * that of this loop:
 *
 *   r = first = 0; B = 0; multi = 0
 *   for j in 0 .. nfrag-1:
 *       frag_pre[j] = B                          # body bytes of its record before fragment j (pending fragments too)
 *       B += frag_len[j] - 4
 *       if wire[frag_start[j]] & 0x80:           # last fragment: record r = fragments [first, j]
 *           rec_frag[r] = first
 *           if B >= 2^31: rec_len[r] = 0; status[r] = ONC_ENC_TOO_LONG
 *           else:
 *               rec_len[r] = 4 + B
 *               status[r] = r < max_records ? ONC_OK : ONC_ENC_WRITE_ZERO
 *               if OK: slot = heads + r * head_len
 *                      slot[0, 4) = BE32(0x80000000 | B)
 *                      slot[4, min(4 + B, head_len)) = the first bytes of the bodies of fragments first..j, concatenated
 *           multi += (j > first); r++; first = j + 1; B = 0
 *   rec_frag[r] = first
 *   result = {r, first, r * head_len, nfrag - first, B, multi}
 *
 * Agreement with the packed form: slot r holds byte for byte the first
 * min(rec_len[r], head_len) bytes of record r in onc_defragment_extents'
 * output, rec_len[r] is rec_off[r+1] - rec_off[r] there, and result[0, 1, 3,
 * 4, 5] are that call's; result[2] is the heads capacity, in bytes, that the
 * batch needs. Nothing is written in a slot past min(rec_len[r], head_len),
 * in the slot of a record that is not OK, in heads at or past max_records *
 * head_len, in rec_len / status from r on, or in rec_frag past r.
 * head_len is a multiple of 16 in [64, 4096], else ONC_RC_EINVAL; heads must
 * be 16-byte aligned, else ONC_RC_EALIGN. NULL codec, rec_frag or result is
 * ONC_RC_EINVAL whatever nfrag is; with nfrag > 0 so is a NULL wire,
 * frag_start, frag_len, rec_len, frag_pre or status; NULL heads with
 * max_records > 0 is ONC_RC_EINVAL. nfrag == 0 gives rec_frag[0] = 0 and a
 * zero result and needs nothing else.
 * Reads: only the whole aligned 16-byte granules of the wire that hold a
 * mark or one of the head bytes copied; no byte of a record at body position
 * >= head_len - 4 is read, so framing-only extents over a mapped host slab
 * stay cheap.
 * Locating the payload: record byte p >= 4 of record r is body byte p - 4; it
 * lies in the last fragment j in [rec_frag[r], rec_frag[r+1]) with
 * frag_pre[j] <= p - 4, at wire[frag_start[j] + 4 + (p - 4 - frag_pre[j])] —
 * no piece list is needed.
 * Asynchronous on the codec's stream; every step is a kernel launch (no
 * memset), so a captured call is a chain of kernel nodes. Scratch is
 * onc_defragment's buffer, no more than 32 bytes per fragment, covered by
 * onc_codec_reserve(max_records >= nfrag); growing it inside a capture is
 * ONC_RC_ECAPTURE. Timing ids: the plan launches report under
 * ONC_K_DEFRAG_PLAN, the gather under ONC_K_DEFRAG_COPY. */
int onc_defragment_heads(onc_codec* codec, const uint8_t* wire,
                         const uint64_t* frag_start, const uint32_t* frag_len, uint64_t nfrag,
                         uint32_t head_len,
                         uint8_t* heads, uint64_t max_records,
                         uint32_t* rec_len  /*[dev, nfrag]*/,
                         uint64_t* rec_frag /*[dev, nfrag + 1]*/,
                         uint64_t* frag_pre /*[dev, nfrag]*/,
                         int32_t* status    /*[dev, nfrag]*/,
                         uint64_t* result   /*[dev, 6]*/);

/* The send side of RFC 5531 §11, the exact inverse of onc_defragment: every
 * record of a packed stream cut into fragments of at most max_frag body
 * bytes, as a sender that flushes through a bounded buffer writes them, or
 * as a peer that caps the fragment size needs them. Record i is
 * wire[rec_off[i], rec_off[i+1]): a single-fragment record as onc_encode,
 * onc_defragment and onc_frame_stream delimit them. The extents are trusted,
 * as in onc_decode; rec_off[0] may be any base. The record's own mark is
 * never read: its body is the extent without its first four bytes,
 * B = extent - 4. The result is exactly that of
 *
 *   pos = 0; nf = 0; multi = 0
 *   for i in 0 .. n-1:
 *       out_off[i] = pos; L = rec_off[i+1] - rec_off[i]
 *       if L == 0: status[i] = ONC_OK; continue                  # a failing record's empty extent: nothing to send
 *       if L < 4:  status[i] = ONC_ENC_BAD_DESCRIPTOR; continue  # no room for a mark; takes no bytes
 *       B = L - 4; k = max(1, ceil(B / max_frag)); len = 4*k + B
 *       status[i] = (pos <= out_cap and len <= out_cap - pos) ? ONC_OK : ONC_ENC_WRITE_ZERO
 *       if OK: fragment j < k-1 = BE32(max_frag) ++ body[j*max_frag, +max_frag)
 *              fragment k-1     = BE32(0x80000000 | (B - (k-1)*max_frag)) ++ the rest
 *                                 (B == 0: the bare mark 80 00 00 00)
 *       pos += len; nf += k; multi += (k > 1)                    # placement ignores out_cap, as onc_defragment
 *   out_off[n] = pos; result = {nf, pos, multi}
 *
 *   max_frag        : the largest fragment body, 1 .. 0x7FFFFFFF (anything
 *                     else is ONC_RC_EINVAL). With 0x7FFFFFFF and every
 *                     B < 2^31 the output is the input byte for byte.
 *   out_off[dev, n + 1]: where record i's fragments start in out;
 *                     out_off[n] is the capacity the batch needs.
 *   out[dev]        : any byte address (as onc_encode); must not overlap
 *                     wire. A record that gets ONC_ENC_WRITE_ZERO writes none
 *                     of its bytes, and neither does any record after it. No
 *                     byte before out, at or after out + out_cap, or outside
 *                     an OK record's extent is written.
 *   status[dev, n]  : ONC_OK / ONC_ENC_BAD_DESCRIPTOR / ONC_ENC_WRITE_ZERO.
 *   result[dev, 3]  : {fragments, out bytes (= out_off[n]), records of more
 *                     than one fragment}; both counts include records beyond
 *                     the capacity.
 * B is not limited: this is how a body of 2^31 bytes or more, which
 * serialise_into refuses (rpc_message.rs:146-151) and onc_defragment cannot
 * write, gets sent at all. len can exceed 2^32 (max_frag = 1 gives 5 B), so
 * bytes and fragments are scanned in 64 bits, not by onc_scan_lengths.
 * Placeholders (failing records that keep an extent, ABI 7) are framable
 * records and are fragmented like any other; a caller that wants the
 * reference's stream runs onc_compact first.
 * n == 0 gives out_off[0] = 0 and a zero result, and needs no wire, rec_off,
 * status or out. Wire reads follow onc_decode's rule: only whole aligned
 * 16-byte granules that hold bytes of a record with an extent of at least 4
 * bytes. Asynchronous on the codec's stream. Scratch: under 32 bytes per
 * record (8, and 24 per 256 records), whatever max_frag and the number of
 * fragments are, in onc_defragment's buffer: onc_codec_reserve(max_records
 * >= n) covers it; growing it inside a capture is ONC_RC_ECAPTURE.
 * Kernels (fragment.hip): a plan over records (one 64-bit scan of {bytes,
 * fragments, multi}) and a copy partitioned by output bytes in which
 * fragment j of a record stands at the closed-form position j * (max_frag +
 * 4): no per-fragment table and no search among fragments. */
int onc_fragment(onc_codec* codec, const uint8_t* wire, const uint64_t* rec_off, uint64_t n,
                 uint32_t max_frag,
                 uint8_t* out, uint64_t out_cap,
                 uint64_t* out_off /*[dev, n + 1]*/, int32_t* status /*[dev, n]*/,
                 uint64_t* result /*[dev, 3]*/);

/* onc_fragment for the vectored encode: the records of onc_encode_iov's (or
 * onc_compact_iov's) list cut into fragments without a byte being copied.
 * Fragmenting a vectored record needs no wire byte: its own mark is never
 * read, every fragment mark is a function of the entry's two lengths and the
 * limit, and every fragment body is one or two slices of memory that already
 * exists. So the call reads only the entries of `iov` (never hdr_out or the
 * payload arena, to which it takes no pointer; wire_off is ignored; the
 * entries are trusted, as onc_fragment trusts rec_off) and writes 4 bytes per
 * fragment into `marks` and a list of 16-byte pieces: gathering the pieces
 * in order (a writev() list) is the fragmented stream. The result is exactly
 * that of
 *
 *   pos = nf = multi = np = 0
 *   for i in 0 .. n-1:
 *       out_off[i] = pos; piece_off[i] = np
 *       hl = iov[i].hdr_len; pl = iov[i].payload_len; L = hl + pl            # 64-bit
 *       F = rec_max_frag ? rec_max_frag[i] : max_frag
 *       if L == 0: status[i] = ONC_OK; continue                              # a failing record: nothing to send
 *       if hl < 4 or F < 1 or F > 0x7FFFFFFF: status[i] = ONC_ENC_BAD_DESCRIPTOR; continue   # takes nothing
 *       Hb = hl - 4; B = L - 4; k = max(1, ceil(B / F))
 *       x = (Hb % F != 0 and pl > 0) ? 1 : 0                                 # one fragment holds header bytes, then payload bytes
 *       e = (B == 0) ? 1 : 2k + x                                            # pieces of this record
 *       fits = np <= max_pieces and e <= max_pieces - np and 4nf <= marks_cap and 4k <= marks_cap - 4nf
 *       status[i] = fits ? ONC_OK : ONC_ENC_WRITE_ZERO
 *       if fits: for j in 0 .. k-1:   [a, b) = [jF, min((j+1)F, B))
 *           marks[4(nf+j) ..] = BE32((j == k-1 ? 0x80000000 : 0) | (b - a))
 *           piece {MARK, 4(nf+j), 4}
 *           if a < Hb and b > a:  piece {HDR, iov[i].hdr_off + 4 + a, min(b, Hb) - a}
 *           if b > Hb and pl > 0: s = max(a, Hb); piece {PAYLOAD, iov[i].payload_off + s - Hb, b - s}
 *       pos += 4k + B; nf += k; multi += (k > 1); np += e                    # placement ignores both capacities
 *   out_off[n] = pos; piece_off[n] = np; result = {nf, pos, multi, np}
 *
 * A piece {src, off, len} is `len` bytes at byte `off` of `marks`
 * (ONC_PIECE_MARK), of onc_encode_iov's hdr_out (ONC_PIECE_HDR) or of the
 * batch's payload arena (ONC_PIECE_PAYLOAD); record i's pieces are
 * pieces[piece_off[i], piece_off[i+1]) and stand for the stream bytes
 * [out_off[i], out_off[i+1]).
 *  - Equivalence with the packed path: when everything fits, the gathered
 *    pieces are, byte for byte, what onc_fragment writes for onc_encode's
 *    packed output of the same batch at the same max_frag; out_off, status
 *    and result[0..2] are onc_fragment's.
 *  - Capacity cut: placements only grow and a record that takes pieces also
 *    takes marks, so the first ONC_ENC_WRITE_ZERO record and everything
 *    after it write nothing. No piece at or past max_pieces is written and no
 *    byte of marks at or past marks_cap.
 *  - Needed capacities: result[3] pieces and 4 * result[0] bytes of marks
 *    (a call with both capacities 0 is the plan alone).
 *  - Zero-length pieces are never emitted. A placeholder (ABI 7) is a record
 *    like any other; onc_compact_iov first gives the reference's stream.
 *  - rec_max_frag[dev, n] (optional): a limit per record. NULL means the
 *    uniform max_frag; when it is given max_frag is ignored but must still be
 *    valid. A record whose own value is outside 1 .. 0x7FFFFFFF is
 *    ONC_ENC_BAD_DESCRIPTOR and its neighbours are unaffected.
 *  - ONC_RC_EINVAL: a NULL codec, out_off, piece_off or result; max_frag
 *    outside 1 .. 0x7FFFFFFF; with n > 0 a NULL iov or status, NULL marks with
 *    marks_cap > 0, NULL pieces with max_pieces > 0. ONC_RC_EALIGN: marks not
 *    4-byte aligned or pieces not 16-byte aligned. n == 0 gives a zero result
 *    and out_off[0] = piece_off[0] = 0 and needs nothing else.
 * marks and pieces must not overlap iov, rec_max_frag or each other.
 * All counts are 64 bits wide (hdr_len = payload_len = 0xFFFFFFFF at
 * max_frag 1 is 2^33 fragments and 2^34 pieces). Asynchronous on the codec's
 * stream. Scratch: under 32 bytes per record (16, and 32 per 256 records), in
 * onc_defragment's buffer: onc_codec_reserve(max_records >= n) covers it;
 * growing it inside a capture is ONC_RC_ECAPTURE. The three plan launches
 * report under ONC_K_DEFRAG_PLAN and the fill under ONC_K_DEFRAG_COPY.
 * Kernels (fragment_iov.hip): onc_fragment's plan with a fourth sum (pieces),
 * and a fill partitioned by output pieces: a lane writes whole 16-byte pieces
 * (and the mark of a MARK piece), its record found in a window of the sorted
 * piece prefix staged in LDS, the piece's place inside the record by closed
 * form (fragment_iov_plan.h): no per-fragment table and no search. */
#define ONC_PIECE_MARK    0u   /* off: byte offset into `marks` */
#define ONC_PIECE_HDR     1u   /* off: byte offset into onc_encode_iov's hdr_out */
#define ONC_PIECE_PAYLOAD 2u   /* off: byte offset into the batch's payload arena */
typedef struct onc_frag_piece {
    uint64_t off;
    uint32_t len;
    uint32_t src;
} onc_frag_piece;   /* 16 bytes */

int onc_fragment_iov(onc_codec* codec, const onc_iov_rec* iov, uint64_t n,
                     uint32_t max_frag, const uint32_t* rec_max_frag /*[dev, n], optional*/,
                     uint8_t* marks, uint64_t marks_cap /*bytes*/,
                     onc_frag_piece* pieces, uint64_t max_pieces,
                     uint64_t* out_off /*[dev, n + 1]*/, uint64_t* piece_off /*[dev, n + 1]*/,
                     int32_t* status /*[dev, n]*/, uint64_t* result /*[dev, 4]*/);

/* A piece list written as one stream on the device: what a writev() of the
 * pieces sends, gathered straight from the three sources into one contiguous
 * buffer, a window of the stream at a time — each payload byte moves once,
 * where onc_encode + onc_fragment move it twice. The stream is the pieces back
 * to back; piece i is pieces[i].len bytes at byte pieces[i].off of source
 * pieces[i].src (ONC_PIECE_MARK / _HDR / _PAYLOAD index base[] and len[]). Any
 * list is accepted, not only onc_fragment_iov's: pieces of no bytes anywhere
 * (long runs of them too), pieces that repeat, overlap and stand in any source
 * order. A piece is OK when it lies inside its source,
 *
 *   ok(p) = p.len == 0 or (p.src <= 2 and p.off <= len[p.src] and p.len <= len[p.src] - p.off)
 *
 * (no sum is formed: off + len may wrap near 2^64), and bad otherwise. A bad
 * piece keeps its place in the stream but is never read: its bytes of `out`
 * are left as they were and its neighbours are unaffected.
 *
 * onc_piece_offsets: where every piece starts in the stream, and the bad ones
 * counted. The result is exactly that of
 *
 *   pos = bad = 0; first_bad = npieces
 *   for i in 0 .. npieces-1:
 *       piece_pos[i] = pos
 *       if !ok(pieces[i]): bad += 1; first_bad = min(first_bad, i)
 *       pos += pieces[i].len
 *   piece_pos[npieces] = pos; result = {pos, bad, first_bad}
 *
 * onc_gather_pieces: stream bytes [from, from + count) into out[0, count), as
 * far as the stream goes. The result is exactly that of
 *
 *   end = from + count                                   # 64-bit, saturating
 *   for i in 0 .. npieces-1:
 *       a = max(piece_pos[i], from); b = min(piece_pos[i] + pieces[i].len, end)
 *       if a < b and ok(pieces[i]):
 *           out[a - from, b - from) = base[src_i][off_i + (a - piece_pos[i]), off_i + (b - piece_pos[i]))
 *
 *   src[host]       : the three sources' device addresses and lengths, read
 *                     by the call itself (not by the kernels). base[k] may be
 *                     NULL when len[k] is 0.
 *   piece_pos[dev, npieces + 1]: onc_piece_offsets writes it, onc_gather_pieces
 *                     reads it (as written for the same pieces and sources; it
 *                     is trusted). 8-byte aligned; pieces 16-byte aligned.
 *   result[dev, 3]  : {stream bytes (= piece_pos[npieces]), bad pieces, index
 *                     of the first bad piece (npieces: none)}.
 *   out[dev]        : any byte address (as onc_encode), device memory or
 *                     mapped host memory (a send buffer); must not overlap the
 *                     sources, pieces or piece_pos. No byte before out, at or
 *                     after out + count, or at or past stream position
 *                     piece_pos[npieces] is written. Whole aligned 16-byte
 *                     chunks of out that lie inside one OK piece go with one
 *                     load and one store; the ends of the window and chunks
 *                     that span pieces are resolved byte by byte (such a
 *                     chunk is still stored at once when all 16 of its bytes
 *                     are written).
 * Source reads follow onc_decode's rule: only whole aligned 16-byte granules
 * that hold bytes of an OK piece inside the window, so a mapped host source
 * stays cheap. The stream must be shorter than 2^64 bytes.
 *  - ONC_RC_EINVAL: a NULL codec, src or piece_pos; a NULL result
 *    (onc_piece_offsets); NULL pieces with npieces > 0; NULL out with
 *    count > 0 (onc_gather_pieces); a source with len > 0 and a NULL base.
 *    ONC_RC_EALIGN: pieces not 16-byte aligned or piece_pos not 8-byte aligned.
 *  - npieces == 0 gives piece_pos[0] = 0 and the result {0, 0, 0}, and a gather
 *    that writes nothing; count == 0 writes nothing.
 * Both calls are asynchronous on the codec's stream and every step is a kernel
 * launch (no memset or memcpy node in a captured call). Scratch:
 * onc_piece_offsets keeps its block sums (24 bytes per 256 pieces: under 1
 * byte per piece) in onc_defragment's buffer: onc_codec_reserve(max_records
 * >= npieces) covers it; growing it inside a capture is ONC_RC_ECAPTURE.
 * onc_gather_pieces uses none. The offsets' launches report under
 * ONC_K_DEFRAG_PLAN and the gather under ONC_K_DEFRAG_COPY.
 * Kernels (gather.hip): onc_fragment's plan shape (block sums, one-workgroup
 * scan, apply) over {bytes, bad, first bad}, and onc_defragment's copy with
 * three source bases and no mark: partitioned by output bytes (a wave per
 * 8 KiB tile of the window), the pieces reaching into a tile staged in LDS. */
typedef struct onc_gather_src {          /* indexed by ONC_PIECE_MARK / _HDR / _PAYLOAD */
    const uint8_t* base[3];              /* [dev]; may be NULL when len is 0 */
    uint64_t       len[3];               /* bytes in each source */
} onc_gather_src;

int onc_piece_offsets(onc_codec* codec, const onc_frag_piece* pieces, uint64_t npieces,
                      const onc_gather_src* src /*host*/,
                      uint64_t* piece_pos /*[dev, npieces + 1]*/, uint64_t* result /*[dev, 3]*/);

int onc_gather_pieces(onc_codec* codec, const onc_frag_piece* pieces, const uint64_t* piece_pos,
                      uint64_t npieces, const onc_gather_src* src /*host*/,
                      uint64_t from, uint64_t count, uint8_t* out);

/* Decoded payloads placed in aligned slots on the device: the receive-side
 * counterpart of onc_gather_pieces. After onc_defragment_heads +
 * onc_decode_heads every payload still lies scattered over its record's
 * fragments in the caller's receive slab, and after onc_frame_streams +
 * onc_decode_extents at an arbitrary byte address of it; these two calls move
 * each payload byte exactly once, from where it arrived to an aligned slot of
 * a caller's buffer (an NFS WRITE body for storage, the arguments of a GPU
 * kernel), after which the slab can be reused. A decoded batch then re-encodes
 * with msgs_out as the descriptors, auth_arena = the heads (or the wire) and
 * payload_arena = the placed buffer.
 *
 * onc_payload_slots: where each decoded record's payload is, and where it
 * goes. The result is exactly that of
 *
 *   off = k = bytes = 0
 *   for r in 0 .. n-1:
 *       m = msgs[r]
 *       has = status[r] == ONC_OK and m.payload_len > 0 and
 *             (m.msg_type == ONC_MSG_CALL or
 *              (m.msg_type == ONC_MSG_REPLY and m.reply_stat == ONC_REPLY_ACCEPTED and m.stat == ONC_ACCEPT_SUCCESS))
 *       base = rec_start ? rec_start[r] : r * head_len      # onc_decode_extents' offsets | onc_decode_heads'
 *       pay_pos[r] = has ? u32(m.payload_off - base) : 0    # position in the record, mark included (>= 4)
 *       pay_len[r] = has ? m.payload_len : 0
 *       slot_off[r] = off
 *       if msgs_out: msgs_out[r] = m, with payload_off = off when has
 *       off += round_up(pay_len[r], align); k += has; bytes += pay_len[r]
 *   slot_off[n] = off; result = {k, bytes, off}
 *
 *   msgs, status[dev, n]: a decode's descriptors and statuses. The payload
 *                     words of a record that is not OK, or of a message kind
 *                     that carries no payload, are ignored.
 *   rec_start[dev, n]: the extents onc_decode_extents decoded; NULL: the heads
 *                     form, record r's offsets count from r * head_len
 *                     (head_len as in onc_decode_heads: a multiple of 16 in
 *                     [64, 4096]). head_len is ignored with rec_start.
 *   align           : a power of two in [1, 2^20]; every slot starts at a
 *                     multiple of it.
 *   msgs_out[dev, n]: optional; may be msgs itself.
 *   result[dev, 3]  : {records with a payload, payload bytes, the capacity
 *                     the destination needs (= slot_off[n])}.
 *  - ONC_RC_EINVAL: a NULL codec, result or slot_off, an align that is not a
 *    power of two in [1, 2^20], or (with rec_start NULL) a bad head_len,
 *    whatever n is; with n > 0 a NULL msgs, status, pay_pos or pay_len.
 *    ONC_RC_EALIGN: msgs or msgs_out not 16-byte aligned, slot_off not 8-byte
 *    aligned. n == 0 gives slot_off[0] = 0 and a zero result.
 *
 * onc_place_payloads: the copy. The result is exactly that of
 *
 *   for r in 0 .. n-1:
 *       if pay_len[r] == 0: continue
 *       ok = pay_pos[r] >= 4 and pay_pos[r] <= rec_len[r] and pay_len[r] <= rec_len[r] - pay_pos[r]
 *            and slot_off[r] <= dst_cap and pay_len[r] <= dst_cap - slot_off[r]     # no sum is formed
 *       if not ok: continue                                  # never read, nothing written
 *       for i in 0 .. pay_len[r]-1:
 *           x = pay_pos[r] - 4 + i
 *           j = rec_frag ? the last j in [rec_frag[r], rec_frag[r+1]) with frag_pre[j] <= x : r
 *           pre = rec_frag ? frag_pre[j] : 0
 *           dst[slot_off[r] + i] = wire[frag_start[j] + 4 + (x - pre)]
 *
 *   frag_start, frag_len[dev, nfrag]: onc_defragment_heads' inputs (the
 *                     caller's own extents, trusted); rec_frag[dev, n + 1],
 *                     frag_pre[dev, nfrag] and rec_len[dev, n] its outputs.
 *                     The identity form, rec_frag = frag_pre = NULL: record r
 *                     is fragment r — frag_start, frag_len and rec_len are
 *                     onc_frame_streams' rec_start, rec_len and rec_len again
 *                     (nfrag >= n).
 *   pay_pos, pay_len[dev, n]: any slice of the record's body, not only the
 *                     whole payload (the data of an NFS WRITE behind its
 *                     arguments), which is why it is checked against the
 *                     record.
 *   slot_off[dev, n]: trusted as piece_pos is in onc_gather_pieces: it is
 *                     non-decreasing, and slot_off[r] + pay_len[r] <=
 *                     slot_off[r+1] wherever pay_len[r] > 0 — what
 *                     onc_payload_slots writes; a caller's own list may leave
 *                     larger gaps. (slot_off[n] is not read.)
 *   dst[dev]        : any byte address, device memory or mapped host memory;
 *                     must not overlap the wire or any of the arrays. No byte
 *                     of dst is written outside the slices of OK records: the
 *                     padding between slots, the bytes before dst and those at
 *                     or after dst + dst_cap stay as they were.
 * Source reads follow onc_decode's rule: only whole aligned 16-byte granules
 * that hold bytes that are copied; no byte of a record outside its slice is
 * read and nothing of a skipped record.
 *  - ONC_RC_EINVAL: a NULL codec; a NULL rec_frag with a non-NULL frag_pre or
 *    the reverse; the identity form with nfrag < n; with n > 0 a NULL wire,
 *    frag_start, frag_len, rec_len, pay_pos, pay_len, slot_off or dst.
 *    n == 0 launches nothing.
 * Both calls are asynchronous on the codec's stream and every step is a kernel
 * launch (no memset or memcpy node in a captured call). Scratch:
 * onc_payload_slots keeps its block sums (24 bytes per 256 records: under 1
 * byte per record) in onc_defragment's buffer: onc_codec_reserve(max_records
 * >= n) covers it; growing it inside a capture is ONC_RC_ECAPTURE.
 * onc_place_payloads uses none. The slots' launches report under
 * ONC_K_DEFRAG_PLAN and the copy under ONC_K_DEFRAG_COPY.
 * Kernels (payload.hip): onc_fragment's plan shape (block sums, one-workgroup
 * scan, apply) over {slot bytes, records, payload bytes}, and
 * onc_gather_pieces' copy with one more level of lookup: partitioned by the
 * bytes of dst (a wave per 8 KiB tile), the records reaching into a tile
 * staged in LDS, the fragment of a body byte found by binary search of
 * frag_pre. All index arithmetic is 64-bit: frag_start, slot_off and the
 * extent of dst may exceed 2^32. */
int onc_payload_slots(onc_codec* codec, const onc_msg* msgs, const int32_t* status, uint64_t n,
                      uint32_t head_len, const uint64_t* rec_start /* NULL: the heads form */,
                      uint32_t align,
                      uint32_t* pay_pos  /*[dev, n]*/, uint32_t* pay_len /*[dev, n]*/,
                      uint64_t* slot_off /*[dev, n + 1]*/,
                      onc_msg* msgs_out  /*[dev, n], optional; may be msgs itself*/,
                      uint64_t* result   /*[dev, 3]*/);

int onc_place_payloads(onc_codec* codec, const uint8_t* wire,
                       const uint64_t* frag_start, const uint32_t* frag_len, uint64_t nfrag,
                       const uint64_t* rec_frag /*[dev, n + 1]; NULL: record r is fragment r*/,
                       const uint64_t* frag_pre /*[dev, nfrag]; NULL with rec_frag NULL*/,
                       const uint32_t* rec_len  /*[dev, n]*/,
                       const uint32_t* pay_pos, const uint32_t* pay_len, const uint64_t* slot_off, uint64_t n,
                       uint8_t* dst, uint64_t dst_cap);

/* ------------------------------------------------------------------------ */
/* Dispatch: decoded Calls to their handlers                                 */
/* ------------------------------------------------------------------------ */

/* A decode leaves n descriptors in arrival order: Calls of every program,
 * version and procedure the peers chose to send, a client's Replies, failed
 * records. Before any handler can run a server finds each Call's handler,
 * hands every handler its Calls as one contiguous batch, and answers the Calls
 * it does not serve as RFC 5531 §9 prescribes (the reference leaves that loop
 * to the application: CallBody::program / program_version / procedure, and
 * AcceptedStatus::ProgramUnavailable / ProgramMismatch{low, high} /
 * ProcedureUnavailable, src/reply/accepted_reply.rs). onc_route_calls is that
 * loop as one batch call on the device: it classifies every record against a
 * small route table, groups the records stably by handler and writes the reply
 * descriptors — complete for the Calls nobody serves, skeletons for the rest —
 * in an order onc_encode takes directly. Credential checks (AUTH_ERROR
 * rejections) and the matching of a client's Replies to its outstanding xids
 * are not part of it (the latter is onc_match_replies, below).
 *
 * A route: the procedures [proc_first, proc_first + proc_count) of one
 * (program, version). Procedure p goes to handler handler_first + (p -
 * proc_first), or to handler_first for every p with ONC_ROUTE_ONE_HANDLER. */
#define ONC_ROUTE_TABLE_MAX    1024u   /* entries */
#define ONC_ROUTE_HANDLERS_MAX 253u    /* so that handlers + 3 special bins <= 256 */
#define ONC_ROUTE_ONE_HANDLER  0x1u    /* flags: every procedure of the range goes to handler_first */

typedef struct onc_route {            /* 24 bytes */
    uint32_t program;
    uint32_t version;
    uint32_t proc_first;              /* procedures [proc_first, proc_first + proc_count) */
    uint32_t proc_count;
    uint32_t handler_first;
    uint32_t flags;                   /* ONC_ROUTE_*; other bits must be 0 */
} onc_route;

/* The nh + 3 bins: handler h < nh holds the OK Calls routed to it; then */
#define ONC_ROUTE_BIN_REJECTED(nh) ((uint32_t)(nh))        /* OK Calls that no route serves */
#define ONC_ROUTE_BIN_NOT_CALL(nh) ((uint32_t)(nh) + 1u)   /* OK records whose msg_type != ONC_MSG_CALL */
#define ONC_ROUTE_BIN_FAILED(nh)   ((uint32_t)(nh) + 2u)   /* records whose status != ONC_OK */
#define ONC_ROUTE_TILE 1024u   /* records per workgroup of the kernels (tests: the sizes around it) */

/* onc_route_calls. The result is exactly that of
 *
 *   valid(table): for every i:
 *       proc_count >= 1
 *       proc_first + proc_count <= 2^32
 *       (flags & ~1) == 0
 *       handler_first + (ONE_HANDLER ? 1 : proc_count) <= nh
 *     and for every i + 1 < ntab:
 *       (program, version, proc_first)[i] < [i+1] lexicographically, unsigned
 *       with equal (program, version): proc_first[i] + proc_count[i] <= proc_first[i+1]
 *   bad = the first i that breaks a rule of its own, or whose pair (i, i+1) breaks an order rule
 *   if bad exists:
 *       result = {0, 0, 0, bad + 1}; bin_first[0 .. nh+3] = 0
 *       route, order, calls_out and replies are not written; return
 *
 *   for r in 0 .. n-1:
 *       m = msgs[r]
 *       if   status[r] != ONC_OK:          bin = nh + 2          # the descriptor is not looked at
 *       elif m.msg_type != ONC_MSG_CALL:   bin = nh + 1
 *       else:
 *           e = the entry with program == m.program, version == m.program_version,
 *               proc_first <= m.procedure < proc_first + proc_count            # at most one
 *           if e:                      bin = handler of m.procedure by e; stat = ONC_ACCEPT_SUCCESS
 *           elif any entry has (m.program, m.program_version):
 *                                      bin = nh; stat = ONC_ACCEPT_PROC_UNAVAIL
 *           elif any entry has m.program:
 *                                      bin = nh; stat = ONC_ACCEPT_PROG_MISMATCH
 *                                      low / high = least / greatest version among that program's entries
 *           else:                      bin = nh; stat = ONC_ACCEPT_PROG_UNAVAIL
 *       route[r] = bin
 *
 *   order = the record indices sorted by route[], stably (ascending r inside a bin)
 *   bin_first[b] = number of records in bins < b, for b in 0 .. nh+3      # bin b is order[bin_first[b] .. bin_first[b+1])
 *   for k in 0 .. n-1:
 *       r = order[k]
 *       if calls_out: calls_out[k] = msgs[r]          # all 64 bytes, untouched, in every bin
 *       if replies:   replies[k] = all zero, unless r is an OK Call; then:
 *           xid = msgs[r].xid; msg_type = ONC_MSG_REPLY; reply_stat = ONC_REPLY_ACCEPTED; stat = stat above
 *           u.mismatch = {low, high, 0} for PROG_MISMATCH, else zero
 *           verf = AuthNone(None): id 0, kind_len ONC_AUTH_PACK(ONC_KIND_NONE, 0), ref 0
 *           cred zero; payload_len = payload_off = 0
 *   result = {Calls in handler bins, Calls in the rejected bin, records in the last two bins, 0}
 *
 *  - replies + bin_first[nh], count bin_first[nh+1] - bin_first[nh], is an
 *    onc_batch.msgs that onc_encode serialises as it stands, without arenas:
 *    the finished error replies. A handler fills payload_off / payload_len of
 *    its own slice replies[bin_first[h] .. bin_first[h+1]) and encodes that.
 *    `order` carries whatever else the caller keeps per record (rec_seg, slot
 *    offsets) into the same order.
 *  - ntab == 0 is a valid table: every Call is PROG_UNAVAIL. nh == 0 is valid
 *    too, and only an empty table satisfies it.
 *  - The checks come before anything is launched, pointers before alignment.
 *    ONC_RC_EINVAL: a NULL codec, result or bin_first; ntab >
 *    ONC_ROUTE_TABLE_MAX; nh > ONC_ROUTE_HANDLERS_MAX; n >= 2^32 (an order
 *    entry is 32 bits); ntab > 0 with a NULL table; with n > 0 a NULL msgs,
 *    status, route or order; calls_out == msgs or replies == msgs (a
 *    permutation cannot be done in place); calls_out == replies when both are
 *    given. ONC_RC_EALIGN: msgs, calls_out or replies not 16-byte aligned,
 *    bin_first or result not 8-byte aligned, table not 4-byte aligned.
 *    n == 0 still validates the table and writes bin_first (zeros) and result.
 * The call is asynchronous on the codec's stream and every step is a kernel
 * launch (no memset or memcpy node: a captured call replays). Scratch: the
 * per-tile bin counts and a total per bin, (tiles + 1) × (nh + 3) × 4 bytes
 * with ONC_ROUTE_TILE records a tile (about a byte per record at 256 bins), in
 * onc_defragment's buffer: onc_codec_reserve(max_records >= n) covers it;
 * growing it inside a capture is ONC_RC_ECAPTURE. The classify and scan
 * launches report under ONC_K_DEFRAG_PLAN and the scatter under
 * ONC_K_DEFRAG_COPY.
 * Kernels (route.hip), the launch boundary being the only barrier between
 * workgroups: route_classify (a workgroup per tile: the table staged in LDS
 * and validated by every workgroup, the first publishing result[3]; a lane
 * per record loads its status and, for an OK record only, the descriptor's
 * first two 16-byte granules, binary-searches the table, writes route[] and
 * counts the tile's records per bin in LDS; the counts go to the scratch
 * bin-major), route_scan_bins (a workgroup per bin: the bin's tile counts
 * scanned in place, its total kept), route_scan_total (one workgroup: the
 * totals scanned into bin_first, and result), route_scatter (a workgroup per
 * tile: route[] re-read, every record ranked stably — inside a wave among the
 * peers of its bin, found with one ballot per bin bit, across waves by
 * per-wave counts added in wave order — then order[], calls_out and replies
 * as whole 16-byte stores; a rejected Call's stat, low and high are derived
 * again from the table in LDS, nothing is carried in route[] or beside it).
 * All keys are compared unsigned, proc_first + proc_count is formed in 64
 * bits, and every index that addresses memory is 64-bit. */
int onc_route_calls(onc_codec* codec, const onc_msg* msgs, const int32_t* status, uint64_t n,
                    const onc_route* table /*[dev, ntab]*/, uint32_t ntab, uint32_t nh,
                    uint32_t* route     /*[dev, n]*/,
                    uint32_t* order     /*[dev, n]*/,
                    uint64_t* bin_first /*[dev, nh + 4]*/,
                    onc_msg*  calls_out /*[dev, n], optional*/,
                    onc_msg*  replies   /*[dev, n], optional*/,
                    uint64_t* result    /*[dev, 4]*/);

/* ------------------------------------------------------------------------ */
/* XDR of the arguments: a handler's payloads unpacked into columns          */
/* ------------------------------------------------------------------------ */

/* What a handler gets from onc_route_calls is a slice of calls_out whose
 * payloads are still (payload_off, payload_len): an opaque run of XDR bytes
 * (the reference stops there too: CallBody::payload() is a byte slice,
 * src/call_body.rs:150-152). onc_xdr_unpack parses the payload of every
 * payload-carrying record of such a slice against one flat XDR schema
 * (RFC 4506) and writes one column per field — structure of arrays: offset[],
 * count[], where the file handle is — a parse status per record and, when
 * asked, the GARBAGE_ARGS answers (RFC 5531 §9) into onc_route_calls'
 * skeletons. One handler's slice and one schema make one call.
 *
 * A schema is a list of at most ONC_XDR_FIELDS_MAX fields. Nested structs
 * flatten to consecutive fields. XDR optional-data (*T, NFSv3's set_it unions,
 * post_op_attr) is a BOOL | SELECT field followed by the fields of T, each
 * with IF and cond_val 1; a time_how-style three-way union is a U32 | SELECT
 * followed by arms with different cond_val. There is one selector register
 * per record: no nesting stack, no recursion, no linked lists.
 * Opaque and array bodies are never parsed: a column says where they are.
 * Padding follows the reference's Opaque::from_wire (src/opaque.rs:76-95):
 * the maximum is checked first, then the padded end against the slice; the
 * pad bytes must be there and are not checked for zero. */
#define ONC_XDR_FIELDS_MAX 64u
/* type = type_flags & 0xFF */
#define ONC_XDR_U32          0u  /* int, unsigned, enum, float bits: 4 bytes            -> u32 column              */
#define ONC_XDR_U64          1u  /* hyper, unsigned hyper, double bits: 8 bytes, high word first -> u64 column      */
#define ONC_XDR_BOOL         2u  /* 4 bytes, value 0 or 1                               -> u32 column              */
#define ONC_XDR_OPAQUE_FIXED 3u  /* opaque[arg]: arg bytes + pad to 4                   -> u32 column: position    */
#define ONC_XDR_OPAQUE_VAR   4u  /* opaque<arg>, string<arg>: length word, bytes, pad   -> n positions, then n lengths */
#define ONC_XDR_ARRAY32      5u  /* T<arg>, 4-byte elements: count word, 4*count bytes  -> n positions, then n counts  */
#define ONC_XDR_ARRAY64      6u  /* T<arg>, 8-byte elements                              -> likewise                */
/* flags */
#define ONC_XDR_SELECT    0x100u /* U32/BOOL only: the parsed value becomes the selector */
#define ONC_XDR_IF        0x200u /* the field is on the wire only if the selector is set and == cond_val */
#define ONC_XDR_NO_COLUMN 0x400u /* parsed and checked, nothing stored; col_off must be 0 */
/* call flags */
#define ONC_XDR_EXACT     0x1u   /* bytes left after the last field are an error */

typedef struct onc_xdr_field {   /* 24 bytes */
    uint32_t type_flags;
    uint32_t arg;                /* OPAQUE_FIXED: n; OPAQUE_VAR / ARRAY*: the maximum; else 0 */
    uint64_t col_off;            /* byte offset of the column in cols */
    uint32_t cond_val;           /* with ONC_XDR_IF, else 0 */
    uint32_t reserved;           /* 0 */
} onc_xdr_field;

/* xstat[r] = code | failing field << 8 (field nf for ONC_XDR_TRAILING) */
#define ONC_XDR_OK         0u
#define ONC_XDR_SKIPPED    1u   /* the record carries no payload (status != ONC_OK, a reply without one) */
#define ONC_XDR_BAD_EXTENT 2u   /* the payload lies outside the wire, the head slot or the record */
#define ONC_XDR_SHORT      3u   /* a field ends past the payload */
#define ONC_XDR_BAD_BOOL   4u   /* a BOOL word above 1 */
#define ONC_XDR_TOO_LONG   5u   /* a length or count above the field's maximum */
#define ONC_XDR_TRAILING   6u   /* ONC_XDR_EXACT: bytes left after the last field */
#define ONC_XDR_HEAD_SHORT 7u   /* heads form: a word read ends past the head (repeat with longer heads) */
#define ONC_XDR_TILE 256u       /* records per workgroup of the kernel (tests: the sizes around it) */

/* Column widths for n records: U32, BOOL and OPAQUE_FIXED take 4 n bytes; U64
 * takes 8 n bytes, col_off a multiple of 8, the value a native uint64_t;
 * OPAQUE_VAR and the arrays take 8 n bytes: uint32_t pos[n], then uint32_t
 * len_or_count[n] at col_off + 4 n — the form onc_place_payloads takes as
 * pay_pos / pay_len. All other col_off values are multiples of 4.
 *
 * onc_xdr_schema_check validates a schema on the host (no codec): 0, or
 * bad + 1 where `bad` is the first field that breaks a rule; ONC_RC_EINVAL for
 * nf > ONC_XDR_FIELDS_MAX or a NULL fields with nf > 0. The rules: the type is
 * at most 6; no flag bits other than the three above, and reserved == 0;
 * SELECT only on U32 or BOOL; IF only after an earlier SELECT field;
 * cond_val == 0 without IF; arg == 0 where the type does not use it (U32, U64,
 * BOOL); with NO_COLUMN, col_off == 0; otherwise the alignment above,
 * col_off <= cols_cap and width * n <= cols_cap - col_off (no sum wraps), and
 * the column's byte range overlaps no earlier field's. nf == 0 is valid. */
int onc_xdr_schema_check(const onc_xdr_field* fields /*host*/, uint32_t nf, uint64_t n, uint64_t cols_cap);

/* onc_xdr_unpack. The result is exactly this per record r:
 *
 *   pad4(x) = (x + 3) & ~3, in 64 bits. Every comparison below is written so that no sum wraps.
 *   m = msgs[r]
 *   carries = status[r] == ONC_OK and (m.msg_type == CALL or (REPLY and ACCEPTED and stat == SUCCESS))
 *   if not carries: code = SKIPPED          # status != OK: the descriptor is not looked at at all
 *   L = m.payload_len; o = m.payload_off
 *   heads form (rec_start NULL, head_len != 0):
 *       lo = r*head_len; hi = lo + head_len; base = o - lo; bad = o < lo or o > hi
 *   else:
 *       hi = wire_len; bad = o > wire_len or L > wire_len - o
 *       base = rec_start ? o - rec_start[r] : 0; bad |= rec_start and o < rec_start[r]
 *   bad |= base + L > 0xFFFFFFFF
 *   if bad: code = BAD_EXTENT               # nothing read
 *   p = 0; sel_ok = false
 *   reading k bytes at p: if k > L - p: fail SHORT;
 *                         if o + p + k > hi: fail HEAD_SHORT (heads form only)
 *   for f in 0 .. nf-1:
 *       if IF and not (sel_ok and sel == cond_val):      # absent
 *           column(s)[r] = 0; if SELECT: sel_ok = false; continue
 *       U32:   v = be32; p += 4
 *       BOOL:  v = be32; v > 1 -> fail BAD_BOOL; p += 4
 *       U64:   8 bytes; p += 8
 *       OPAQUE_FIXED: pad4(arg) > L - p -> SHORT (bytes not read); pos = base + p; p += pad4(arg)
 *       OPAQUE_VAR:   len = be32; len > arg -> TOO_LONG; pad4(len) > L - (p+4) -> SHORT;
 *                     pos = base + p + 4; p += 4 + pad4(len)
 *       ARRAY32/64:   c = be32; c > arg -> TOO_LONG; c*4|8 (64-bit) > L - (p+4) -> SHORT;
 *                     pos = base + p + 4; p += 4 + bytes
 *       present bit f set; if SELECT: sel = v; sel_ok = true
 *   if EXACT and L - p != 0: fail TRAILING at field nf
 *   xstat[r] = code | f_fail << 8
 *
 *  - The first failure wins. The failing field and every field after it write
 *    0; `present` keeps the bits of the fields that were completed. rest_pos /
 *    rest_len are base + p, L - p for an OK record, else 0. SKIPPED and
 *    BAD_EXTENT records write 0 everywhere. Every element r < n of every
 *    column is written, and nothing else of cols is.
 *  - Positions: with rec_start (onc_decode_extents' input) they count from the
 *    record's first byte, mark included, as onc_place_payloads' pay_pos does;
 *    in the heads form (onc_decode_heads' descriptors) likewise, from the
 *    record's head slot; with neither, from the payload's first byte.
 *  - replies[dev, n] (optional, in/out): a record with msg_type == CALL and a
 *    code of 3..6 gets replies[r].stat = ONC_ACCEPT_GARBAGE_ARGS; no other byte
 *    of replies is written. Pass the slice of onc_route_calls' skeletons that
 *    matches the calls_out slice. HEAD_SHORT is not patched: as after
 *    onc_decode_heads, the caller repeats with longer heads.
 *  - result[dev, 4] = {OK records, records with a code of 3..6, records with
 *    any other code, 0}.
 *  - fields[host, nf] is read before the call returns.
 *  - The checks come before anything is launched, pointers before alignment.
 *    ONC_RC_EINVAL: a NULL codec or result; a schema onc_xdr_schema_check
 *    refuses; unknown call flags; both rec_start and head_len; a head_len that
 *    onc_decode_heads would refuse; wire_len < n * head_len in the heads form;
 *    one of rest_pos / rest_len without the other; with n > 0 a NULL wire,
 *    msgs, status or xstat; a NULL cols when some field has a column.
 *    ONC_RC_EALIGN: msgs or replies not 16-byte aligned; cols, present or
 *    result not 8-byte aligned. n == 0 writes a zero result.
 * The call is asynchronous on the codec's stream and every step is a kernel
 * launch (a captured call replays). No atomics on caller arrays: any of them
 * may be mapped host memory, and the receive slab normally is. Wire reads
 * follow onc_decode's rule: only whole aligned 16-byte granules that hold at
 * least one byte of the record's payload inside the readable window (the
 * wire, or the head slot); nothing is read for SKIPPED and BAD_EXTENT records,
 * and an opaque or array body only where it shares the first 80 bytes' granules
 * with the words around it. Scratch: three counts per workgroup of
 * ONC_XDR_TILE records, in onc_defragment's buffer: onc_codec_reserve
 * (max_records >= n) covers it; growing it inside a capture is
 * ONC_RC_ECAPTURE. Both launches report under ONC_K_DEC_PARSE.
 * Kernels (xdr.hip): xdr_unpack (a lane per record; the schema travels by
 * value in the kernel arguments, so the field loop is wave-uniform: scalar
 * loads of the schema, uniform branches on type and flags; a lane loads the
 * descriptor's first two 16-byte granules for an OK record only, fetches up
 * front the granules as far as the schema's word reads can reach with every
 * length at its maximum, five at most, and the rest on demand; a column store writes consecutive records from consecutive lanes) and
 * xdr_result (one workgroup: the counts summed into result). The arithmetic
 * is xdr_plan.h, shared with the host. */
int onc_xdr_unpack(onc_codec* codec, const uint8_t* wire, uint64_t wire_len,
                   const onc_msg* msgs, const int32_t* status, uint64_t n,
                   const uint64_t* rec_start /*[dev, n], optional*/, uint32_t head_len /*heads form, else 0*/,
                   const onc_xdr_field* fields /*[host, nf]: read before the call returns*/, uint32_t nf, uint32_t flags,
                   uint8_t* cols /*[dev, cols_cap]*/, uint64_t cols_cap,
                   uint32_t* xstat /*[dev, n]*/, uint64_t* present /*[dev, n], optional*/,
                   uint32_t* rest_pos, uint32_t* rest_len /*[dev, n], optional, both or neither*/,
                   onc_msg* replies /*[dev, n], optional, in/out*/, uint64_t* result /*[dev, 4]*/);

/* The other half of every exchange: a client that sent Calls over many
 * connections gets their Replies back in whatever order the servers finished
 * them, and pairs each with the Call it answers by (connection, xid) (the
 * reference leaves that loop to the application too: RpcMessage::xid() and
 * reply_body(), nothing more). onc_match_replies is that loop as one batch
 * call on the device: a hash join of the decoded records against the caller's
 * list of pending Calls. The call keeps nothing between batches: the caller
 * owns the pending list, the codec only scratch. */
typedef struct onc_pending {      /* 16 bytes */
    uint32_t conn;                /* the connection the Call went out on: what onc_frame_streams' rec_seg
                                     says for its Reply. Any value, 0xFFFFFFFF included */
    uint32_t xid;                 /* any value */
    uint64_t tag;                 /* the caller's (a request slot, a send time): copied, never looked at */
} onc_pending;

#define ONC_MATCH_UNKNOWN   0xFFFFFFFFu  /* match[r]: an OK Reply whose (conn, xid) is not pending */
#define ONC_MATCH_DUPLICATE 0xFFFFFFFEu  /* an OK Reply whose entry an earlier record of this batch answers */
#define ONC_MATCH_NOT_REPLY 0xFFFFFFFDu  /* an OK record whose msg_type != ONC_MSG_REPLY */
#define ONC_MATCH_FAILED    0xFFFFFFFCu  /* status != ONC_OK: neither descriptor nor rec_conn is looked at */
#define ONC_MATCH_NONE      0xFFFFFFFFu  /* hit[p]: no record of this batch answers entry p */
#define ONC_MATCH_MAX       0xFFFFFFF0u  /* n and np must be below it */
#define ONC_MATCH_TILE      1024u        /* records / entries per workgroup (tests: the sizes around it) */

/* onc_match_replies. The result is exactly that of
 *
 *   lead(c, x) = the lowest p with pending[p].conn == c and pending[p].xid == x, or none
 *   for r in 0 .. n-1:
 *       if   status[r] != ONC_OK:                 match[r] = FAILED
 *       elif msgs[r].msg_type != ONC_MSG_REPLY:   match[r] = NOT_REPLY
 *       else:
 *           p = lead(rec_conn ? rec_conn[r] : 0, msgs[r].xid)
 *           if   p is none:                                        match[r] = UNKNOWN
 *           elif an r' < r is an OK Reply with the same lead p:    match[r] = DUPLICATE
 *           else:                                                  match[r] = p
 *   for p in 0 .. np-1:  hit[p] = the r with match[r] == p, or ONC_MATCH_NONE
 *   if tag_out: tag_out[r] = pending[match[r]].tag when match[r] < np, else 0
 *   if still:   still[0 .. k) = the entries with hit[p] == NONE, in ascending p, all 16 bytes untouched
 *   result = {matched, unknown, duplicate, not_reply, failed, k}      # the first five sum to n; k is counted with still NULL too
 *
 *  - Repeated pending keys. An entry that repeats an earlier entry's (conn,
 *    xid) is never hit while the earlier one stands: it stays in `still` and
 *    becomes the lead once the earlier one is answered. Repeated xids are
 *    answered first sent, first matched, over successive batches.
 *  - The next pending list. `still` followed by the Calls sent since is the
 *    pending list of the next call.
 *  - No key value is reserved: (0, 0) and (0xFFFFFFFF, 0xFFFFFFFF) are
 *    ordinary keys.
 *  - reply_stat, stat and everything else in the descriptor is not looked at:
 *    a denied Reply answers its Call as well. Of a failed record neither the
 *    descriptor nor rec_conn is looked at.
 *  - The checks come before anything is launched, pointers before alignment.
 *    ONC_RC_EINVAL: a NULL codec or result; n or np >= ONC_MATCH_MAX; with
 *    n > 0 a NULL msgs, status or match; with np > 0 a NULL pending or hit;
 *    still == pending. ONC_RC_EALIGN: msgs, pending or still not 16-byte
 *    aligned; tag_out or result not 8-byte aligned; rec_conn, match, hit or
 *    status not 4-byte aligned. n == 0 still writes hit (all NONE), still (a
 *    copy of the list) and result; np == 0 sends every OK Reply to UNKNOWN.
 * The call is asynchronous on the codec's stream and every step is a kernel
 * launch (no memset or memcpy node: a captured call replays). Every caller
 * array is read and written with plain loads and stores only, so any of them
 * may be mapped host memory; all atomics go to the scratch. Scratch: the slot
 * table (S 32-bit slots, S the least power of two >= 2 np and >= 16),
 * first_rec[np] and the tiles' counts — under 32 bytes per pending entry plus
 * under 1 byte per 32 records — in onc_defragment's buffer:
 * onc_codec_reserve(max_records >= max(n, np)) covers it; growing it inside a
 * capture is ONC_RC_ECAPTURE. The clear, insert, probe, resolve and scan
 * launches report under ONC_K_DEFRAG_PLAN and the compaction under
 * ONC_K_DEFRAG_COPY.
 * Kernels (match.hip), the launch boundary being the only barrier between
 * workgroups — none waits for another, nothing spins on memory, and every
 * probe loop ends after S slots: match_clear (slots and first_rec filled with
 * 0xFFFFFFFF, 16-byte stores), match_insert (a lane per pending entry: hash
 * of (conn, xid), linear probing; atomicCAS(slot, EMPTY, p) claims an empty
 * slot; the index q it returns otherwise names the slot's key, pending[q]:
 * equal keys atomicMin(slot, p), different keys the next slot; the kernel
 * decides only from what the atomics return, so each key ends in exactly one
 * slot holding its lowest index: which slot depends on the race, no output
 * does), match_probe (a lane per record: the status and, for an OK record
 * only, the descriptor's first 16-byte granule and rec_conn[r]; the chain
 * walked with plain loads to an equal key or an empty slot; match[r]
 * provisional; atomicMin(&first_rec[p], r)), match_resolve (a lane per record:
 * a provisional p whose first_rec[p] != r becomes DUPLICATE, tag_out, the
 * tile's five classes counted; a lane per pending entry: hit[p] =
 * first_rec[p], the tile's unanswered entries counted), match_scan (one
 * workgroup: the unanswered counts scanned, the class counts summed, result),
 * match_compact (only with still: a lane per pending entry ranked among its
 * tile's unanswered entries with a ballot and per-wave counts; the whole
 * 16-byte entry moved). Every index that addresses memory is 64-bit.
 * ONC_VARIANT_MATCH_ONE_CHAIN hashes every key to slot S - 2: the whole list
 * is then one chain that wraps round the end of the table (quadratic: tests
 * only); results are bit-identical. */
int onc_match_replies(onc_codec* codec, const onc_msg* msgs, const int32_t* status,
                      const uint32_t* rec_conn /*[dev, n], optional: NULL = every record on connection 0*/,
                      uint64_t n,
                      const onc_pending* pending /*[dev, np]*/, uint64_t np,
                      uint32_t* match       /*[dev, n]*/,
                      uint32_t* hit         /*[dev, np]*/,
                      uint64_t* tag_out     /*[dev, n], optional*/,
                      onc_pending* still    /*[dev, np], optional*/,
                      uint64_t* result      /*[dev, 6]*/);

/* onc_route_calls leaves the reply descriptors in handler order and onc_encode
 * serialises them in that order; a server sends per connection, one socket
 * each, and a client's Calls are built in whatever order the application
 * produced them. onc_group_by_conn is the step between: a stable sort of the
 * item indices by connection id, the start of every connection's run, and
 * optionally the descriptors gathered into that order, so that onc_encode's
 * output is one contiguous stream per connection (onc_conn_extents: where). */
#define ONC_GROUP_CONN_MAX 0x00FFFFFFu   /* nconn at most 2^24 - 1 */
#define ONC_GROUP_TILE     1024u         /* items per workgroup (tests: the sizes around it) */

/* onc_group_by_conn. The result is exactly that of
 *
 *   for k in 0 .. n-1:
 *       s = via ? via[k] : k
 *       c = s < nsrc ? rec_conn[s] : nconn       # an index outside rec_conn is never read
 *       key[k] = min(c, nconn)                   # group nconn: "no connection", nothing to send
 *   order = the item indices 0 .. n-1 sorted by key[], stably (ascending k inside a group)
 *   conn_first[c] = number of items with key < c, for c in 0 .. nconn+1
 *                   # group c is order[conn_first[c] .. conn_first[c+1]); conn_first[nconn+1] == n
 *   if msgs_out: msgs_out[j] = msgs[order[j]]    # all 64 bytes, untouched; msgs is indexed by item, not through via
 *   result = {conn_first[nconn], n - conn_first[nconn], number of c < nconn with a non-empty group}
 *
 *  - Server: rec_conn = onc_frame_streams' rec_seg, via = onc_route_calls'
 *    order, n = bin_first[nh + 1] (the Calls, served and rejected: the last
 *    two bins have zero replies), msgs = replies after the handlers filled
 *    their slices. msgs_out[0 .. result[0]) is then an onc_batch.msgs that
 *    onc_encode serialises as it stands; connection c's stream is the records
 *    [conn_first[c], conn_first[c+1]) of it, in the items' order: handler by
 *    handler and, inside a handler, in the order the connection sent its
 *    Calls (a peer pairs a Reply with its Call by xid, not by position). A
 *    writev sender takes the same slice of onc_encode_iov's entries.
 *  - Client: via NULL, rec_conn = the connection per Call; `order` carries the
 *    caller's onc_pending list into the same order.
 *  - A connection id of nconn or more (0xFFFFFFFF for instance) marks an item
 *    that is not sent: those come last, in group nconn.
 *  - The checks come before anything is launched, pointers before alignment.
 *    ONC_RC_EINVAL: a NULL codec, result or conn_first; nconn >
 *    ONC_GROUP_CONN_MAX; n >= 2^32 (an order entry is 32 bits); with via NULL,
 *    nsrc != n; with n > 0 a NULL order; with n > 0 and nsrc > 0 a NULL
 *    rec_conn; msgs_out without msgs; msgs_out == msgs; order == via (a
 *    permutation cannot be done in place). ONC_RC_EALIGN: msgs or msgs_out not
 *    16-byte aligned, conn_first or result not 8-byte aligned, rec_conn, via
 *    or order not 4-byte aligned. n == 0 still writes conn_first (zeros) and
 *    result. nconn == 0 is valid: everything is group 0 and order is the
 *    identity.
 * The call is asynchronous on the codec's stream and every step is a kernel
 * launch (no memset or memcpy node: a captured call replays); how many depends
 * on n and nconn only. Every caller array is read and written with plain loads
 * and stores only, so any of them may be mapped host memory; all atomics go to
 * LDS. Scratch: the tiles' digit counts and two (key, index) buffers, 17 bytes
 * per item and 7 KiB, in onc_defragment's buffer: onc_codec_reserve(
 * max_records >= n) covers it; growing it inside a capture is
 * ONC_RC_ECAPTURE. The counts, scans, bounds and result launches report under
 * ONC_K_DEFRAG_PLAN, the scatters and the gather under ONC_K_DEFRAG_COPY.
 * Kernels (group.hip), the launch boundary being the only barrier between
 * workgroups: a least-significant-digit radix sort of (key, index) pairs with
 * 8-bit digits, passes = ceil(bits(nconn) / 8) with bits(0) = 0, so 0 to 3.
 * Without a pass group_identity writes order. Per pass: group_count (a
 * workgroup per tile of ONC_GROUP_TILE items; the first pass reads rec_conn
 * through via and clamps, later passes read the pairs in sequence; a digit's
 * peers in a wave found with one ballot per digit bit; the tile's counts go to
 * the scratch digit-major), group_scan_digits (a workgroup per digit: its tile
 * counts scanned in place), group_scan_total (the 256 totals scanned),
 * group_scatter (every item ranked stably — inside a wave by the ballots,
 * across waves by per-wave counts added in wave order — and its pair written
 * there; the last pass writes order). Then group_bounds (a lane per entry of
 * conn_first: a lower-bound binary search of the sorted keys, 32 dependent
 * loads at most, and the non-empty groups counted per workgroup), group_result
 * (one workgroup: those counts summed; result) and, with msgs_out,
 * group_gather (four consecutive lanes on the four 16-byte pieces of a
 * descriptor: a wave's stores are whole lines). Every index that addresses
 * memory is 64-bit. */
int onc_group_by_conn(onc_codec* codec,
                      const uint32_t* rec_conn /*[dev, nsrc]*/, uint64_t nsrc,
                      const uint32_t* via      /*[dev, n], optional*/,
                      uint64_t n, uint32_t nconn,
                      uint32_t* order          /*[dev, n]*/,
                      uint64_t* conn_first     /*[dev, nconn + 2]*/,
                      const onc_msg* msgs      /*[dev, n], optional*/,
                      onc_msg* msgs_out        /*[dev, n], optional; needs msgs*/,
                      uint64_t* result         /*[dev, 3]*/);

/* onc_conn_extents: conn_off[c] = rec_off[min(conn_first[c], nrec)] for c in
 * 0 .. nconn+1: connection c's bytes of the encoded stream are
 * out[conn_off[c], conn_off[c+1]). rec_off is any nrec + 1 offsets:
 * onc_encode's, its offsets after onc_compact, or onc_fragment's out_off. A
 * caller that encoded only the first result[0] descriptors passes that as
 * nrec: the clamp keeps the dropped group's entries inside rec_off, and
 * nothing outside it is ever read. One kernel with a lane per entry
 * (ONC_K_DEFRAG_PLAN), no scratch. ONC_RC_EINVAL: a NULL codec, rec_off,
 * conn_first or conn_off; nconn > ONC_GROUP_CONN_MAX. ONC_RC_EALIGN: a
 * pointer that is not 8-byte aligned. */
int onc_conn_extents(onc_codec* codec, const uint64_t* rec_off /*[dev, nrec + 1]*/, uint64_t nrec,
                     const uint64_t* conn_first /*[dev, nconn + 2]*/, uint32_t nconn,
                     uint64_t* conn_off /*[dev, nconn + 2]*/);

/* Exclusive scan of record lengths into offsets:
 * rec_off[0] = base, rec_off[i+1] = rec_off[i] + rec_len[i]  ([dev]). */
int onc_scan_lengths(onc_codec* codec, const uint32_t* rec_len, uint64_t n,
                     uint64_t base, uint64_t* rec_off);

/* onc_scan_lengths + onc_decode in one pass: record i is
 * wire[off_i, off_i + rec_len[i]) with off_0 = base, off_(i+1) = off_i +
 * rec_len[i] (the caller's length-delimited slices, each decoded as by
 * TryFrom<&[u8]> / TryFrom<Bytes>, rpc_message.rs:235-314). The offsets are
 * computed inside the decode (no offsets pass over the batch); rec_off
 * (optional, n + 1 entries, [dev]) receives them. Same outputs, over-read
 * rule and errors as onc_decode. */
int onc_decode_lengths(onc_codec* codec, const uint8_t* wire, const uint32_t* rec_len, uint64_t n,
                       uint64_t base, int mode, uint64_t* rec_off, const onc_decoded* out);

/* ------------------------------------------------------------------------ */
/* Body-level roots (ONC_ROOT_*)                                             */
/* ------------------------------------------------------------------------ */

/* Decode record i = wire[rec_off[i] .. rec_off[i+1]) as `root`'s TryFrom
 * over exactly that slice (slice mode: a Cursor over it, so every opaque
 * bound is the record; Bytes mode: a Bytes of it). Unlike RpcMessage, a body
 * has no framing header and no trailing-bytes check (the reference's body
 * TryFrom impls return what they parsed and ignore the rest).
 *   param[dev, n]   : AUTH_UNIX_PARAMS slice mode: expected_len; OPAQUE:
 *                     max_len (both modes); required for those, else ignored
 *                     (may be NULL).
 *   out             : as onc_decode (descriptor shape per root above).
 *   consumed[dev, n]: optional: bytes the value occupies (the cursor's final
 *                     position = its serialised_len(); Call / Success
 *                     payloads extend to the record's end); 0 on error.
 * ONC_ROOT_RPC_MESSAGE is onc_decode (consumed = the record length on OK).
 * Same over-read rule as onc_decode. */
int onc_decode_body(onc_codec* codec, int root, const uint8_t* wire, const uint64_t* rec_off, uint64_t n,
                    int mode, const uint32_t* param, const onc_decoded* out, uint32_t* consumed);

/* ------------------------------------------------------------------------ */
/* Bounded decode — the three decodes above with the wire's length           */
/* ------------------------------------------------------------------------ */

/* onc_decode, onc_decode_lengths and onc_decode_body trust the caller's
 * extents; these take wire_len, the number of readable bytes from `wire`,
 * and never read outside [wire, wire + wire_len) beyond the over-read rule
 * of onc_decode (whole 16-byte granules that hold bytes of a record with a
 * good extent). Offsets are relative to `wire`; `base` counts. Use them for
 * offsets or lengths that do not come from onc_frame_stream (the reference
 * takes a slice: RpcMessage::try_from reads only inside it,
 * rpc_message.rs:243-267, and cutting &wire[off..off + len] out of range
 * panics).
 * A record whose extent lies inside the wire — an empty record at
 * off == wire_len included — decodes exactly as by the unbounded call. A
 * record with a bad extent gets ONC_DEC_BAD_EXTENT with aux0 = the first of
 * ONC_EXTENT_NOT_MONOTONIC (offset forms), ONC_EXTENT_START_PAST_WIRE,
 * ONC_EXTENT_END_PAST_WIRE that applies and aux1 = 0, a zeroed descriptor, no
 * AUTH_UNIX slot and consumed = 0; no byte is read for it, and like any
 * other failed record it takes no slot from its group's OK records.
 * onc_decode_lengths_bounded still writes the true prefix sums to rec_off
 * for every record; once they pass wire_len every later record is
 * ONC_EXTENT_START_PAST_WIRE. Arguments, return codes, scratch
 * (onc_codec_reserve) and graph capture are those of the unbounded calls. */
int onc_decode_bounded(onc_codec* codec, const uint8_t* wire, uint64_t wire_len, const uint64_t* rec_off,
                       uint64_t n, int mode, const onc_decoded* out);
int onc_decode_lengths_bounded(onc_codec* codec, const uint8_t* wire, uint64_t wire_len, const uint32_t* rec_len,
                               uint64_t n, uint64_t base, int mode, uint64_t* rec_off, const onc_decoded* out);
int onc_decode_body_bounded(onc_codec* codec, int root, const uint8_t* wire, uint64_t wire_len,
                            const uint64_t* rec_off, uint64_t n, int mode, const uint32_t* param,
                            const onc_decoded* out, uint32_t* consumed);

/* Decode records that are not back to back: record i is
 * wire[rec_start[i], rec_start[i] + rec_len[i]) — in any address order, with
 * gaps or overlaps between records (onc_frame_streams' outputs: records of
 * different connections' buffers, a cut tail or a slot's free space between
 * them). Each is decoded exactly as onc_decode_bounded decodes that slice:
 * status, aux words, the descriptor with wire offsets, and the AUTH_UNIX
 * slots, which stay grouped per 64 *output* records from 128g. Always
 * bounded: a record with rec_start[i] > wire_len, or rec_len[i] > wire_len -
 * rec_start[i], gets ONC_DEC_BAD_EXTENT with aux0 = ONC_EXTENT_START_PAST_WIRE
 * / ONC_EXTENT_END_PAST_WIRE (ONC_EXTENT_NOT_MONOTONIC cannot occur), a zeroed
 * descriptor and no slot; the sum rec_start + rec_len is never formed and no
 * byte is read for it. wire_len = UINT64_MAX is the way to trust the extents.
 * Over-read rule, return codes and graph capture as onc_decode; no scratch.
 * (A wave's loads go through one buffer resource based at its lowest record
 * window — not at its first record's, as in the offset forms — so extents in
 * descending address order keep the cooperative loaders.) */
int onc_decode_extents(onc_codec* codec, const uint8_t* wire, uint64_t wire_len,
                       const uint64_t* rec_start, const uint32_t* rec_len, uint64_t n,
                       int mode, const onc_decoded* out);

/* Decode records of which only the head is present (onc_defragment_heads'
 * output, or the header buffers of a NIC that splits header and data):
 * record i is a record of rec_len[i] bytes whose first P_i = min(rec_len[i],
 * head_len) bytes exist, at heads + i * head_len. It is decoded exactly as
 * onc_decode decodes the whole record: status and aux words, the descriptor,
 * the AUTH_UNIX slots (grouped per 64 output records from 128g). Every wire
 * offset in the outputs is relative to heads — i * head_len + the position
 * in the record: payload_off, the auth refs of the non-UNIX kinds, name_off —
 * so payload_off - i * head_len is the payload's position in the record;
 * payload_len is the true length (rec_len[i] minus that position). A decoded
 * batch re-encodes with auth_arena = heads.
 * The one new outcome is a record whose header does not fit its head:
 * ONC_DEC_BAD_EXTENT with aux0 = ONC_EXTENT_HEAD_SHORT and aux1 = 0, a zeroed
 * descriptor, no slot. (a) The parse proceeds in the reference's order; if it
 * needs a 4-byte word, or the gid block, that ends past P_i while ending
 * inside the record, the record is HEAD_SHORT (a read ending past the record
 * itself is still the reference's short-read error). (b) A parse that ends OK
 * but whose header — up to where the payload starts, or the whole record when
 * it has no payload — reaches past P_i is HEAD_SHORT too (a Call's verifier
 * body is skipped, never read): every auth body and machine name of an OK
 * record lies inside heads. An error met before any such read is reported
 * exactly as onc_decode reports it. With head_len >= 736 (ONC_HEAD_SPAN_MAX
 * rounded up) HEAD_SHORT cannot occur. rec_len[i] == 0 decodes as onc_decode
 * decodes an empty extent.
 * head_len is a multiple of 16 in [64, 4096], else ONC_RC_EINVAL; heads must
 * be 16-byte aligned, else ONC_RC_EALIGN. Reads: only the whole 16-byte
 * granules of slot i that hold bytes below P_i; the bytes of a slot past P_i,
 * and the next slot, never affect a result. No scratch; graph capture and
 * the other return codes as onc_decode_extents; timing under ONC_K_DEC_PARSE;
 * both first-round policies apply, bounded by P_i. */
int onc_decode_heads(onc_codec* codec, const uint8_t* heads, uint32_t head_len,
                     const uint32_t* rec_len, uint64_t n, int mode, const onc_decoded* out);

/* serialised_len() of every descriptor as `root` + the checks of that
 * root's serialise_into: shape (ONC_ENC_BAD_DESCRIPTOR), construction panics
 * (NAME_GT_255, GIDS_GT_16), a body >= 2^31 bytes (ONC_ENC_TOO_LONG: the
 * RpcMessage limit, rpc_message.rs:146-151, applied to every root), and the
 * assoc > 200 assert (flavor.rs:110) for roots that serialise an AuthFlavor
 * (MESSAGE_TYPE, CALL_BODY, REPLY_BODY, ACCEPTED_REPLY, AUTH_FLAVOR).
 * Outputs as onc_encode_lengths. */
int onc_encode_body_lengths(onc_codec* codec, int root, const onc_batch* batch, uint32_t* rec_len,
                            int32_t* status);

/* Every descriptor serialised as `root` back to back into out — the batch
 * form of `root`::serialise_into on one Cursor<Vec<u8>>. Same outputs, writer
 * position and capacity rules as onc_encode. */
int onc_encode_body(onc_codec* codec, int root, const onc_batch* batch, uint8_t* out, uint64_t out_cap,
                    uint64_t* rec_off, int32_t* status, uint32_t* rec_len);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* ONC_RPC_H */
