// onc_rpc.hpp — C++ mirror of the reference crate's types over the C ABI.
//
// The reference (domodwyer/onc-rpc v0.3.3) is a Rust crate; the Rust
// toolchain is not in this image, so its public surface for the hot path is
// restated here in C++17 with the same names, argument meanings and error
// behaviour (see INTEGRATION.md for the Rust extern "C" binding):
//
//   RpcMessage      src/rpc_message.rs:97-233     new, xid, message, call_body,
//                                                 reply_body, serialised_len,
//                                                 serialise_into, serialise,
//                                                 try_from (slice / Bytes mode)
//   MessageType     src/rpc_message.rs:22-93      Call | Reply
//   CallBody        src/call_body.rs:17-166       new, rpc_version, program, ...
//   AuthFlavor      src/auth/flavor.rs:18-174     AuthNone(Option<T>) | AuthUnix |
//                                                 AuthShort | Unknown{id, data}
//   AuthUnixParams  src/auth/unix_params.rs:72-245
//   ReplyBody / AcceptedReply / AcceptedStatus / RejectedReply / AuthError
//                   src/reply/*.rs
//   Error           src/errors.rs:6-97            (thrown as onc_rpc::Error)
//   expected_message_len  src/rpc_message.rs:343-367
//
// Values are generic over byte storage in the reference (`T, P:
// AsRef<[u8]>`); here they hold non-owning `Bytes` views (pointer + length),
// exactly like the reference's `&'a [u8]` instantiation: decoded messages
// borrow the caller's wire buffer, encoded messages borrow the caller's
// payload and auth bodies.
//
// All codec work runs on the GPU through libonc_rpc_amd.so:
//   BatchEncoder  — the caller's serialise_into loop over many messages,
//                   one onc_encode_body call (one pass, no length pass);
//                   serialise_vectored is its zero-copy form: headers only,
//                   the records fragmented as a writev() list of pieces
//                   (onc_encode_iov + onc_fragment_iov), and
//                   serialise_fragmented that list gathered into bytes by
//                   the device (onc_piece_offsets + onc_gather_pieces).
//   BatchDecoder  — the caller's try_from loop over many records, one
//                   onc_decode_lengths_bounded call (a record length that
//                   runs past the wire is Error(ONC_DEC_BAD_EXTENT), unread).
//   Both stage their inputs and outputs in the codec's mapped pinned host
//   memory (Codec::stage): the kernels read and write it in place over PCIe
//   — no device allocation and no copy calls, one synchronisation per call.
//   RpcMessage::serialise_into / serialised_len / try_from — single-message
//                   forms, implemented as batches of one (for API parity;
//                   use the batch classes for throughput).
// There is no CPU codec in this header: the value classes only describe
// messages; lengths, bytes and parse results always come from the kernels.
// The reference's panics (auth data > 200 bytes, machine name > 255 bytes,
// more than 16 gids) are thrown as std::logic_error where the reference
// panics (constructors) and reported as ONC_ENC_* statuses by the batch
// encoder.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <variant>
#include <vector>

#include "onc_rpc.h"

namespace onc_rpc {

// ----------------------------------------------------------------------------
// Bytes: a borrowed byte slice (&[u8])
// ----------------------------------------------------------------------------
struct Bytes {
    const uint8_t* ptr = nullptr;
    size_t len = 0;
    Bytes() = default;
    Bytes(const uint8_t* p, size_t n) : ptr(p), len(n) {}
    Bytes(const std::vector<uint8_t>& v) : ptr(v.data()), len(v.size()) {}  // NOLINT
    const uint8_t* data() const { return ptr; }
    size_t size() const { return len; }
    bool empty() const { return len == 0; }
    std::vector<uint8_t> to_vec() const { return std::vector<uint8_t>(ptr, ptr + len); }
    bool operator==(const Bytes& o) const { return len == o.len && (len == 0 || std::memcmp(ptr, o.ptr, len) == 0); }
    bool operator!=(const Bytes& o) const { return !(*this == o); }
};

// ----------------------------------------------------------------------------
// Error — src/errors.rs:6-97 (Display strings follow the #[error] attributes)
// ----------------------------------------------------------------------------
class Error : public std::exception {
public:
    Error(int32_t code, uint32_t aux0 = 0, uint32_t aux1 = 0) : code_(code), aux0_(aux0), aux1_(aux1) {
        msg_ = describe(code, aux0, aux1);
    }
    int32_t code() const { return code_; }
    // IncompleteMessage{buffer_len, expected}; the offending value for the
    // Invalid*(u32) variants.
    uint32_t buffer_len() const { return aux0_; }
    uint32_t expected() const { return aux1_; }
    uint32_t value() const { return aux0_; }
    const char* what() const noexcept override { return msg_.c_str(); }
    bool operator==(const Error& o) const { return code_ == o.code_ && aux0_ == o.aux0_ && aux1_ == o.aux1_; }

    static std::string describe(int32_t code, uint32_t a0, uint32_t a1) {
        switch (code) {
            case ONC_ERR_INCOMPLETE_MESSAGE:
                return "incomplete rpc message (got " + std::to_string(a0) + " bytes, expected " +
                       std::to_string(a1) + ")";
            case ONC_ERR_INCOMPLETE_HEADER: return "incomplete fragment header";
            case ONC_ERR_FRAGMENTED: return "RPC message is fragmented";
            case ONC_ERR_INVALID_MESSAGE_TYPE: return "invalid rpc message type " + std::to_string(a0);
            case ONC_ERR_INVALID_REPLY_TYPE: return "invalid rpc reply type " + std::to_string(a0);
            case ONC_ERR_INVALID_REPLY_STATUS: return "invalid rpc reply status " + std::to_string(a0);
            case ONC_ERR_INVALID_AUTH_DATA: return "invalid rpc auth data";
            case ONC_ERR_INVALID_AUTH_ERROR: return "invalid rpc auth error status " + std::to_string(a0);
            case ONC_ERR_INVALID_REJECTED_REPLY_TYPE:
                return "invalid rpc rejected reply type " + std::to_string(a0);
            case ONC_ERR_INVALID_LENGTH: return "invalid length in rpc message";
            case ONC_ERR_INVALID_RPC_VERSION: return "invalid rpc version " + std::to_string(a0);
            case ONC_ERR_INVALID_MACHINE_NAME: return "invalid machine name";
            case ONC_ERR_IO_UNEXPECTED_EOF: return "i/o error (UnexpectedEof): failed to fill whole buffer";
            // not a reference error: where the caller's &wire[off..off + len] would panic
            case ONC_DEC_BAD_EXTENT:
                return std::string("slice index out of range: record ") +
                       (a0 == ONC_EXTENT_NOT_MONOTONIC ? "offsets decrease"
                        : a0 == ONC_EXTENT_START_PAST_WIRE ? "starts past the wire" : "ends past the wire");
            default: {
                const char* s = onc_status_str(code);
                return s ? std::string(s) : "error " + std::to_string(code);
            }
        }
    }

private:
    int32_t code_;
    uint32_t aux0_, aux1_;
    std::string msg_;
};

// Device/runtime failure (not a reference error): HIP error or bad argument.
class CodecError : public std::runtime_error {
public:
    using std::runtime_error::runtime_error;
};

enum class DecodeMode { Slice = ONC_DECODE_SLICE, Bytes = ONC_DECODE_BYTES };
class Codec;

// ----------------------------------------------------------------------------
// AuthUnixParams — src/auth/unix_params.rs:72-245
// ----------------------------------------------------------------------------
class AuthUnixParams {
public:
    // AuthUnixParams::from_cursor(r, expected_len) over `buf` (slice rules,
    // unix_params.rs:90-129) and TryFrom<Bytes> (:248-276); serialise_into
    // (:162-176) / serialised_len (:219-230). Body-level decode/encode on the
    // GPU (onc_decode_body / onc_encode_body, ONC_ROOT_AUTH_UNIX_PARAMS).
    static AuthUnixParams from_cursor(Codec& codec, Bytes buf, uint32_t expected_len);
    static AuthUnixParams try_from(Codec& codec, Bytes buf);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;

    // AuthUnixParams::new (unix_params.rs:142-158): panics on a machine name
    // longer than 255 bytes (:149) or more than 16 gids (Gids, :47).
    AuthUnixParams(uint32_t stamp, Bytes machine_name, uint32_t uid, uint32_t gid, std::vector<uint32_t> gids)
        : stamp_(stamp), machine_name_(machine_name), uid_(uid), gid_(gid), gids_(std::move(gids)) {
        if (machine_name.len > ONC_MAX_MACHINE_NAME_LEN) throw std::logic_error("machine name longer than 255 bytes");
        if (gids_.size() > ONC_MAX_GIDS) throw std::logic_error("more than 16 gids");
    }
    uint32_t stamp() const { return stamp_; }
    Bytes machine_name() const { return machine_name_; }
    std::string machine_name_str() const {
        return std::string(reinterpret_cast<const char*>(machine_name_.ptr), machine_name_.len);
    }
    uint32_t uid() const { return uid_; }
    uint32_t gid() const { return gid_; }
    // None (nullopt) when there are no gids (unix_params.rs:210-216).
    std::optional<std::vector<uint32_t>> gids() const {
        if (gids_.empty()) return std::nullopt;
        return gids_;
    }
    const std::vector<uint32_t>& gids_vec() const { return gids_; }
    bool operator==(const AuthUnixParams& o) const {
        return stamp_ == o.stamp_ && machine_name_ == o.machine_name_ && uid_ == o.uid_ && gid_ == o.gid_ &&
               gids_ == o.gids_;
    }

private:
    uint32_t stamp_;
    Bytes machine_name_;
    uint32_t uid_, gid_;
    std::vector<uint32_t> gids_;
};

// ----------------------------------------------------------------------------
// AuthFlavor — src/auth/flavor.rs:18-174
// ----------------------------------------------------------------------------
class AuthFlavor {
public:
    enum class Kind { AuthNone, AuthUnix, AuthShort, Unknown };

    static AuthFlavor none(std::optional<Bytes> data = std::nullopt) {
        AuthFlavor a(Kind::AuthNone);
        a.data_ = data;
        return a;
    }
    static AuthFlavor unix(AuthUnixParams p) {
        AuthFlavor a(Kind::AuthUnix);
        a.unix_ = std::move(p);
        return a;
    }
    static AuthFlavor short_(Bytes data) {
        AuthFlavor a(Kind::AuthShort);
        a.data_ = data;
        return a;
    }
    static AuthFlavor unknown(uint32_t id, Bytes data) {
        AuthFlavor a(Kind::Unknown);
        a.id_ = id;
        a.data_ = data;
        return a;
    }

    Kind kind() const { return kind_; }
    // TryFrom<&[u8]> (flavor.rs:177-184) / TryFrom<Bytes> (:186-222);
    // serialise_into (:106-129) / serialised_len (:154-174) — on the GPU.
    static AuthFlavor try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;
    // associated_data_len (flavor.rs:142-150; unix_params.rs:234-245): the
    // body bytes without prefixes or padding (the value the 200-byte assert
    // of serialise_into checks).
    uint32_t associated_data_len() const {
        if (kind_ == Kind::AuthUnix)
            return uint32_t(12 + unix_->machine_name().len + 4 * unix_->gids_vec().size());
        return data_ ? uint32_t(data_->len) : 0u;
    }
    // Wire discriminant (flavor.rs:132-139).
    uint32_t id() const {
        switch (kind_) {
            case Kind::AuthNone: return ONC_AUTH_NONE;
            case Kind::AuthUnix: return ONC_AUTH_UNIX;
            case Kind::AuthShort: return ONC_AUTH_SHORT;
            default: return id_;
        }
    }
    // AuthNone's optional body / AuthShort / Unknown data.
    std::optional<Bytes> data() const { return data_; }
    const AuthUnixParams& unix_params() const {
        if (!unix_) throw std::logic_error("not AuthUnix");
        return *unix_;
    }
    bool operator==(const AuthFlavor& o) const {
        if (kind_ != o.kind_ || id() != o.id()) return false;
        if (kind_ == Kind::AuthUnix) return *unix_ == *o.unix_;
        if (data_.has_value() != o.data_.has_value()) return false;
        return !data_ || *data_ == *o.data_;
    }

private:
    explicit AuthFlavor(Kind k) : kind_(k) {}
    Kind kind_;
    uint32_t id_ = 0;
    std::optional<Bytes> data_;
    std::optional<AuthUnixParams> unix_;
};

// ----------------------------------------------------------------------------
// CallBody — src/call_body.rs:17-166
// ----------------------------------------------------------------------------
class CallBody {
public:
    CallBody(uint32_t program, uint32_t program_version, uint32_t procedure, AuthFlavor auth_credentials,
             AuthFlavor auth_verifier, Bytes payload)
        : program_(program), program_version_(program_version), procedure_(procedure),
          cred_(std::move(auth_credentials)), verf_(std::move(auth_verifier)), payload_(payload) {}
    uint32_t rpc_version() const { return 2; }   // RPC_VERSION call_body.rs:10
    // TryFrom<&[u8]> (call_body.rs:168-175) / TryFrom<Bytes> (:177-210);
    // serialise_into (:98-108) / serialised_len (:111-119) — on the GPU.
    static CallBody try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;
    uint32_t program() const { return program_; }
    uint32_t program_version() const { return program_version_; }
    uint32_t procedure() const { return procedure_; }
    const AuthFlavor& auth_credentials() const { return cred_; }
    const AuthFlavor& auth_verifier() const { return verf_; }
    Bytes payload() const { return payload_; }
    bool operator==(const CallBody& o) const {
        return program_ == o.program_ && program_version_ == o.program_version_ && procedure_ == o.procedure_ &&
               cred_ == o.cred_ && verf_ == o.verf_ && payload_ == o.payload_;
    }

private:
    uint32_t program_, program_version_, procedure_;
    AuthFlavor cred_, verf_;
    Bytes payload_;
};

// ----------------------------------------------------------------------------
// Replies — src/reply/*.rs
// ----------------------------------------------------------------------------
enum class AuthError : uint32_t {   // rejected_reply.rs:130-173
    Success = 0,
    BadCredentials = 1,
    RejectedCredentials = 2,
    BadVerifier = 3,
    RejectedVerifier = 4,
    TooWeak = 5,
    InvalidResponseVerifier = 6,
    Failed = 7,
};

class RejectedReply {   // rejected_reply.rs:24-95
public:
    enum class Kind { RpcVersionMismatch, AuthError };
    static RejectedReply rpc_version_mismatch(uint32_t low, uint32_t high) {
        RejectedReply r(Kind::RpcVersionMismatch);
        r.low_ = low;
        r.high_ = high;
        return r;
    }
    static RejectedReply auth_error(AuthError e) {
        RejectedReply r(Kind::AuthError);
        r.err_ = e;
        return r;
    }
    Kind kind() const { return kind_; }
    std::pair<uint32_t, uint32_t> mismatch() const { return {low_, high_}; }
    AuthError auth_error() const { return err_; }
    // TryFrom<&[u8]> (rejected_reply.rs:98-105) / TryFrom<Bytes> (:107-125);
    // serialise_into (:61-73) / serialised_len (:76-95) — on the GPU.
    static RejectedReply try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;
    bool operator==(const RejectedReply& o) const {
        return kind_ == o.kind_ && (kind_ == Kind::AuthError ? err_ == o.err_ : (low_ == o.low_ && high_ == o.high_));
    }

private:
    explicit RejectedReply(Kind k) : kind_(k) {}
    Kind kind_;
    uint32_t low_ = 0, high_ = 0;
    AuthError err_ = AuthError::Success;
};

class AcceptedStatus {   // accepted_reply.rs:109-231
public:
    enum class Kind { Success, ProgramUnavailable, ProgramMismatch, ProcedureUnavailable, GarbageArgs, SystemError };
    static AcceptedStatus success(Bytes payload) {
        AcceptedStatus s(Kind::Success);
        s.payload_ = payload;
        return s;
    }
    static AcceptedStatus program_mismatch(uint32_t low, uint32_t high) {
        AcceptedStatus s(Kind::ProgramMismatch);
        s.low_ = low;
        s.high_ = high;
        return s;
    }
    static AcceptedStatus of(Kind k) { return AcceptedStatus(k); }
    Kind kind() const { return kind_; }
    // TryFrom<&[u8]> (accepted_reply.rs:234-241) / TryFrom<Bytes> (:243-265);
    // serialise_into (:195-211) / serialised_len (:214-231) — on the GPU.
    static AcceptedStatus try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;
    Bytes payload() const { return payload_; }
    std::pair<uint32_t, uint32_t> mismatch() const { return {low_, high_}; }
    bool operator==(const AcceptedStatus& o) const {
        if (kind_ != o.kind_) return false;
        if (kind_ == Kind::Success) return payload_ == o.payload_;
        if (kind_ == Kind::ProgramMismatch) return low_ == o.low_ && high_ == o.high_;
        return true;
    }

private:
    explicit AcceptedStatus(Kind k) : kind_(k) {}
    Kind kind_;
    Bytes payload_;
    uint32_t low_ = 0, high_ = 0;
};

class AcceptedReply {   // accepted_reply.rs:20-77
public:
    AcceptedReply(AuthFlavor auth_verifier, AcceptedStatus status)
        : verf_(std::move(auth_verifier)), status_(std::move(status)) {}
    const AuthFlavor& auth_verifier() const { return verf_; }
    const AcceptedStatus& status() const { return status_; }
    // TryFrom<&[u8]> (accepted_reply.rs:79-86) / TryFrom<Bytes> (:88-105);
    // serialise_into (:58-61) / serialised_len (:64-66) — on the GPU.
    static AcceptedReply try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;
    bool operator==(const AcceptedReply& o) const { return verf_ == o.verf_ && status_ == o.status_; }

private:
    AuthFlavor verf_;
    AcceptedStatus status_;
};

class ReplyBody {   // reply_body.rs:16-73
public:
    static ReplyBody accepted(AcceptedReply r) { return ReplyBody(std::move(r)); }
    static ReplyBody denied(RejectedReply r) { return ReplyBody(std::move(r)); }
    bool is_accepted() const { return std::holds_alternative<AcceptedReply>(v_); }
    const AcceptedReply* accepted() const { return std::get_if<AcceptedReply>(&v_); }
    const RejectedReply* denied() const { return std::get_if<RejectedReply>(&v_); }
    bool operator==(const ReplyBody& o) const { return v_ == o.v_; }
    // TryFrom<&[u8]> (reply_body.rs:76-83) / TryFrom<Bytes> (:85-98);
    // serialise_into (:45-56) / serialised_len (:60-73) — on the GPU.
    static ReplyBody try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;

private:
    explicit ReplyBody(AcceptedReply r) : v_(std::move(r)) {}
    explicit ReplyBody(RejectedReply r) : v_(std::move(r)) {}
    std::variant<AcceptedReply, RejectedReply> v_;
};

// MessageType — rpc_message.rs:22-32
class MessageType {
public:
    static MessageType call(CallBody c) { return MessageType(std::move(c)); }
    static MessageType reply(ReplyBody r) { return MessageType(std::move(r)); }
    const CallBody* call_body() const { return std::get_if<CallBody>(&v_); }
    const ReplyBody* reply_body() const { return std::get_if<ReplyBody>(&v_); }
    bool operator==(const MessageType& o) const { return v_ == o.v_; }
    // from_cursor (rpc_message.rs:39-45) / TryFrom<Bytes> (:80-93);
    // serialise_into (:55-68) / serialised_len (:72-77) — on the GPU.
    static MessageType try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    uint32_t serialised_len(Codec& codec) const;

private:
    explicit MessageType(CallBody c) : v_(std::move(c)) {}
    explicit MessageType(ReplyBody r) : v_(std::move(r)) {}
    std::variant<CallBody, ReplyBody> v_;
};

// AuthError::from_cursor (rejected_reply.rs:176-190) / TryFrom<Bytes>
// (:215-236); serialise_into (:194-207) — on the GPU.
AuthError auth_error_try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);
void serialise_into(Codec& codec, AuthError e, std::vector<uint8_t>& buf);

// ----------------------------------------------------------------------------
// Codec: one onc_codec handle (device + stream + scan scratch)
// ----------------------------------------------------------------------------
class Codec {
public:
    explicit Codec(int device = 0, hipStream_t stream = nullptr) {
        if (onc_codec_create(&h_, device, stream) != ONC_RC_OK) throw CodecError("onc_codec_create failed");
    }
    ~Codec() {
        if (h_) {
            (void)onc_codec_sync(h_);
            onc_codec_destroy(h_);
        }
        if (stage_host_) (void)hipHostFree(stage_host_);
    }
    Codec(const Codec&) = delete;
    Codec& operator=(const Codec&) = delete;
    onc_codec* get() const { return h_; }
    void check(int rc, const char* what) const {
        if (rc != ONC_RC_OK) throw CodecError(std::string(what) + ": " + onc_codec_last_error(h_));
    }
    void sync() const { check(onc_codec_sync(h_), "onc_codec_sync"); }

    // The mirror's staging area: mapped pinned host memory (hipHostMalloc,
    // hipHostMallocMapped). Every BatchEncoder / BatchDecoder call (and so
    // every single-message form) puts its inputs there and points the
    // kernels' outputs there, so the kernels read and write it in place over
    // PCIe (include/onc_rpc.h ABI 7: a [dev] pointer may be mapped host
    // memory) — no device allocation, no copy calls, one stream
    // synchronisation per call. `host` and `dev` address the same bytes;
    // valid until the next stage() call on this codec (every mirror call
    // synchronises before it returns). A stage that grows keeps its first
    // `keep` bytes (they move with it: re-derive pointers from offsets).
    struct Stage {
        uint8_t* host;
        uint8_t* dev;
    };
    size_t stage_capacity() const { return stage_cap_; }
    Stage stage(size_t n, size_t keep = 0) {
        if (n > stage_cap_) {
            size_t want = stage_cap_ ? stage_cap_ : (size_t(1) << 20);
            while (want < n) want *= 2;
            void* h = nullptr;
            if (hipHostMalloc(&h, want, hipHostMallocMapped) != hipSuccess) throw CodecError("hipHostMalloc(stage)");
            if (stage_host_) {
                sync();
                if (keep) std::memcpy(h, stage_host_, std::min(keep, stage_cap_));
                (void)hipHostFree(stage_host_);
                stage_host_ = stage_dev_ = nullptr;
                stage_cap_ = 0;
            }
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
                (void)hipHostFree(h);
                throw CodecError("hipHostGetDevicePointer(stage)");
            }
            stage_host_ = static_cast<uint8_t*>(h);
            stage_dev_ = static_cast<uint8_t*>(d);
            stage_cap_ = want;
        }
        return Stage{stage_host_, stage_dev_};
    }

private:
    onc_codec* h_ = nullptr;
    uint8_t* stage_host_ = nullptr;
    uint8_t* stage_dev_ = nullptr;
    size_t stage_cap_ = 0;
};

namespace detail {

inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw CodecError(std::string(what) + ": " + hipGetErrorString(e));
}

// Typed regions of a staging area (256-byte aligned): sized first with
// need(), then taken in the same order from the codec's stage.
inline size_t rounded(size_t b) { return (b + 255) & ~size_t(255); }
template <class T>
struct Region {
    T* host;
    T* dev;
};
struct Carve {
    Codec::Stage s;
    size_t off = 0;
    template <class T>
    Region<T> take(size_t count) {
        const size_t a = off;
        off += rounded(count * sizeof(T) + 16);
        return Region<T>{reinterpret_cast<T*>(s.host + a), reinterpret_cast<T*>(s.dev + a)};
    }
};
template <class T>
inline size_t need(size_t count) { return rounded(count * sizeof(T) + 16); }

}  // namespace detail

// ----------------------------------------------------------------------------
// RpcMessage — src/rpc_message.rs:97-233
// ----------------------------------------------------------------------------
class RpcMessage {
public:
    RpcMessage(uint32_t xid, MessageType message) : xid_(xid), message_(std::move(message)) {}
    uint32_t xid() const { return xid_; }
    const MessageType& message() const { return message_; }
    const CallBody* call_body() const { return message_.call_body(); }
    const ReplyBody* reply_body() const { return message_.reply_body(); }
    bool operator==(const RpcMessage& o) const { return xid_ == o.xid_ && message_ == o.message_; }

    // Single-message calls: each is a whole GPU round trip (the message
    // staged in mapped host memory, the kernels reading and writing it in
    // place, a stream synchronisation) — tens of microseconds where the
    // reference's CPU call takes ~100 ns (tests/cpp/test_mirror.cpp
    // test_single_message_cost prints both). They exist for tests and tiny
    // batches; a caller with many messages uses BatchEncoder / BatchDecoder
    // (one launch per batch). The same holds for every body type's
    // serialised_len / serialise_into / try_from taking a Codec.
    //
    // serialised_len (rpc_message.rs:201-204), computed by the encoder's
    // length kernel. Throws std::logic_error where the reference panics.
    uint32_t serialised_len(Codec& codec) const;
    // serialise_into (rpc_message.rs:136-164): appends the record to `buf`.
    void serialise_into(Codec& codec, std::vector<uint8_t>& buf) const;
    // serialise (rpc_message.rs:193-197)
    std::vector<uint8_t> serialise(Codec& codec) const;
    // TryFrom<&[u8]> (rpc_message.rs:235-271) / TryFrom<Bytes> (:273-314):
    // `buf` must hold exactly one message; the result borrows `buf`.
    static RpcMessage try_from(Codec& codec, Bytes buf, DecodeMode mode = DecodeMode::Slice);

    // Encode statuses -> the reference's behaviour: panics for the
    // construction/assert failures, io::Error for TooLong/WriteZero.
    static void raise_encode_status(int32_t st) {
        switch (st) {
            case ONC_OK: return;
            case ONC_ENC_AUTH_GT_200: throw std::logic_error("auth associated data longer than 200 bytes");
            case ONC_ENC_NAME_GT_255: throw std::logic_error("machine name longer than 255 bytes");
            case ONC_ENC_GIDS_GT_16: throw std::logic_error("more than 16 gids");
            case ONC_ENC_BAD_DESCRIPTOR: throw std::logic_error("invalid message descriptor");
            case ONC_ENC_TOO_LONG: throw std::runtime_error("message length exceeds maximum");
            case ONC_ENC_WRITE_ZERO: throw std::runtime_error("failed to write whole buffer");
            default: throw std::runtime_error(onc_status_str(st));
        }
    }

private:
    uint32_t xid_;
    MessageType message_;
};

// What BatchEncoder::serialise_vectored returns: the stream as a writev()
// list. Piece i is pieces[i].len bytes at pieces[i].off of `marks`
// (ONC_PIECE_MARK), of `headers` (ONC_PIECE_HDR) or of the encoder's payload
// arena (ONC_PIECE_PAYLOAD); message m's pieces are
// pieces[piece_off[m], piece_off[m + 1]) and stand for stream bytes
// [out_off[m], out_off[m + 1]). A failing message has none.
struct VectoredStream {
    std::vector<uint8_t> headers;          // onc_encode_iov's hdr_out
    std::vector<uint8_t> marks;            // 4 bytes per fragment
    std::vector<onc_frag_piece> pieces;
    std::vector<uint64_t> piece_off;       // n + 1
    std::vector<uint64_t> out_off;         // n + 1
    std::vector<int32_t> status;           // per message: ONC_OK or ONC_ENC_*
    size_t n_frags = 0;                    // fragments (= marks.size() / 4)
    size_t n_multi = 0;                    // messages cut into more than one fragment
    uint64_t bytes = 0;                    // the stream's length (= out_off.back())

    // (pointer, length) of piece i, as an iovec entry.
    std::pair<const uint8_t*, size_t> piece_ptr(size_t i, const uint8_t* payload_arena) const {
        const onc_frag_piece& p = pieces.at(i);
        const uint8_t* base = p.src == ONC_PIECE_MARK ? marks.data() : p.src == ONC_PIECE_HDR ? headers.data() : payload_arena;
        return {base + p.off, size_t(p.len)};
    }
    // The byte stream the pieces stand for.
    std::vector<uint8_t> gather(const uint8_t* payload_arena) const {
        std::vector<uint8_t> out;
        out.reserve(size_t(bytes));
        for (size_t i = 0; i < pieces.size(); ++i) {
            const auto p = piece_ptr(i, payload_arena);
            out.insert(out.end(), p.first, p.first + p.second);
        }
        return out;
    }
    // Stream bytes [from, from + count), as far as the stream goes: what
    // onc_gather_pieces writes for that window (from + count saturates).
    std::vector<uint8_t> gather_window(uint64_t from, uint64_t count, const uint8_t* payload_arena) const {
        std::vector<uint8_t> out;
        const uint64_t end = count > ~uint64_t(0) - from ? ~uint64_t(0) : from + count;
        uint64_t pos = 0;
        for (size_t i = 0; i < pieces.size(); ++i) {
            const auto p = piece_ptr(i, payload_arena);
            const uint64_t a = std::max(pos, from), b = std::min(pos + p.second, end);
            if (a < b) out.insert(out.end(), p.first + (a - pos), p.first + (b - pos));
            pos += p.second;
        }
        return out;
    }
};

// What BatchEncoder::serialise_fragmented returns: the fragmented stream as
// bytes. Message m's fragments are bytes[out_off[m], out_off[m + 1]); a
// message that fails (status[m] != ONC_OK) has none.
struct FragmentedStream {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> out_off;         // n + 1
    std::vector<int32_t> status;           // per message: ONC_OK or ONC_ENC_*
    size_t n_frags = 0;                    // fragments
    size_t n_multi = 0;                    // messages cut into more than one fragment
};

// ----------------------------------------------------------------------------
// BatchEncoder: serialise_into of many messages into one send buffer
// ----------------------------------------------------------------------------
class BatchEncoder {
public:
    // Describe one message (copies its borrowed bytes into the host arenas).
    void push(const RpcMessage& m);
    // Body-level values (ONC_ROOT_*): a batch holds values of one type and
    // is serialised as that type (onc_encode_body); mixing throws.
    void push(const MessageType& m);
    void push(const CallBody& c);
    void push(const ReplyBody& r);
    void push(const AcceptedReply& r);
    void push(const AcceptedStatus& s);
    void push(const RejectedReply& r);
    void push(AuthError e);
    void push(const AuthFlavor& a);
    void push(const AuthUnixParams& p);
    int root() const { return root_ < 0 ? ONC_ROOT_RPC_MESSAGE : root_; }
    size_t size() const { return msgs_.size(); }
    void clear() {
        msgs_.clear();
        unix_.clear();
        auth_.clear();
        payload_.clear();
        root_ = -1;
    }

    // Encode every pushed message back to back and APPEND the bytes to `out`
    // (the reference's serialise_into on a Cursor<Vec<u8>> positioned at the
    // end). Returns one status per message (ONC_OK or ONC_ENC_*; failing
    // messages occupy 0 bytes). rec_off, if given, receives n+1 offsets
    // relative to the start of the appended region.
    std::vector<int32_t> serialise_into(Codec& codec, std::vector<uint8_t>& out,
                                        std::vector<uint64_t>* rec_off = nullptr);
    // serialised_len() of every pushed message (0 for failing ones).
    std::vector<uint32_t> serialised_lens(Codec& codec, std::vector<int32_t>* status = nullptr);
    // The zero-copy form of serialise_into (RpcMessage batches only): only
    // the headers are serialised (onc_encode_iov, then onc_compact_iov when a
    // message fails), the payloads stay in this encoder's arena, and the
    // records are cut into fragments of at most max_frag body bytes as a list
    // of pieces (onc_fragment_iov) — nothing is copied. Throws CodecError for
    // a body-level batch or a max_frag outside 1 .. 0x7FFFFFFF.
    VectoredStream serialise_vectored(Codec& codec, uint32_t max_frag = 0x7FFFFFFFu);
    // serialise_vectored's stream as bytes, written once by the device:
    // onc_encode_iov -> onc_fragment_iov -> onc_piece_offsets ->
    // onc_gather_pieces, straight from the marks, the headers and the payload
    // arena into the codec's mapped staging (no packed intermediate, as
    // serialise_into + fragment_stream make). rec_limits, if given, holds a
    // fragment limit per message (size() values; max_frag is then ignored but
    // must still be valid): a message whose own limit is outside
    // 1 .. 0x7FFFFFFF gets ONC_ENC_BAD_DESCRIPTOR and contributes nothing.
    // Throws CodecError for a body-level batch, a max_frag outside
    // 1 .. 0x7FFFFFFF or a rec_limits of another size.
    FragmentedStream serialise_fragmented(Codec& codec, uint32_t max_frag = 0x7FFFFFFFu,
                                          const std::vector<uint32_t>* rec_limits = nullptr);
    // The payload bytes ONC_PIECE_PAYLOAD pieces point into: valid until the
    // next push() or clear().
    const std::vector<uint8_t>& payload_arena() const { return payload_; }

private:
    // the batch's descriptors, AUTH_UNIX table and arenas copied into the
    // codec's mapped staging (the kernels read them there in place)
    size_t staged_bytes() const;
    onc_batch stage_batch(detail::Carve& c) const;
    void put_auth(const AuthFlavor& a, onc_auth& d);
    void put_payload(Bytes p, onc_msg& d);
    void put_call(const CallBody& c, onc_msg& d);
    void put_accepted(const AcceptedReply& a, onc_msg& d);
    void put_status(const AcceptedStatus& s, onc_msg& d);
    void put_rejected(const RejectedReply& r, onc_msg& d);
    void put_reply(const ReplyBody& r, onc_msg& d);
    void set_root(int root);

    int root_ = -1;

    std::vector<onc_msg> msgs_;
    std::vector<onc_unix_params> unix_;
    std::vector<uint8_t> auth_, payload_;
};

// Result of decoding one record (Result<RpcMessage<&[u8], &[u8]>, Error>).
struct Decoded {
    int32_t status = ONC_OK;
    uint32_t aux0 = 0, aux1 = 0;
    std::optional<RpcMessage> message;   // set iff status == ONC_OK
    bool ok() const { return status == ONC_OK; }
    Error error() const { return Error(status, aux0, aux1); }
};

// ----------------------------------------------------------------------------
// HostRegistration: a caller's receive buffer mapped for the kernels
// (onc_host_register, ABI 7). BatchDecoder given one decodes the bytes where
// they lie — no copy into the stage; only the 16-byte granules of the headers
// it parses cross PCIe (call_body.rs:53-59: payloads are slices, never read).
// Registration pins the pages (a server maps its socket buffers once);
// unpinned on destruction, so it must outlive the decodes using it.
// ----------------------------------------------------------------------------
class HostRegistration {
public:
    HostRegistration(Codec& codec, const uint8_t* buf, size_t len) : codec_(codec), host_(buf), len_(len) {
        void* d = nullptr;
        codec.check(onc_host_register(codec.get(), const_cast<uint8_t*>(buf), len ? len : 1, &d),
                    "onc_host_register");
        dev_ = static_cast<const uint8_t*>(d);
    }
    ~HostRegistration() { (void)onc_host_unregister(codec_.get(), const_cast<uint8_t*>(host_)); }
    HostRegistration(const HostRegistration&) = delete;
    HostRegistration& operator=(const HostRegistration&) = delete;
    const uint8_t* host() const { return host_; }
    const uint8_t* dev() const { return dev_; }
    size_t size() const { return len_; }

private:
    Codec& codec_;
    const uint8_t* host_;
    const uint8_t* dev_ = nullptr;
    size_t len_;
};

// One connection's receive buffer inside a slab (try_from_streams):
// wire[off, off + len).
struct Segment {
    uint64_t off = 0, len = 0;
};
// What try_from_streams reports per segment: its records are results
// [first, first + n), `consumed` bytes of it were framed (memmove the rest to
// the buffer's start and read on), and why framing stopped there, as
// try_from_stream's `stop` (ONC_OK: at the segment's end).
struct SegmentResult {
    uint64_t first = 0, n = 0, consumed = 0;
    int32_t status = ONC_OK;
    uint32_t aux0 = 0, aux1 = 0;
    bool ok() const { return status == ONC_OK; }
    Error error() const { return Error(status, aux0, aux1); }
};

// What try_from_mixed_streams returns: one result list per connection, in
// stream order, whether its peer fragments its records or not.
struct MixedStreams {
    std::vector<std::vector<Decoded>> per_connection;
    // per connection: n = its results, `consumed` bytes of its buffer are done
    // with (memmove the rest down and read on), status why it stopped there
    // (ONC_OK: at the buffer's end, or on a fragment boundary inside a record
    // whose last fragment has not arrived); `first` is not used
    std::vector<SegmentResult> segments;
    // the records of the fragmenting peers, reassembled: their results' payload
    // views point here (the others' into the caller's wire)
    std::vector<uint8_t> reassembled;
};

struct FragmentedHeads;   // try_from_fragmented_heads' result (defined with reassemble_heads below)

// ----------------------------------------------------------------------------
// BatchDecoder: try_from of many records (one buffer per record)
// ----------------------------------------------------------------------------
class BatchDecoder {
public:
    // Decode records wire[off_i, off_i + rec_len[i]) back to back (host
    // buffer). Decoded messages borrow `wire` (zero-copy, like the
    // reference's &[u8] instantiation), so it must outlive the results.
    std::vector<Decoded> try_from(Codec& codec, const uint8_t* wire, size_t wire_len,
                                  const std::vector<uint32_t>& rec_len, DecodeMode mode = DecodeMode::Slice);

    // A socket read buffer of back-to-back records: frame it on the device
    // (the caller's expected_message_len loop, rpc_message.rs:343-367), then
    // decode every complete record. `consumed` receives the bytes used;
    // `stop` why framing stopped before the end (nullopt when the buffer
    // ended on a record boundary): an incomplete trailing record means
    // "read more", as with the reference.
    std::vector<Decoded> try_from_stream(Codec& codec, const uint8_t* wire, size_t wire_len,
                                         DecodeMode mode = DecodeMode::Slice, size_t* consumed = nullptr,
                                         std::optional<Error>* stop = nullptr);

    // The same over a registered (mapped) buffer, decoded in place.
    std::vector<Decoded> try_from(Codec& codec, const HostRegistration& wire, const std::vector<uint32_t>& rec_len,
                                  DecodeMode mode = DecodeMode::Slice) {
        return lengths_at(codec, wire.host(), wire.dev(), wire.size(), rec_len, mode);
    }
    std::vector<Decoded> try_from_stream(Codec& codec, const HostRegistration& wire,
                                         DecodeMode mode = DecodeMode::Slice, size_t* consumed = nullptr,
                                         std::optional<Error>* stop = nullptr) {
        return stream_at(codec, wire.host(), wire.dev(), wire.size(), mode, consumed, stop);
    }

    // Many connections' receive buffers at once (slots of one slab, each
    // filled to its own level): every segment framed on its own — the
    // caller's expected_message_len loop per connection — and every whole
    // record of every segment decoded, in two calls (onc_frame_streams,
    // onc_decode_extents). Results are ordered by segment, then by position;
    // per_segment (optional) receives one SegmentResult per segment. A cut
    // tail or a fragmented mark stops only its own segment.
    std::vector<Decoded> try_from_streams(Codec& codec, const uint8_t* wire, size_t wire_len,
                                          const std::vector<Segment>& segments,
                                          std::vector<SegmentResult>* per_segment = nullptr,
                                          DecodeMode mode = DecodeMode::Slice) {
        return streams_at(codec, wire, nullptr, wire_len, segments, per_segment, mode);
    }
    std::vector<Decoded> try_from_streams(Codec& codec, const HostRegistration& wire,
                                          const std::vector<Segment>& segments,
                                          std::vector<SegmentResult>* per_segment = nullptr,
                                          DecodeMode mode = DecodeMode::Slice) {
        return streams_at(codec, wire.host(), wire.dev(), wire.size(), segments, per_segment, mode);
    }

    // The same for a server some of whose peers fragment their records (RFC
    // 5531 §11): try_from_streams first — single-fragment peers are decoded in
    // place — then the rests of the segments that stopped with
    // ONC_ERR_FRAGMENTED reassembled in one pass (reassemble_streams:
    // onc_frame_fragment_streams + onc_defragment_extents) and decoded.
    MixedStreams try_from_mixed_streams(Codec& codec, const uint8_t* wire, size_t wire_len,
                                        const std::vector<Segment>& segments, DecodeMode mode = DecodeMode::Slice);

    // Fragmenting peers without the copy: every segment's fragment chain
    // followed (onc_frame_fragment_streams), only each record's head gathered
    // (onc_defragment_heads) and decoded (onc_decode_heads); the payloads stay
    // in the caller's wire and come back as slices of it
    // (FragmentedHeads::payload_pieces). If a record's header does not fit a
    // head of head_len bytes (ONC_EXTENT_HEAD_SHORT) the batch is done once
    // more with 736-byte heads, which hold every header: the result is always
    // the exact one. head_len 160 is the decode window's size.
    FragmentedHeads try_from_fragmented_heads(Codec& codec, const uint8_t* wire, size_t wire_len,
                                              const std::vector<Segment>& segments,
                                              DecodeMode mode = DecodeMode::Slice, uint32_t head_len = 160);

private:
    std::vector<Decoded> streams_at(Codec& codec, const uint8_t* wire, const uint8_t* dev_wire, size_t wire_len,
                                    const std::vector<Segment>& segments, std::vector<SegmentResult>* per_segment,
                                    DecodeMode mode);
    // dev_wire: the kernels' address of `wire` (a registration), or null:
    // the wire is copied into the stage first
    std::vector<Decoded> lengths_at(Codec& codec, const uint8_t* wire, const uint8_t* dev_wire, size_t wire_len,
                                    const std::vector<uint32_t>& rec_len, DecodeMode mode);
    std::vector<Decoded> stream_at(Codec& codec, const uint8_t* wire, const uint8_t* dev_wire, size_t wire_len,
                                   DecodeMode mode, size_t* consumed, std::optional<Error>* stop);
    // the decode outputs in staging regions, read after the synchronisation
    struct Out {
        detail::Region<onc_msg> msgs;
        detail::Region<onc_unix_params> unix;
        detail::Region<int32_t> status;
        detail::Region<uint32_t> aux0, aux1;
        onc_decoded dev() const { return onc_decoded{msgs.dev, unix.dev, status.dev, aux0.dev, aux1.dev}; }
    };
    static size_t out_bytes(size_t n);
    static Out take_out(detail::Carve& c, size_t n);
    static std::vector<Decoded> results(const Out& o, size_t n, const uint8_t* wire);
};

// expected_message_len (rpc_message.rs:343-367); throws Error.
inline uint32_t expected_message_len(Bytes data) {
    uint32_t n = 0;
    const int32_t st = onc_expected_message_len(data.ptr, data.len, &n);
    if (st != ONC_OK) throw Error(st);
    return n;
}

// ----------------------------------------------------------------------------
// BatchEncoder implementation
// ----------------------------------------------------------------------------
inline void BatchEncoder::put_auth(const AuthFlavor& a, onc_auth& d) {
    d.id = a.id();
    switch (a.kind()) {
        case AuthFlavor::Kind::AuthUnix: {
            const AuthUnixParams& p = a.unix_params();
            onc_unix_params u{};
            u.stamp = p.stamp();
            u.uid = p.uid();
            u.gid = p.gid();
            u.ngids = uint32_t(p.gids_vec().size());
            for (size_t i = 0; i < p.gids_vec().size(); ++i) u.gids[i] = p.gids_vec()[i];
            u.name_off = auth_.size();
            u.name_len = uint32_t(p.machine_name().len);
            auth_.insert(auth_.end(), p.machine_name().ptr, p.machine_name().ptr + p.machine_name().len);
            // ABI 6: declare serialised_len (unix_params.rs:219-230) so that the
            // encoder's length pass reads no parameter block; a block that
            // would panic is left undeclared (0: every check up front)
            const uint32_t ng = u.ngids, nl = u.name_len;
            d.kind_len = ONC_AUTH_PACK(ONC_KIND_UNIX, nl <= ONC_MAX_MACHINE_NAME_LEN && ng <= ONC_MAX_GIDS
                                                          ? 20u + 4u * ((nl + 3u) / 4u) + 4u * ng
                                                          : 0u);
            d.ref = unix_.size();
            unix_.push_back(u);
            return;
        }
        case AuthFlavor::Kind::AuthNone:
        case AuthFlavor::Kind::AuthShort:
        case AuthFlavor::Kind::Unknown: {
            const uint32_t kind = a.kind() == AuthFlavor::Kind::AuthNone    ? ONC_KIND_NONE
                                  : a.kind() == AuthFlavor::Kind::AuthShort ? ONC_KIND_SHORT
                                                                            : ONC_KIND_UNKNOWN;
            const Bytes b = a.data().value_or(Bytes());
            // Bodies longer than the 24-bit descriptor field cannot be
            // described; the reference would panic on them (> 200 bytes).
            if (b.len > 0xFFFFFFu) throw std::logic_error("auth associated data longer than 200 bytes");
            d.kind_len = ONC_AUTH_PACK(kind, b.len);
            d.ref = auth_.size();
            auth_.insert(auth_.end(), b.ptr, b.ptr + b.len);
            return;
        }
    }
}

inline void BatchEncoder::set_root(int root) {
    if (root_ >= 0 && root_ != root) throw std::logic_error("BatchEncoder: values of different types in one batch");
    root_ = root;
}

inline void BatchEncoder::put_payload(Bytes p, onc_msg& d) {
    if (p.len > 0xFFFFFFFFull) throw std::runtime_error("message length exceeds maximum");
    d.payload_len = uint32_t(p.len);
    d.payload_off = payload_.size();
    payload_.insert(payload_.end(), p.ptr, p.ptr + p.len);
}

inline void BatchEncoder::put_call(const CallBody& c, onc_msg& d) {
    d.msg_type = ONC_MSG_CALL;
    d.u.call.program = c.program();
    d.u.call.program_version = c.program_version();
    d.u.call.procedure = c.procedure();
    put_auth(c.auth_credentials(), d.cred);
    put_auth(c.auth_verifier(), d.verf);
    put_payload(c.payload(), d);
}

inline void BatchEncoder::put_status(const AcceptedStatus& s, onc_msg& d) {
    d.msg_type = ONC_MSG_REPLY;
    d.reply_stat = ONC_REPLY_ACCEPTED;
    d.stat = uint8_t(s.kind());
    if (s.kind() == AcceptedStatus::Kind::Success) {
        put_payload(s.payload(), d);
    } else if (s.kind() == AcceptedStatus::Kind::ProgramMismatch) {
        d.u.mismatch.low = s.mismatch().first;
        d.u.mismatch.high = s.mismatch().second;
    }
}

inline void BatchEncoder::put_accepted(const AcceptedReply& a, onc_msg& d) {
    put_auth(a.auth_verifier(), d.verf);
    put_status(a.status(), d);
}

inline void BatchEncoder::put_rejected(const RejectedReply& j, onc_msg& d) {
    d.msg_type = ONC_MSG_REPLY;
    d.reply_stat = ONC_REPLY_DENIED;
    if (j.kind() == RejectedReply::Kind::RpcVersionMismatch) {
        d.stat = ONC_REJECT_RPC_MISMATCH;
        d.u.mismatch.low = j.mismatch().first;
        d.u.mismatch.high = j.mismatch().second;
    } else {
        d.stat = ONC_REJECT_AUTH_ERROR;
        d.auth_stat = uint8_t(j.auth_error());
    }
}

inline void BatchEncoder::put_reply(const ReplyBody& r, onc_msg& d) {
    if (const AcceptedReply* a = r.accepted()) put_accepted(*a, d);
    else put_rejected(*r.denied(), d);
}

inline void BatchEncoder::push(const RpcMessage& m) {
    set_root(ONC_ROOT_RPC_MESSAGE);
    onc_msg d{};
    d.xid = m.xid();
    if (const CallBody* c = m.call_body()) put_call(*c, d);
    else put_reply(*m.reply_body(), d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const MessageType& m) {
    set_root(ONC_ROOT_MESSAGE_TYPE);
    onc_msg d{};
    if (const CallBody* c = m.call_body()) put_call(*c, d);
    else put_reply(*m.reply_body(), d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const CallBody& c) {
    set_root(ONC_ROOT_CALL_BODY);
    onc_msg d{};
    put_call(c, d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const ReplyBody& r) {
    set_root(ONC_ROOT_REPLY_BODY);
    onc_msg d{};
    put_reply(r, d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const AcceptedReply& r) {
    set_root(ONC_ROOT_ACCEPTED_REPLY);
    onc_msg d{};
    put_accepted(r, d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const AcceptedStatus& s) {
    set_root(ONC_ROOT_ACCEPTED_STATUS);
    onc_msg d{};
    put_status(s, d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const RejectedReply& r) {
    set_root(ONC_ROOT_REJECTED_REPLY);
    onc_msg d{};
    put_rejected(r, d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(AuthError e) {
    set_root(ONC_ROOT_AUTH_ERROR);
    onc_msg d{};
    put_rejected(RejectedReply::auth_error(e), d);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const AuthFlavor& a) {
    set_root(ONC_ROOT_AUTH_FLAVOR);
    onc_msg d{};
    d.msg_type = ONC_MSG_CALL;
    put_auth(a, d.cred);
    msgs_.push_back(d);
}

inline void BatchEncoder::push(const AuthUnixParams& p) {
    set_root(ONC_ROOT_AUTH_UNIX_PARAMS);
    onc_msg d{};
    d.msg_type = ONC_MSG_CALL;
    put_auth(AuthFlavor::unix(p), d.cred);
    msgs_.push_back(d);
}

inline size_t BatchEncoder::staged_bytes() const {
    using detail::need;
    return need<onc_msg>(msgs_.size()) + need<onc_unix_params>(unix_.size()) + need<uint8_t>(auth_.size()) +
           need<uint8_t>(payload_.size());
}

inline onc_batch BatchEncoder::stage_batch(detail::Carve& c) const {
    const size_t n = msgs_.size();
    const auto m = c.take<onc_msg>(n);
    const auto u = c.take<onc_unix_params>(unix_.size());
    const auto a = c.take<uint8_t>(auth_.size());
    const auto p = c.take<uint8_t>(payload_.size());
    if (n) std::memcpy(m.host, msgs_.data(), n * sizeof(onc_msg));
    if (!unix_.empty()) std::memcpy(u.host, unix_.data(), unix_.size() * sizeof(onc_unix_params));
    if (!auth_.empty()) std::memcpy(a.host, auth_.data(), auth_.size());
    if (!payload_.empty()) std::memcpy(p.host, payload_.data(), payload_.size());
    onc_batch b{};
    b.n = n;
    b.msgs = m.dev;
    b.unix_params = u.dev;
    b.auth_arena = a.dev;
    b.payload_arena = p.dev;
    b.unix_count = unix_.size();
    b.auth_len = auth_.size();
    b.payload_len = payload_.size();
    return b;
}

inline std::vector<uint32_t> BatchEncoder::serialised_lens(Codec& codec, std::vector<int32_t>* status) {
    using detail::need;
    const size_t n = msgs_.size();
    std::vector<uint32_t> lens(n);
    std::vector<int32_t> st(n);
    if (n) {
        detail::Carve c{codec.stage(staged_bytes() + need<uint32_t>(n) + need<int32_t>(n))};
        const onc_batch b = stage_batch(c);
        const auto dl = c.take<uint32_t>(n);
        const auto ds = c.take<int32_t>(n);
        codec.check(onc_encode_body_lengths(codec.get(), root(), &b, dl.dev, ds.dev), "onc_encode_body_lengths");
        codec.sync();
        std::memcpy(lens.data(), dl.host, n * 4);
        std::memcpy(st.data(), ds.host, n * 4);
    }
    if (status) *status = std::move(st);
    return lens;
}

// One encode pass: the output goes into the stage with a capacity no record
// can reach (a header is at most 460 bytes — 7 words and two auths of 54 —
// and a record keeping a declared extent at most 28 + 2 x 348 bytes before
// its payload), so no separate length pass is needed to size it; the bytes
// are then appended to `out`.
inline std::vector<int32_t> BatchEncoder::serialise_into(Codec& codec, std::vector<uint8_t>& out,
                                                         std::vector<uint64_t>* rec_off) {
    using detail::need;
    const size_t n = msgs_.size();
    std::vector<int32_t> st(n);
    std::vector<uint64_t> off(n + 1, 0);
    if (n) {
        const size_t cap = 1024 * n + payload_.size();
        detail::Carve c{codec.stage(staged_bytes() + need<uint8_t>(cap) + need<uint64_t>(n + 1) + need<int32_t>(n))};
        const onc_batch b = stage_batch(c);
        const auto dout = c.take<uint8_t>(cap);
        const auto doff = c.take<uint64_t>(n + 1);
        const auto ds = c.take<int32_t>(n);
        codec.check(onc_encode_body(codec.get(), root(), &b, dout.dev, cap, doff.dev, ds.dev, nullptr),
                    "onc_encode_body");
        codec.sync();
        std::memcpy(st.data(), ds.host, n * 4);
        // a failing message writes nothing (the reference panics or returns
        // before its first write): placeholder extents dropped (ABI 8)
        for (size_t i = 0; i < n; ++i) {
            if (st[i] != ONC_OK) {
                uint64_t kept = 0;
                codec.check(onc_compact(codec.get(), dout.dev, doff.dev, ds.dev, n, &kept), "onc_compact");
                break;
            }
        }
        std::memcpy(off.data(), doff.host, (n + 1) * 8);
        const uint64_t total = off[n];
        out.insert(out.end(), dout.host, dout.host + total);
    }
    if (rec_off) *rec_off = std::move(off);
    return st;
}

// Headers into the stage (at most 1 KiB each, as above), then the plan alone
// (both capacities 0) for the number of marks and pieces, then the fill into
// a stage grown by exactly that (it keeps the entries; pointers re-derived).
inline VectoredStream BatchEncoder::serialise_vectored(Codec& codec, uint32_t max_frag) {
    using detail::need;
    if (root() != ONC_ROOT_RPC_MESSAGE) throw CodecError("serialise_vectored: a body-level batch has no record marks");
    if (max_frag < 1 || max_frag > 0x7FFFFFFFu) throw CodecError("serialise_vectored: max_frag outside 1 .. 0x7FFFFFFF");
    const size_t n = msgs_.size();
    VectoredStream r;
    r.piece_off.assign(n + 1, 0);
    r.out_off.assign(n + 1, 0);
    r.status.assign(n, ONC_OK);
    if (!n) return r;
    const size_t hcap = 1024 * n;
    detail::Carve c{codec.stage(staged_bytes() + need<uint8_t>(hcap) + need<onc_iov_rec>(n) + 2 * need<int32_t>(n) +
                                2 * need<uint64_t>(n + 1) + need<uint64_t>(4))};
    const onc_batch b = stage_batch(c);
    const auto hdr = c.take<uint8_t>(hcap);
    const size_t iov_at = c.off;
    c.take<onc_iov_rec>(n);
    const auto st = c.take<int32_t>(n);
    const size_t fst_at = c.off;
    c.take<int32_t>(n);
    const size_t off_at = c.off;
    c.take<uint64_t>(n + 1);
    const size_t poff_at = c.off;
    c.take<uint64_t>(n + 1);
    const size_t res_at = c.off;
    const auto res = c.take<uint64_t>(4);
    auto iov = [&] { return reinterpret_cast<onc_iov_rec*>(c.s.dev + iov_at); };
    codec.check(onc_encode_iov(codec.get(), &b, hdr.dev, hcap, iov(), st.dev, res.dev), "onc_encode_iov");
    codec.sync();
    std::memcpy(r.status.data(), st.host, n * 4);
    r.headers.assign(hdr.host, hdr.host + size_t(res.host[0]));
    // a failing message writes nothing: placeholder entries emptied (ABI 8)
    for (size_t i = 0; i < n; ++i) {
        if (r.status[i] != ONC_OK) {
            codec.check(onc_compact_iov(codec.get(), iov(), st.dev, n, nullptr), "onc_compact_iov");
            break;
        }
    }
    auto fragment = [&](uint8_t* marks, uint64_t marks_cap, onc_frag_piece* pieces, uint64_t max_pieces) {
        uint8_t* d = c.s.dev;
        codec.check(onc_fragment_iov(codec.get(), iov(), n, max_frag, nullptr, marks, marks_cap, pieces, max_pieces,
                                     reinterpret_cast<uint64_t*>(d + off_at), reinterpret_cast<uint64_t*>(d + poff_at),
                                     reinterpret_cast<int32_t*>(d + fst_at), reinterpret_cast<uint64_t*>(d + res_at)),
                    "onc_fragment_iov");
        codec.sync();
    };
    fragment(nullptr, 0, nullptr, 0);
    uint64_t d[4];
    std::memcpy(d, c.s.host + res_at, sizeof(d));
    const size_t nf = size_t(d[0]), np = size_t(d[3]);
    const size_t kept = c.off;
    c.s = codec.stage(kept + need<uint8_t>(4 * nf) + need<onc_frag_piece>(np), kept);
    const auto marks = c.take<uint8_t>(4 * nf);
    const auto pieces = c.take<onc_frag_piece>(np);
    fragment(marks.dev, 4 * nf, pieces.dev, np);
    const int32_t* fs = reinterpret_cast<const int32_t*>(c.s.host + fst_at);
    for (size_t i = 0; i < n; ++i)
        if (fs[i] != ONC_OK) throw CodecError(std::string("onc_fragment_iov: ") + onc_status_str(fs[i]));
    r.marks.assign(marks.host, marks.host + 4 * nf);
    r.pieces.assign(pieces.host, pieces.host + np);
    std::memcpy(r.out_off.data(), c.s.host + off_at, (n + 1) * 8);
    std::memcpy(r.piece_off.data(), c.s.host + poff_at, (n + 1) * 8);
    r.n_frags = nf;
    r.n_multi = size_t(d[2]);
    r.bytes = d[1];
    return r;
}

// serialise_vectored's steps with the stream gathered on the device: after the
// plan the stage grows by the marks, the pieces, their positions and the
// stream itself (it keeps the batch, the headers and the entries; every
// pointer is re-derived from its offset), and the sources of the gather are the
// stage's own regions.
inline FragmentedStream BatchEncoder::serialise_fragmented(Codec& codec, uint32_t max_frag,
                                                           const std::vector<uint32_t>* rec_limits) {
    using detail::need;
    if (root() != ONC_ROOT_RPC_MESSAGE) throw CodecError("serialise_fragmented: a body-level batch has no record marks");
    if (max_frag < 1 || max_frag > 0x7FFFFFFFu) throw CodecError("serialise_fragmented: max_frag outside 1 .. 0x7FFFFFFF");
    const size_t n = msgs_.size();
    if (rec_limits && rec_limits->size() != n) throw CodecError("serialise_fragmented: one limit per message");
    FragmentedStream r;
    r.out_off.assign(n + 1, 0);
    r.status.assign(n, ONC_OK);
    if (!n) return r;
    const size_t hcap = 1024 * n;
    detail::Carve c{codec.stage(staged_bytes() + need<uint8_t>(hcap) + need<onc_iov_rec>(n) + 2 * need<int32_t>(n) +
                                need<uint32_t>(n) + 2 * need<uint64_t>(n + 1) + need<uint64_t>(4) + need<uint64_t>(3))};
    const onc_batch b = stage_batch(c);
    const size_t pay_at = size_t(b.payload_arena - c.s.dev);
    const size_t hdr_at = c.off;
    const auto hdr = c.take<uint8_t>(hcap);
    const size_t iov_at = c.off;
    c.take<onc_iov_rec>(n);
    const auto st = c.take<int32_t>(n);
    const size_t fst_at = c.off;
    c.take<int32_t>(n);
    const size_t lim_at = c.off;
    const auto lim = c.take<uint32_t>(n);
    const size_t off_at = c.off;
    c.take<uint64_t>(n + 1);
    const size_t poff_at = c.off;
    c.take<uint64_t>(n + 1);
    const size_t res_at = c.off;
    const auto res = c.take<uint64_t>(4);
    const size_t gres_at = c.off;
    c.take<uint64_t>(3);
    if (rec_limits) std::memcpy(lim.host, rec_limits->data(), n * 4);
    auto iov = [&] { return reinterpret_cast<onc_iov_rec*>(c.s.dev + iov_at); };
    codec.check(onc_encode_iov(codec.get(), &b, hdr.dev, hcap, iov(), st.dev, res.dev), "onc_encode_iov");
    codec.sync();
    std::memcpy(r.status.data(), st.host, n * 4);
    const uint64_t hdr_len = res.host[0];
    // a failing message writes nothing: placeholder entries emptied (ABI 8)
    for (size_t i = 0; i < n; ++i) {
        if (r.status[i] != ONC_OK) {
            codec.check(onc_compact_iov(codec.get(), iov(), st.dev, n, nullptr), "onc_compact_iov");
            break;
        }
    }
    auto fragment = [&](uint8_t* marks, uint64_t marks_cap, onc_frag_piece* pieces, uint64_t max_pieces) {
        uint8_t* d = c.s.dev;
        codec.check(onc_fragment_iov(codec.get(), iov(), n, max_frag,
                                     rec_limits ? reinterpret_cast<const uint32_t*>(d + lim_at) : nullptr, marks, marks_cap,
                                     pieces, max_pieces, reinterpret_cast<uint64_t*>(d + off_at),
                                     reinterpret_cast<uint64_t*>(d + poff_at), reinterpret_cast<int32_t*>(d + fst_at),
                                     reinterpret_cast<uint64_t*>(d + res_at)),
                    "onc_fragment_iov");
    };
    fragment(nullptr, 0, nullptr, 0);
    codec.sync();
    uint64_t d[4];
    std::memcpy(d, c.s.host + res_at, sizeof(d));
    const size_t nf = size_t(d[0]), np = size_t(d[3]), total = size_t(d[1]);
    const size_t kept = c.off;
    c.s = codec.stage(kept + need<uint8_t>(4 * nf) + need<onc_frag_piece>(np) + need<uint64_t>(np + 1) + need<uint8_t>(total),
                      kept);
    const auto marks = c.take<uint8_t>(4 * nf);
    const auto pieces = c.take<onc_frag_piece>(np);
    const auto pos = c.take<uint64_t>(np + 1);
    const auto out = c.take<uint8_t>(total);
    fragment(marks.dev, 4 * nf, pieces.dev, np);
    onc_gather_src src{};
    src.base[ONC_PIECE_MARK] = marks.dev;
    src.len[ONC_PIECE_MARK] = 4 * nf;
    src.base[ONC_PIECE_HDR] = c.s.dev + hdr_at;
    src.len[ONC_PIECE_HDR] = hdr_len;
    src.base[ONC_PIECE_PAYLOAD] = c.s.dev + pay_at;
    src.len[ONC_PIECE_PAYLOAD] = payload_.size();
    uint64_t* gres = reinterpret_cast<uint64_t*>(c.s.dev + gres_at);
    codec.check(onc_piece_offsets(codec.get(), pieces.dev, np, &src, pos.dev, gres), "onc_piece_offsets");
    codec.check(onc_gather_pieces(codec.get(), pieces.dev, pos.dev, np, &src, 0, total, out.dev), "onc_gather_pieces");
    codec.sync();
    uint64_t g[3];
    std::memcpy(g, c.s.host + gres_at, sizeof(g));
    if (g[0] != total || g[1] != 0) throw CodecError("serialise_fragmented: the piece list does not match its sources");
    const int32_t* fs = reinterpret_cast<const int32_t*>(c.s.host + fst_at);
    for (size_t i = 0; i < n; ++i)
        if (r.status[i] == ONC_OK) r.status[i] = fs[i];      // ONC_ENC_BAD_DESCRIPTOR: its own limit is no fragment size
    r.bytes.assign(out.host, out.host + total);
    std::memcpy(r.out_off.data(), c.s.host + off_at, (n + 1) * 8);
    r.n_frags = nf;
    r.n_multi = size_t(d[2]);
    return r;
}

// ----------------------------------------------------------------------------
// BatchDecoder implementation: descriptors -> RpcMessage views over `wire`
// ----------------------------------------------------------------------------
namespace detail {

inline AuthFlavor auth_view(const onc_auth& a, const onc_unix_params* unix, const uint8_t* wire) {
    const uint32_t kind = ONC_AUTH_KIND(a);
    const uint32_t len = ONC_AUTH_LEN(a);
    switch (kind) {
        case ONC_KIND_NONE:
            // AuthNone with an empty body decodes to None (flavor.rs:71-78)
            return len == 0 ? AuthFlavor::none() : AuthFlavor::none(Bytes(wire + a.ref, len));
        case ONC_KIND_UNIX: {
            const onc_unix_params& u = unix[a.ref];
            return AuthFlavor::unix(AuthUnixParams(u.stamp, Bytes(wire + u.name_off, u.name_len), u.uid, u.gid,
                                                   std::vector<uint32_t>(u.gids, u.gids + u.ngids)));
        }
        case ONC_KIND_SHORT: return AuthFlavor::short_(Bytes(wire + a.ref, len));
        default: return AuthFlavor::unknown(a.id, Bytes(wire + a.ref, len));
    }
}

inline RpcMessage message_view(const onc_msg& d, const onc_unix_params* unix, const uint8_t* wire) {
    if (d.msg_type == ONC_MSG_CALL) {
        return RpcMessage(d.xid, MessageType::call(CallBody(d.u.call.program, d.u.call.program_version,
                                                            d.u.call.procedure, auth_view(d.cred, unix, wire),
                                                            auth_view(d.verf, unix, wire),
                                                            Bytes(wire + d.payload_off, d.payload_len))));
    }
    if (d.reply_stat == ONC_REPLY_ACCEPTED) {
        AcceptedStatus s = AcceptedStatus::of(AcceptedStatus::Kind(d.stat));
        if (d.stat == ONC_ACCEPT_SUCCESS) s = AcceptedStatus::success(Bytes(wire + d.payload_off, d.payload_len));
        if (d.stat == ONC_ACCEPT_PROG_MISMATCH) s = AcceptedStatus::program_mismatch(d.u.mismatch.low, d.u.mismatch.high);
        return RpcMessage(d.xid, MessageType::reply(ReplyBody::accepted(
                                     AcceptedReply(auth_view(d.verf, unix, wire), std::move(s)))));
    }
    RejectedReply j = d.stat == ONC_REJECT_RPC_MISMATCH
                          ? RejectedReply::rpc_version_mismatch(d.u.mismatch.low, d.u.mismatch.high)
                          : RejectedReply::auth_error(AuthError(d.auth_stat));
    return RpcMessage(d.xid, MessageType::reply(ReplyBody::denied(j)));
}

}  // namespace detail

inline size_t BatchDecoder::out_bytes(size_t n) {
    using detail::need;
    return need<onc_msg>(n) + need<onc_unix_params>(2 * n) + need<int32_t>(n) + 2 * need<uint32_t>(n);
}

inline BatchDecoder::Out BatchDecoder::take_out(detail::Carve& c, size_t n) {
    Out o;
    o.msgs = c.take<onc_msg>(n);
    o.unix = c.take<onc_unix_params>(2 * n);
    o.status = c.take<int32_t>(n);
    o.aux0 = c.take<uint32_t>(n);
    o.aux1 = c.take<uint32_t>(n);
    return o;
}

// Descriptors -> RpcMessage views over the caller's `wire` (offsets in the
// descriptors are relative to the decoded buffer, the same bytes).
inline std::vector<Decoded> BatchDecoder::results(const Out& o, size_t n, const uint8_t* wire) {
    std::vector<Decoded> res(n);
    for (size_t i = 0; i < n; ++i) {
        res[i].status = o.status.host[i];
        res[i].aux0 = o.aux0.host[i];
        res[i].aux1 = o.aux1.host[i];
        if (res[i].status == ONC_OK) res[i].message = detail::message_view(o.msgs.host[i], o.unix.host, wire);
    }
    return res;
}

// The wire is copied into the stage (the caller's buffer is not pinned) and
// decoded there in place by onc_decode_lengths (offsets inside the decode:
// one pass); the outputs land in the stage.
inline std::vector<Decoded> BatchDecoder::try_from(Codec& codec, const uint8_t* wire, size_t wire_len,
                                                   const std::vector<uint32_t>& rec_len, DecodeMode mode) {
    return lengths_at(codec, wire, nullptr, wire_len, rec_len, mode);
}

inline std::vector<Decoded> BatchDecoder::lengths_at(Codec& codec, const uint8_t* wire, const uint8_t* dev_wire,
                                                     size_t wire_len, const std::vector<uint32_t>& rec_len,
                                                     DecodeMode mode) {
    using detail::need;
    const size_t n = rec_len.size();
    if (!n) return {};
    detail::Carve c{codec.stage((dev_wire ? 0 : need<uint8_t>(wire_len)) + need<uint32_t>(n) + out_bytes(n))};
    const uint8_t* wd = dev_wire;
    if (!dev_wire) {
        const auto w = c.take<uint8_t>(wire_len);
        if (wire_len) std::memcpy(w.host, wire, wire_len);
        wd = w.dev;
    }
    const auto l = c.take<uint32_t>(n);
    std::memcpy(l.host, rec_len.data(), n * 4);
    const Out o = take_out(c, n);
    const onc_decoded d = o.dev();
    // bounded: the lengths are the caller's, wire_len is what was staged or
    // registered — a record running past it is Error(ONC_DEC_BAD_EXTENT), unread
    codec.check(onc_decode_lengths_bounded(codec.get(), wd, wire_len, l.dev, n, 0, int(mode), nullptr, &d),
                "onc_decode_lengths_bounded");
    codec.sync();
    return results(o, n, wire);
}

inline std::vector<Decoded> BatchDecoder::try_from_stream(Codec& codec, const uint8_t* wire, size_t wire_len,
                                                          DecodeMode mode, size_t* consumed,
                                                          std::optional<Error>* stop) {
    return stream_at(codec, wire, nullptr, wire_len, mode, consumed, stop);
}

inline std::vector<Decoded> BatchDecoder::stream_at(Codec& codec, const uint8_t* wire, const uint8_t* dev_wire,
                                                    size_t wire_len, DecodeMode mode, size_t* consumed,
                                                    std::optional<Error>* stop) {
    using detail::need;
    // framed first with only the wire, the offsets (every record is at least
    // 4 bytes) and the result words staged; the decode outputs are carved
    // for the framed count afterwards (sized for max_records they would be
    // ~67 bytes of pinned memory per wire byte)
    const size_t max_records = wire_len / 4 + 1;
    detail::Carve c{codec.stage((dev_wire ? 0 : need<uint8_t>(wire_len)) + need<uint64_t>(max_records + 1) +
                                need<uint64_t>(5))};
    const uint8_t* wd = dev_wire;
    if (!dev_wire) {
        const auto w = c.take<uint8_t>(wire_len);
        if (wire_len) std::memcpy(w.host, wire, wire_len);
        wd = w.dev;
    }
    const size_t off_at = c.off;
    const auto off = c.take<uint64_t>(max_records + 1);
    const auto res = c.take<uint64_t>(5);
    codec.check(onc_frame_stream(codec.get(), wd, wire_len, off.dev, max_records, res.dev), "onc_frame_stream");
    codec.sync();
    uint64_t r[5];
    std::memcpy(r, res.host, sizeof(r));
    if (consumed) *consumed = size_t(r[1]);
    if (stop) {
        if (int32_t(r[2]) == ONC_OK) *stop = std::nullopt;
        else *stop = Error(int32_t(r[2]), uint32_t(r[3]), uint32_t(r[4]));
    }
    const size_t n = size_t(r[0]);
    if (!n) return {};
    // the outputs after what is staged (a stage that grows keeps the staged
    // wire and offsets; their device addresses move with it)
    const size_t mark = c.off;
    c.s = codec.stage(mark + out_bytes(n), mark);
    if (!dev_wire) wd = c.s.dev;
    const uint64_t* offd = reinterpret_cast<const uint64_t*>(c.s.dev + off_at);
    const Out o = take_out(c, n);
    const onc_decoded d = o.dev();
    codec.check(onc_decode(codec.get(), wd, offd, n, int(mode), &d), "onc_decode");
    codec.sync();
    return results(o, n, wire);
}

inline std::vector<Decoded> BatchDecoder::streams_at(Codec& codec, const uint8_t* wire, const uint8_t* dev_wire,
                                                     size_t wire_len, const std::vector<Segment>& segments,
                                                     std::vector<SegmentResult>* per_segment, DecodeMode mode) {
    using detail::need;
    const size_t nseg = segments.size();
    if (per_segment) per_segment->assign(nseg, SegmentResult{});
    if (!nseg) return {};
    // a segment must lie in the wire (the framer trusts its segment list);
    // every record is at least 4 bytes
    size_t max_records = 1;
    for (const Segment& g : segments) {
        if (g.off > wire_len || g.len > wire_len - g.off) throw CodecError("try_from_streams: segment outside the wire");
        max_records += size_t(g.len / 4);
    }
    detail::Carve c{codec.stage((dev_wire ? 0 : need<uint8_t>(wire_len)) + 2 * need<uint64_t>(nseg) +
                                need<uint64_t>(max_records) + need<uint32_t>(max_records) + need<uint64_t>(6 * nseg) +
                                need<uint64_t>(3))};
    const uint8_t* wd = dev_wire;
    if (!dev_wire) {
        const auto w = c.take<uint8_t>(wire_len);
        if (wire_len) std::memcpy(w.host, wire, wire_len);
        wd = w.dev;
    }
    const auto so = c.take<uint64_t>(nseg);
    const auto sl = c.take<uint64_t>(nseg);
    for (size_t i = 0; i < nseg; ++i) {
        so.host[i] = segments[i].off;
        sl.host[i] = segments[i].len;
    }
    const size_t start_at = c.off;
    const auto start = c.take<uint64_t>(max_records);
    const size_t len_at = c.off;
    const auto len = c.take<uint32_t>(max_records);
    const auto rows = c.take<uint64_t>(6 * nseg);
    const auto res = c.take<uint64_t>(3);
    codec.check(onc_frame_streams(codec.get(), wd, so.dev, sl.dev, nseg, start.dev, len.dev, nullptr, max_records,
                                  rows.dev, res.dev),
                "onc_frame_streams");
    codec.sync();
    if (per_segment) {
        for (size_t i = 0; i < nseg; ++i) {
            const uint64_t* r = rows.host + 6 * i;
            (*per_segment)[i] = SegmentResult{r[0], r[1], r[2], int32_t(r[3]), uint32_t(r[4]), uint32_t(r[5])};
        }
    }
    const size_t n = size_t(res.host[0]);
    if (!n) return {};
    // the outputs after what is staged (a stage that grows keeps the staged
    // wire and extents; their device addresses move with it)
    const size_t mark = c.off;
    c.s = codec.stage(mark + out_bytes(n), mark);
    if (!dev_wire) wd = c.s.dev;
    const Out o = take_out(c, n);
    const onc_decoded d = o.dev();
    codec.check(onc_decode_extents(codec.get(), wd, wire_len, reinterpret_cast<const uint64_t*>(c.s.dev + start_at),
                                   reinterpret_cast<const uint32_t*>(c.s.dev + len_at), n, int(mode), &d),
                "onc_decode_extents");
    codec.sync();
    return results(o, n, wire);
}

// ----------------------------------------------------------------------------
// Multi-fragment record streams (RFC 5531 §11) — the reference rejects them
// (Error::Fragmented, rpc_message.rs:359-362; README.md:62)
// ----------------------------------------------------------------------------
// A socket read buffer whose records may come in several fragments, rebuilt
// on the device (onc_frame_fragments + onc_defragment) as the packed stream
// of single-fragment records serialise_into would have written. `bytes` goes
// to BatchDecoder::try_from_stream as it is; the decoded payload views then
// point into `bytes`, which must outlive them.
struct Reassembled {
    std::vector<uint8_t> bytes;      // the reassembled stream (rec_off.back() bytes)
    std::vector<uint64_t> rec_off;   // n + 1 offsets into bytes
    std::vector<int32_t> status;     // per record: ONC_OK or ONC_ENC_TOO_LONG (a body of 2^31 bytes or more)
    size_t consumed = 0;             // wire bytes of the complete records: keep the rest for the next read
    size_t pending_frags = 0;        // framed fragments after the last complete record
    size_t pending_body_bytes = 0;
    size_t n_multi = 0;              // records that came in more than one fragment
    std::optional<Error> stop;       // why fragment framing stopped before the buffer's end, if it did
};

inline Reassembled reassemble_stream(Codec& codec, const uint8_t* wire, size_t len) {
    using detail::need;
    Reassembled r;
    r.rec_off.assign(1, 0);
    const size_t max_frags = len / 4 + 1;
    detail::Carve c{codec.stage(need<uint8_t>(len) + need<uint64_t>(max_frags + 1) + need<uint64_t>(5))};
    const auto w = c.take<uint8_t>(len);
    if (len) std::memcpy(w.host, wire, len);
    const size_t frag_at = c.off;
    const auto frag = c.take<uint64_t>(max_frags + 1);
    const auto fres = c.take<uint64_t>(5);
    codec.check(onc_frame_fragments(codec.get(), w.dev, len, frag.dev, max_frags, fres.dev), "onc_frame_fragments");
    codec.sync();
    uint64_t f[5];
    std::memcpy(f, fres.host, sizeof(f));
    if (int32_t(f[2]) != ONC_OK) r.stop = Error(int32_t(f[2]), uint32_t(f[3]), uint32_t(f[4]));
    const size_t nfrag = size_t(f[0]);
    if (!nfrag) return r;
    // the outputs after what is staged (a stage that grows keeps it); a
    // reassembled record is never longer than its fragments
    const size_t mark = c.off;
    const size_t cap = size_t(f[1]);
    c.s = codec.stage(mark + need<uint8_t>(cap) + need<uint64_t>(nfrag + 1) + need<int32_t>(nfrag) + need<uint64_t>(6),
                      mark);
    const auto out = c.take<uint8_t>(cap);
    const auto off = c.take<uint64_t>(nfrag + 1);
    const auto st = c.take<int32_t>(nfrag);
    const auto res = c.take<uint64_t>(6);
    codec.check(onc_defragment(codec.get(), c.s.dev, reinterpret_cast<const uint64_t*>(c.s.dev + frag_at), nfrag,
                               out.dev, cap, off.dev, st.dev, res.dev),
                "onc_defragment");
    codec.sync();
    uint64_t d[6];
    std::memcpy(d, res.host, sizeof(d));
    const size_t n = size_t(d[0]);
    r.bytes.assign(out.host, out.host + d[2]);
    r.rec_off.assign(off.host, off.host + n + 1);
    r.status.assign(st.host, st.host + n);
    r.consumed = size_t(d[1]);
    r.pending_frags = size_t(d[3]);
    r.pending_body_bytes = size_t(d[4]);
    r.n_multi = size_t(d[5]);
    return r;
}

// The same for many connections' buffers at once (segments of one slab, as
// BatchDecoder::try_from_streams takes them): the fragments of every segment's
// complete records found in one call (onc_frame_fragment_streams) and rebuilt
// in one call (onc_defragment_extents) as one packed stream of single-fragment
// records, ordered by segment. A segment's records are [first_rec, first_rec +
// n_rec) of rec_off; `consumed` bytes of it are done with — up to the end of
// its last complete record: a pending run stays in the buffer — and status
// says why its walk stopped (ONC_OK: at its end or on a fragment boundary).
struct SegmentRecords {
    uint64_t first_rec = 0, n_rec = 0, consumed = 0;
    int32_t status = ONC_OK;
    uint32_t aux0 = 0, aux1 = 0;
    bool ok() const { return status == ONC_OK; }
    Error error() const { return Error(status, aux0, aux1); }
};
struct ReassembledStreams {
    std::vector<uint8_t> bytes;      // the reassembled stream (rec_off.back() bytes)
    std::vector<uint64_t> rec_off;   // n + 1 offsets into bytes
    std::vector<int32_t> status;     // per record: ONC_OK or ONC_ENC_TOO_LONG
    size_t n_frags = 0;              // fragments the records came in
    size_t n_multi = 0;              // records that came in more than one fragment
};

inline ReassembledStreams reassemble_streams(Codec& codec, const uint8_t* wire, size_t wire_len,
                                             const std::vector<Segment>& segments,
                                             std::vector<SegmentRecords>* per_segment = nullptr) {
    using detail::need;
    ReassembledStreams r;
    r.rec_off.assign(1, 0);
    const size_t nseg = segments.size();
    if (per_segment) per_segment->assign(nseg, SegmentRecords{});
    if (!nseg) return r;
    // a segment must lie in the wire (the framer trusts its segment list);
    // every fragment is at least 4 bytes
    size_t max_frags = 1;
    for (const Segment& g : segments) {
        if (g.off > wire_len || g.len > wire_len - g.off) throw CodecError("reassemble_streams: segment outside the wire");
        max_frags += size_t(g.len / 4);
    }
    detail::Carve c{codec.stage(need<uint8_t>(wire_len) + 2 * need<uint64_t>(nseg) + need<uint64_t>(max_frags) +
                                need<uint32_t>(max_frags) + need<uint64_t>(8 * nseg) + need<uint64_t>(4))};
    const auto w = c.take<uint8_t>(wire_len);
    if (wire_len) std::memcpy(w.host, wire, wire_len);
    const auto so = c.take<uint64_t>(nseg);
    const auto sl = c.take<uint64_t>(nseg);
    for (size_t i = 0; i < nseg; ++i) {
        so.host[i] = segments[i].off;
        sl.host[i] = segments[i].len;
    }
    const size_t start_at = c.off;
    const auto start = c.take<uint64_t>(max_frags);
    const size_t len_at = c.off;
    const auto len = c.take<uint32_t>(max_frags);
    const auto rows = c.take<uint64_t>(8 * nseg);
    const auto fres = c.take<uint64_t>(4);
    codec.check(onc_frame_fragment_streams(codec.get(), w.dev, so.dev, sl.dev, nseg, start.dev, len.dev, nullptr,
                                           max_frags, rows.dev, fres.dev),
                "onc_frame_fragment_streams");
    codec.sync();
    size_t cap = 0;                  // a reassembled record is never longer than its fragments
    for (size_t i = 0; i < nseg; ++i) {
        const uint64_t* q = rows.host + 8 * i;
        cap += size_t(q[2]);
        if (per_segment)
            (*per_segment)[i] = SegmentRecords{q[6], q[7], q[2], int32_t(q[3]), uint32_t(q[4]), uint32_t(q[5])};
    }
    const size_t nfrag = size_t(fres.host[0]);
    r.n_frags = nfrag;
    if (!nfrag) return r;
    // the outputs after what is staged (a stage that grows keeps it)
    const size_t mark = c.off;
    c.s = codec.stage(mark + need<uint8_t>(cap) + need<uint64_t>(nfrag + 1) + need<int32_t>(nfrag) + need<uint64_t>(6),
                      mark);
    const auto out = c.take<uint8_t>(cap);
    const auto off = c.take<uint64_t>(nfrag + 1);
    const auto st = c.take<int32_t>(nfrag);
    const auto res = c.take<uint64_t>(6);
    codec.check(onc_defragment_extents(codec.get(), c.s.dev, reinterpret_cast<const uint64_t*>(c.s.dev + start_at),
                                       reinterpret_cast<const uint32_t*>(c.s.dev + len_at), nfrag, out.dev, cap,
                                       off.dev, st.dev, res.dev),
                "onc_defragment_extents");
    codec.sync();
    uint64_t d[6];
    std::memcpy(d, res.host, sizeof(d));
    const size_t n = size_t(d[0]);
    r.bytes.assign(out.host, out.host + d[2]);
    r.rec_off.assign(off.host, off.host + n + 1);
    r.status.assign(st.host, st.host + n);
    r.n_multi = size_t(d[5]);
    return r;
}

// The heads of many connections' fragmented records (reassemble_streams
// without the payloads): the fragments of every segment's complete records
// found in one call (onc_frame_fragment_streams) and the first head_len bytes
// of every record — its synthesised mark included — gathered into fixed-stride
// slots in one call (onc_defragment_heads). The rest of a record stays in the
// caller's wire: pieces() lists any range of it as slices of that wire.
struct ReassembledHeads {
    uint32_t head_len = 0;
    std::vector<uint8_t> heads;        // n * head_len: slot r at r * head_len, min(rec_len[r], head_len) bytes of it set
    std::vector<uint32_t> rec_len;     // n: the records' true lengths (0: ONC_ENC_TOO_LONG)
    std::vector<int32_t> status;       // n: ONC_OK or ONC_ENC_TOO_LONG
    std::vector<uint64_t> rec_frag;    // n + 1: record r is fragments [rec_frag[r], rec_frag[r + 1])
    std::vector<uint64_t> frag_pre;    // per fragment: the body bytes of its record before it
    std::vector<uint64_t> frag_start;  // per fragment: where it starts in the wire (its mark)
    std::vector<uint32_t> frag_len;    // per fragment: its length, mark included
    size_t n_multi = 0;                // records that came in more than one fragment
    size_t n() const { return rec_len.size(); }
    size_t n_frags() const { return frag_start.size(); }

    // Record bytes [pos, pos + len) of record r (pos >= 4: past the mark,
    // pos + len <= rec_len[r]) as slices of `wire`, in order.
    std::vector<Bytes> pieces(const uint8_t* wire, size_t r, uint64_t pos, uint64_t len) const {
        std::vector<Bytes> out;
        if (!len) return out;
        const uint64_t lo = rec_frag[r], hi = rec_frag[r + 1];
        uint64_t x = pos - 4, left = len;
        // the last fragment j in [lo, hi) with frag_pre[j] <= x
        uint64_t a = lo, b = hi;
        while (b - a > 1) {
            const uint64_t mid = a + (b - a) / 2;
            if (frag_pre[mid] <= x) a = mid;
            else b = mid;
        }
        for (uint64_t j = a; j < hi && left; ++j) {
            const uint64_t body = frag_len[j] - 4, at = x - frag_pre[j];
            if (at >= body) continue;                       // an empty fragment
            const uint64_t take = std::min(left, body - at);
            out.push_back(Bytes(wire + frag_start[j] + 4 + at, size_t(take)));
            x += take;
            left -= take;
        }
        return out;
    }
};

inline ReassembledHeads reassemble_heads(Codec& codec, const uint8_t* wire, size_t wire_len,
                                         const std::vector<Segment>& segments, uint32_t head_len = 160,
                                         std::vector<SegmentRecords>* per_segment = nullptr) {
    using detail::need;
    ReassembledHeads r;
    r.head_len = head_len;
    r.rec_frag.assign(1, 0);
    const size_t nseg = segments.size();
    if (per_segment) per_segment->assign(nseg, SegmentRecords{});
    if (head_len < 64 || head_len > 4096 || head_len % 16) throw CodecError("reassemble_heads: head_len");
    if (!nseg) return r;
    size_t max_frags = 1;
    for (const Segment& g : segments) {
        if (g.off > wire_len || g.len > wire_len - g.off) throw CodecError("reassemble_heads: segment outside the wire");
        max_frags += size_t(g.len / 4);
    }
    detail::Carve c{codec.stage(need<uint8_t>(wire_len) + 2 * need<uint64_t>(nseg) + need<uint64_t>(max_frags) +
                                need<uint32_t>(max_frags) + need<uint64_t>(8 * nseg) + need<uint64_t>(4))};
    const auto w = c.take<uint8_t>(wire_len);
    if (wire_len) std::memcpy(w.host, wire, wire_len);
    const auto so = c.take<uint64_t>(nseg);
    const auto sl = c.take<uint64_t>(nseg);
    for (size_t i = 0; i < nseg; ++i) {
        so.host[i] = segments[i].off;
        sl.host[i] = segments[i].len;
    }
    const size_t start_at = c.off;
    const auto start = c.take<uint64_t>(max_frags);
    const size_t len_at = c.off;
    const auto len = c.take<uint32_t>(max_frags);
    const auto rows = c.take<uint64_t>(8 * nseg);
    const auto fres = c.take<uint64_t>(4);
    codec.check(onc_frame_fragment_streams(codec.get(), w.dev, so.dev, sl.dev, nseg, start.dev, len.dev, nullptr,
                                           max_frags, rows.dev, fres.dev),
                "onc_frame_fragment_streams");
    codec.sync();
    if (per_segment)
        for (size_t i = 0; i < nseg; ++i) {
            const uint64_t* q = rows.host + 8 * i;
            (*per_segment)[i] = SegmentRecords{q[6], q[7], q[2], int32_t(q[3]), uint32_t(q[4]), uint32_t(q[5])};
        }
    const size_t nfrag = size_t(fres.host[0]);
    const size_t nrec = size_t(fres.host[2]);
    if (!nfrag) return r;
    r.frag_start.assign(start.host, start.host + nfrag);
    r.frag_len.assign(len.host, len.host + nfrag);
    // the outputs after what is staged (a stage that grows keeps it)
    const size_t mark = c.off;
    c.s = codec.stage(mark + need<uint8_t>(nrec * head_len) + need<uint32_t>(nfrag) + 2 * need<uint64_t>(nfrag + 1) +
                          need<int32_t>(nfrag) + need<uint64_t>(6),
                      mark);
    const auto heads = c.take<uint8_t>(nrec * head_len);
    const auto rl = c.take<uint32_t>(nfrag);
    const auto rf = c.take<uint64_t>(nfrag + 1);
    const auto fp = c.take<uint64_t>(nfrag + 1);
    const auto st = c.take<int32_t>(nfrag);
    const auto res = c.take<uint64_t>(6);
    std::memset(heads.host, 0, nrec * head_len);            // (slot bytes past a short record stay zero)
    codec.check(onc_defragment_heads(codec.get(), c.s.dev, reinterpret_cast<const uint64_t*>(c.s.dev + start_at),
                                     reinterpret_cast<const uint32_t*>(c.s.dev + len_at), nfrag, head_len, heads.dev,
                                     nrec, rl.dev, rf.dev, fp.dev, st.dev, res.dev),
                "onc_defragment_heads");
    codec.sync();
    uint64_t d[6];
    std::memcpy(d, res.host, sizeof(d));
    const size_t n = size_t(d[0]);
    if (n != nrec) throw CodecError("reassemble_heads: record counts differ");
    r.heads.assign(heads.host, heads.host + n * head_len);
    r.rec_len.assign(rl.host, rl.host + n);
    r.rec_frag.assign(rf.host, rf.host + n + 1);
    r.frag_pre.assign(fp.host, fp.host + nfrag);
    r.status.assign(st.host, st.host + n);
    r.n_multi = size_t(d[5]);
    return r;
}

// What try_from_fragmented_heads returns: the records of all segments in
// segment order (segment s's are results [first_rec, first_rec + n_rec) of
// segments[s]). A result's message borrows `heads.heads` for its auth bodies
// and machine names; its own payload view covers only the payload bytes that
// lie inside the head. The whole payload is payload_pieces(r) — slices of the
// caller's wire, nothing copied — or payload(r), a gathered copy.
// What place_payloads returns: every decoded payload in an aligned slot of one
// device buffer (onc_payload_slots + onc_place_payloads), each payload byte
// moved once from where it arrived. Everything here is device memory, owned by
// this object (one hipMalloc, freed with it): record r's payload is
// views[r].len bytes at the device address views[r].ptr = dev + slot_off[r],
// a multiple of `align` from dev. fetch() copies one back for a look at it.
struct PlacedPayloads {
    uint8_t* dev = nullptr;                // the placed bytes: `bytes` of them
    uint64_t* slot_off_dev = nullptr;      // n + 1 words behind them
    uint64_t bytes = 0;                    // the capacity the slots need (slot_off[n])
    uint32_t align = 1;
    size_t n_payloads = 0;                 // records with a payload
    uint64_t payload_bytes = 0;            // their bytes, unpadded
    std::vector<uint64_t> slot_off;        // n + 1 (a host copy)
    std::vector<Bytes> views;              // n: device addresses; empty for a record without a payload

    PlacedPayloads() = default;
    PlacedPayloads(const PlacedPayloads&) = delete;
    PlacedPayloads& operator=(const PlacedPayloads&) = delete;
    PlacedPayloads(PlacedPayloads&& o) noexcept { *this = std::move(o); }
    PlacedPayloads& operator=(PlacedPayloads&& o) noexcept {
        if (this != &o) {
            if (dev) (void)hipFree(dev);
            dev = o.dev;
            slot_off_dev = o.slot_off_dev;
            bytes = o.bytes;
            align = o.align;
            n_payloads = o.n_payloads;
            payload_bytes = o.payload_bytes;
            slot_off = std::move(o.slot_off);
            views = std::move(o.views);
            o.dev = nullptr;
            o.slot_off_dev = nullptr;
        }
        return *this;
    }
    ~PlacedPayloads() {
        if (dev) (void)hipFree(dev);
    }
    std::vector<uint8_t> fetch(size_t r) const {
        std::vector<uint8_t> out(views[r].len);
        if (!out.empty())
            detail::hip_check(hipMemcpy(out.data(), views[r].ptr, out.size(), hipMemcpyDeviceToHost), "hipMemcpy(payload)");
        return out;
    }
};

namespace detail {

// Where a slab's records lie for onc_place_payloads: the heads form
// (rec_frag / frag_pre set) or the identity form (both null: record r is
// fragment r).
struct PlaceSource {
    const uint8_t* wire;
    size_t wire_len;
    const uint64_t* frag_start;
    const uint32_t* frag_len;
    size_t nfrag;
    const uint64_t* rec_frag;      // n + 1, or null
    const uint64_t* frag_pre;      // nfrag, or null
    const uint32_t* rec_len;       // n
    const uint64_t* rec_start;     // n: onc_payload_slots' rec_start form, or null: the heads form
    uint32_t head_len;
};

// onc_payload_slots + onc_place_payloads of n decoded records, inputs through
// the stage, outputs in one device allocation; one synchronisation.
inline PlacedPayloads place_decoded(Codec& codec, const PlaceSource& s, const onc_msg* msgs, const int32_t* status,
                                    size_t n, uint32_t align) {
    PlacedPayloads p;
    p.align = align;
    p.slot_off.assign(n + 1, 0);
    p.views.assign(n, Bytes());
    if (align == 0 || align > (1u << 20) || (align & (align - 1))) throw CodecError("place_payloads: align");
    if (!n) return p;
    // the capacity is known here too (the device computes the same sum)
    uint64_t cap = 0;
    for (size_t r = 0; r < n; ++r) {
        const onc_msg& m = msgs[r];
        const bool has = status[r] == ONC_OK && m.payload_len &&
                         (m.msg_type == ONC_MSG_CALL || (m.msg_type == ONC_MSG_REPLY && m.reply_stat == ONC_REPLY_ACCEPTED &&
                                                         m.stat == ONC_ACCEPT_SUCCESS));
        if (has) cap += (uint64_t(m.payload_len) + align - 1) & ~uint64_t(align - 1);
    }
    const size_t off_at = size_t((cap + 15) & ~uint64_t(15));
    void* d = nullptr;
    hip_check(hipMalloc(&d, off_at + 8 * (n + 1) + 16), "hipMalloc(placed payloads)");
    p.dev = static_cast<uint8_t*>(d);
    p.slot_off_dev = reinterpret_cast<uint64_t*>(p.dev + off_at);
    const bool heads = s.rec_frag != nullptr;
    Carve c{codec.stage(need<uint8_t>(s.wire_len) + need<uint64_t>(s.nfrag) + need<uint32_t>(s.nfrag) +
                        2 * need<uint64_t>(s.nfrag + 1) + need<uint64_t>(n) + 3 * need<uint32_t>(n) + need<onc_msg>(n) +
                        need<int32_t>(n) + need<uint64_t>(3))};
    const auto w = c.take<uint8_t>(s.wire_len);
    if (s.wire_len) std::memcpy(w.host, s.wire, s.wire_len);
    const auto fs = c.take<uint64_t>(s.nfrag);
    const auto fl = c.take<uint32_t>(s.nfrag);
    const auto rf = c.take<uint64_t>(s.nfrag + 1);
    const auto fp = c.take<uint64_t>(s.nfrag + 1);
    const auto rs = c.take<uint64_t>(n);
    const auto rl = c.take<uint32_t>(n);
    const auto pp = c.take<uint32_t>(n);
    const auto pl = c.take<uint32_t>(n);
    const auto dm = c.take<onc_msg>(n);
    const auto st = c.take<int32_t>(n);
    const auto res = c.take<uint64_t>(3);
    std::memcpy(fs.host, s.frag_start, 8 * s.nfrag);
    std::memcpy(fl.host, s.frag_len, 4 * s.nfrag);
    if (heads) {
        std::memcpy(rf.host, s.rec_frag, 8 * (n + 1));
        std::memcpy(fp.host, s.frag_pre, 8 * s.nfrag);
    }
    if (s.rec_start) std::memcpy(rs.host, s.rec_start, 8 * n);
    std::memcpy(rl.host, s.rec_len, 4 * n);
    std::memcpy(dm.host, msgs, sizeof(onc_msg) * n);
    std::memcpy(st.host, status, 4 * n);
    codec.check(onc_payload_slots(codec.get(), dm.dev, st.dev, n, s.head_len, s.rec_start ? rs.dev : nullptr, align,
                                  pp.dev, pl.dev, p.slot_off_dev, nullptr, res.dev),
                "onc_payload_slots");
    codec.check(onc_place_payloads(codec.get(), w.dev, fs.dev, fl.dev, s.nfrag, heads ? rf.dev : nullptr,
                                   heads ? fp.dev : nullptr, rl.dev, pp.dev, pl.dev, p.slot_off_dev, n, p.dev, cap),
                "onc_place_payloads");
    codec.sync();
    hip_check(hipMemcpy(p.slot_off.data(), p.slot_off_dev, 8 * (n + 1), hipMemcpyDeviceToHost), "hipMemcpy(slot_off)");
    p.n_payloads = size_t(res.host[0]);
    p.payload_bytes = res.host[1];
    p.bytes = res.host[2];
    if (p.bytes != cap || p.slot_off[n] != cap) throw CodecError("place_payloads: capacities differ");
    for (size_t r = 0; r < n; ++r)
        if (pl.host[r]) p.views[r] = Bytes(p.dev + p.slot_off[r], pl.host[r]);
    return p;
}

}  // namespace detail

struct FragmentedHeads {
    std::vector<Decoded> results;
    std::vector<SegmentRecords> segments;
    ReassembledHeads heads;
    std::vector<uint64_t> payload_pos;     // per record: where its payload starts in the record (0: none)
    std::vector<uint64_t> payload_len;     // per record: its true length
    std::vector<onc_msg> descriptors;      // per record: as onc_decode_heads wrote it (offsets count from heads.heads)
    std::vector<int32_t> status;           // per record: its decode status
    const uint8_t* wire = nullptr;
    bool retried = false;                  // a header did not fit head_len: decoded from 736-byte heads

    // Every payload gathered from its fragments into an `align`-aligned slot
    // of one device buffer, on the device (onc_payload_slots +
    // onc_place_payloads; payload(r) below walks the fragments on the host).
    PlacedPayloads place_payloads(Codec& codec, uint32_t align = 16) const {
        const size_t nfrag = heads.n_frags();
        size_t wire_len = 0;
        for (size_t j = 0; j < nfrag; ++j)
            wire_len = std::max<size_t>(wire_len, size_t(heads.frag_start[j] + heads.frag_len[j]));
        const detail::PlaceSource s{wire, wire_len, heads.frag_start.data(), heads.frag_len.data(), nfrag,
                                    heads.rec_frag.data(), heads.frag_pre.data(), heads.rec_len.data(), nullptr,
                                    heads.head_len};
        return detail::place_decoded(codec, s, descriptors.data(), status.data(), descriptors.size(), align);
    }

    std::vector<Bytes> payload_pieces(size_t r) const {
        if (!payload_len[r]) return {};
        return heads.pieces(wire, r, payload_pos[r], payload_len[r]);
    }
    std::vector<uint8_t> payload(size_t r) const {
        std::vector<uint8_t> out;
        out.reserve(size_t(payload_len[r]));
        for (const Bytes& b : payload_pieces(r)) out.insert(out.end(), b.ptr, b.ptr + b.len);
        return out;
    }
};

// The same for records decoded where they lie — try_from_streams' results (or
// try_from_stream's, try_from's), whose payload views point into the caller's
// `wire` at arbitrary byte addresses: every payload moved once into an
// `align`-aligned slot of one device buffer, after which the wire can be
// reused (onc_payload_slots' rec_start form + onc_place_payloads' identity
// form; a record is described by its payload's extent alone).
inline PlacedPayloads place_payloads(Codec& codec, const uint8_t* wire, size_t wire_len,
                                     const std::vector<Decoded>& results, uint32_t align = 16) {
    const size_t n = results.size();
    std::vector<onc_msg> msgs(n);
    std::vector<int32_t> status(n);
    std::vector<uint64_t> start(n, 0);
    std::vector<uint32_t> len(n, 4);
    for (size_t r = 0; r < n; ++r) {
        std::memset(&msgs[r], 0, sizeof(onc_msg));
        status[r] = results[r].status;
        if (!results[r].ok()) continue;
        const RpcMessage& m = *results[r].message;
        Bytes p;
        if (const CallBody* cb = m.call_body()) {
            p = cb->payload();
        } else if (const AcceptedReply* a = m.reply_body()->accepted()) {
            if (a->status().kind() == AcceptedStatus::Kind::Success) p = a->status().payload();
        }
        if (!p.len) continue;
        if (p.ptr < wire + 4 || p.ptr + p.len > wire + wire_len) throw CodecError("place_payloads: a payload outside the wire");
        msgs[r].msg_type = ONC_MSG_CALL;
        msgs[r].payload_len = uint32_t(p.len);
        msgs[r].payload_off = uint64_t(p.ptr - wire);
        start[r] = msgs[r].payload_off - 4;                  // the four bytes before it stand for a mark: never read
        len[r] = uint32_t(p.len) + 4;
    }
    const detail::PlaceSource s{wire, wire_len, start.data(), len.data(), n, nullptr, nullptr, len.data(), start.data(), 0};
    return detail::place_decoded(codec, s, msgs.data(), status.data(), n, align);
}

// ----------------------------------------------------------------------------
// Dispatch: decoded Calls to their handlers (onc_route_calls)
// ----------------------------------------------------------------------------
// A server's route table: which handler serves procedures [proc_first,
// proc_first + proc_count) of a (program, version). Rows are given in any
// order; sorted() puts them in the order the device wants and refuses
// overlapping ranges, empty ranges, unknown flags and handlers beyond
// n_handlers() on the host (CodecError), so the device never sees a bad table.
class RouteTable {
public:
    explicit RouteTable(uint32_t n_handlers) : nh_(n_handlers) {
        if (n_handlers > ONC_ROUTE_HANDLERS_MAX) throw CodecError("RouteTable: too many handlers");
    }
    // handler of procedure p: handler_first + (p - proc_first), or
    // handler_first for every p with ONC_ROUTE_ONE_HANDLER in flags
    RouteTable& add(uint32_t program, uint32_t version, uint32_t proc_first, uint32_t proc_count,
                    uint32_t handler_first, uint32_t flags = 0) {
        if (rows_.size() == ONC_ROUTE_TABLE_MAX) throw CodecError("RouteTable: too many entries");
        rows_.push_back(onc_route{program, version, proc_first, proc_count, handler_first, flags});
        return *this;
    }
    uint32_t n_handlers() const { return nh_; }
    size_t size() const { return rows_.size(); }
    std::vector<onc_route> sorted() const {
        std::vector<onc_route> t = rows_;
        std::sort(t.begin(), t.end(), [](const onc_route& a, const onc_route& b) {
            return std::tie(a.program, a.version, a.proc_first) < std::tie(b.program, b.version, b.proc_first);
        });
        for (size_t i = 0; i < t.size(); ++i) {
            const onc_route& e = t[i];
            const uint64_t end = uint64_t(e.proc_first) + e.proc_count;
            if (e.proc_count == 0 || end > (uint64_t(1) << 32)) throw CodecError("RouteTable: an empty or wrapping range");
            if (e.flags & ~uint32_t(ONC_ROUTE_ONE_HANDLER)) throw CodecError("RouteTable: unknown flags");
            if (uint64_t(e.handler_first) + ((e.flags & ONC_ROUTE_ONE_HANDLER) ? 1u : e.proc_count) > nh_)
                throw CodecError("RouteTable: a handler beyond n_handlers");
            if (i + 1 < t.size() && t[i + 1].program == e.program && t[i + 1].version == e.version &&
                t[i + 1].proc_first < end)
                throw CodecError("RouteTable: procedure ranges overlap");
        }
        return t;
    }

private:
    uint32_t nh_;
    std::vector<onc_route> rows_;
};

// What route_calls returns: the records grouped stably by bin — handler h's
// Calls, the Calls no route serves, the records that are no Calls, the failed
// ones — as positions in `order`. calls[k] / replies[k] describe record
// order[k]: its Call descriptor (xid, program, version, procedure; the
// payload and the auths stay in the Decoded result order[k] points at) and its
// reply descriptor (a Success skeleton for a served Call, the finished RFC 5531
// §9 rejection for the others).
struct RoutedCalls {
    struct Span {
        const onc_msg* calls = nullptr;    // n Call descriptors, in arrival order
        const onc_msg* replies = nullptr;  // their reply descriptors
        const uint32_t* index = nullptr;   // their positions in the decoded batch
        size_t n = 0;
    };
    uint32_t nh = 0;
    std::vector<uint32_t> order;           // n
    std::vector<uint64_t> bin_first;       // nh + 4
    std::vector<onc_msg> calls, replies;   // n each
    size_t n_served = 0, n_rejected = 0, n_other = 0;

    Span bin(uint32_t b) const {
        const size_t lo = size_t(bin_first[b]);
        return Span{calls.data() + lo, replies.data() + lo, order.data() + lo, size_t(bin_first[b + 1]) - lo};
    }
    Span handler(uint32_t h) const {
        if (h >= nh) throw CodecError("RoutedCalls: no such handler");
        return bin(h);
    }
    Span rejected() const { return bin(ONC_ROUTE_BIN_REJECTED(nh)); }
    Span not_calls() const { return bin(ONC_ROUTE_BIN_NOT_CALL(nh)); }
    Span failed() const { return bin(ONC_ROUTE_BIN_FAILED(nh)); }

    // The rejected Calls' replies (PROG_UNAVAIL, PROG_MISMATCH{low, high},
    // PROC_UNAVAIL with an AUTH_NONE verifier), serialised back to back and
    // appended to `out` through BatchEncoder; rec_off as serialise_into's.
    std::vector<int32_t> reject_replies(Codec& codec, std::vector<uint8_t>& out,
                                        std::vector<uint64_t>* rec_off = nullptr) const {
        const Span r = rejected();
        BatchEncoder enc;
        for (size_t k = 0; k < r.n; ++k) {
            const onc_msg& d = r.replies[k];
            AcceptedStatus s = d.stat == ONC_ACCEPT_PROG_MISMATCH
                                   ? AcceptedStatus::program_mismatch(d.u.mismatch.low, d.u.mismatch.high)
                                   : AcceptedStatus::of(d.stat == ONC_ACCEPT_PROG_UNAVAIL
                                                            ? AcceptedStatus::Kind::ProgramUnavailable
                                                            : AcceptedStatus::Kind::ProcedureUnavailable);
            enc.push(RpcMessage(d.xid, MessageType::reply(ReplyBody::accepted(AcceptedReply(AuthFlavor::none(), std::move(s))))));
        }
        if (!r.n) {
            if (rec_off) rec_off->assign(1, 0);
            return {};
        }
        return enc.serialise_into(codec, out, rec_off);
    }
};

// onc_route_calls over a BatchDecoder result: every record classified against
// the table on the device and grouped by handler. Inputs and outputs go through
// the codec's stage; one synchronisation.
inline RoutedCalls route_calls(Codec& codec, const std::vector<Decoded>& results, const RouteTable& table) {
    using detail::need;
    const std::vector<onc_route> t = table.sorted();
    const size_t n = results.size(), ntab = t.size();
    const uint32_t nh = table.n_handlers();
    if (n >= (uint64_t(1) << 32)) throw CodecError("route_calls: too many records");
    detail::Carve c{codec.stage(3 * need<onc_msg>(n) + need<int32_t>(n) + need<onc_route>(ntab) + 2 * need<uint32_t>(n) +
                                need<uint64_t>(nh + 4) + need<uint64_t>(4))};
    const auto dm = c.take<onc_msg>(n);
    const auto st = c.take<int32_t>(n);
    const auto tb = c.take<onc_route>(ntab);
    const auto route = c.take<uint32_t>(n);
    const auto order = c.take<uint32_t>(n);
    const auto first = c.take<uint64_t>(nh + 4);
    const auto co = c.take<onc_msg>(n);
    const auto rp = c.take<onc_msg>(n);
    const auto res = c.take<uint64_t>(4);
    for (size_t r = 0; r < n; ++r) {
        onc_msg& d = dm.host[r];
        std::memset(&d, 0, sizeof(d));
        st.host[r] = results[r].status;
        if (!results[r].ok()) continue;
        const RpcMessage& m = *results[r].message;
        d.xid = m.xid();
        if (const CallBody* cb = m.call_body()) {
            d.msg_type = ONC_MSG_CALL;
            d.u.call.program = cb->program();
            d.u.call.program_version = cb->program_version();
            d.u.call.procedure = cb->procedure();
        } else {
            d.msg_type = ONC_MSG_REPLY;
        }
    }
    if (ntab) std::memcpy(tb.host, t.data(), sizeof(onc_route) * ntab);
    codec.check(onc_route_calls(codec.get(), dm.dev, st.dev, n, ntab ? tb.dev : nullptr, uint32_t(ntab), nh, route.dev,
                                order.dev, first.dev, co.dev, rp.dev, res.dev),
                "onc_route_calls");
    codec.sync();
    if (res.host[3] != 0) throw CodecError("route_calls: the device refused the table");
    RoutedCalls out;
    out.nh = nh;
    out.order.assign(order.host, order.host + n);
    out.bin_first.assign(first.host, first.host + nh + 4);
    out.calls.assign(co.host, co.host + n);
    out.replies.assign(rp.host, rp.host + n);
    out.n_served = size_t(res.host[0]);
    out.n_rejected = size_t(res.host[1]);
    out.n_other = size_t(res.host[2]);
    return out;
}

// ---------------------------------------------------------------------------
// Call arguments unpacked into columns (onc_xdr_unpack)
// ---------------------------------------------------------------------------
// A flat XDR schema, field by field in wire order: u32() .. array64() append a
// field; select(), when(v) and skip() qualify the field appended last.
//   XdrSchema s;                       // NFSv3 WRITE3args
//   s.opaque(64).u64().u32().u32().opaque(0xFFFFFFFFu);
//   s.boolean().select().u32().when(1);    // an optional: set_it, then the value
// layout(n) places the columns of n records itself, back to back and 8-byte
// aligned, and checks the schema on the host (onc_xdr_schema_check): the
// device never sees a bad one.
class XdrSchema {
public:
    XdrSchema& u32() { return add(ONC_XDR_U32, 0); }
    XdrSchema& u64() { return add(ONC_XDR_U64, 0); }
    XdrSchema& boolean() { return add(ONC_XDR_BOOL, 0); }
    XdrSchema& opaque_fixed(uint32_t n) { return add(ONC_XDR_OPAQUE_FIXED, n); }
    XdrSchema& opaque(uint32_t max) { return add(ONC_XDR_OPAQUE_VAR, max); }
    XdrSchema& array32(uint32_t max) { return add(ONC_XDR_ARRAY32, max); }
    XdrSchema& array64(uint32_t max) { return add(ONC_XDR_ARRAY64, max); }
    // the field's value becomes the selector of the fields that follow
    XdrSchema& select() { return flag(ONC_XDR_SELECT); }
    // the field is on the wire only if the selector is v
    XdrSchema& when(uint32_t v) {
        flag(ONC_XDR_IF);
        fields_.back().cond_val = v;
        return *this;
    }
    // parsed and checked, no column
    XdrSchema& skip() { return flag(ONC_XDR_NO_COLUMN); }
    size_t size() const { return fields_.size(); }
    static uint32_t width(uint32_t type_flags) {
        const uint32_t t = type_flags & 0xFFu;
        return (t == ONC_XDR_U32 || t == ONC_XDR_BOOL || t == ONC_XDR_OPAQUE_FIXED) ? 4u : 8u;
    }
    std::vector<onc_xdr_field> layout(size_t n, uint64_t* cols_cap) const {
        std::vector<onc_xdr_field> f = fields_;
        uint64_t off = 0;
        for (onc_xdr_field& e : f) {
            if (e.type_flags & ONC_XDR_NO_COLUMN) continue;
            e.col_off = off;
            off += (uint64_t(width(e.type_flags)) * n + 7) & ~uint64_t(7);
        }
        const int bad = onc_xdr_schema_check(f.data(), uint32_t(f.size()), n, off);
        if (bad != 0) throw CodecError("XdrSchema: field " + std::to_string(bad - 1) + " breaks a schema rule");
        *cols_cap = off;
        return f;
    }

private:
    XdrSchema& add(uint32_t type, uint32_t arg) {
        if (fields_.size() == ONC_XDR_FIELDS_MAX) throw CodecError("XdrSchema: too many fields");
        fields_.push_back(onc_xdr_field{type, arg, 0, 0, 0});
        return *this;
    }
    XdrSchema& flag(uint32_t f) {
        if (fields_.empty()) throw CodecError("XdrSchema: no field to qualify");
        fields_.back().type_flags |= f;
        return *this;
    }
    std::vector<onc_xdr_field> fields_;
};

// What unpack_args returns: one column per field over the n records of the
// slice, a parse status per record, and the reply descriptors with
// GARBAGE_ARGS set for the Calls whose arguments do not parse. Positions count
// from each payload's first byte; bytes(f, r) is the body they point at, in the
// caller's wire.
struct UnpackedArgs {
    size_t n = 0;
    std::vector<onc_xdr_field> fields;
    std::vector<uint8_t> cols;
    std::vector<uint32_t> xstat, rest_pos, rest_len;
    std::vector<uint64_t> present;
    std::vector<onc_msg> replies;              // n: the slice's skeletons, patched
    std::vector<Bytes> payloads;               // n: where each record's arguments lie
    size_t n_ok = 0, n_garbage = 0, n_other = 0;

    uint32_t code(size_t r) const { return xstat[r] & 0xFFu; }
    uint32_t failed_field(size_t r) const { return xstat[r] >> 8; }
    bool ok(size_t r) const { return code(r) == ONC_XDR_OK; }
    bool has(size_t f, size_t r) const { return (present[r] >> f) & 1u; }
    // the column of a U32 / BOOL field (uint32_t), of a U64 field (uint64_t),
    // or the positions of an opaque or array field (uint32_t; lengths(f): the
    // lengths or counts)
    template <class T>
    const T* column(size_t f) const {
        const onc_xdr_field& e = field(f);
        const bool wide = (e.type_flags & 0xFFu) == ONC_XDR_U64;
        if (wide != (sizeof(T) == 8) || (sizeof(T) != 4 && sizeof(T) != 8)) throw CodecError("UnpackedArgs: column type");
        return reinterpret_cast<const T*>(cols.data() + e.col_off);
    }
    const uint32_t* lengths(size_t f) const {
        if ((field(f).type_flags & 0xFFu) < ONC_XDR_OPAQUE_VAR) throw CodecError("UnpackedArgs: the field has no lengths");
        return column<uint32_t>(f) + n;
    }
    // the body of an opaque or array field of record r (empty when the field is absent or the record failed)
    Bytes bytes(size_t f, size_t r) const {
        const onc_xdr_field& e = field(f);
        const uint32_t t = e.type_flags & 0xFFu;
        if (t < ONC_XDR_OPAQUE_FIXED) throw CodecError("UnpackedArgs: the field has no body");
        if (!has(f, r)) return Bytes();
        const uint32_t pos = column<uint32_t>(f)[r];
        const uint64_t len = t == ONC_XDR_OPAQUE_FIXED ? e.arg
                                                       : uint64_t(lengths(f)[r]) * (t == ONC_XDR_ARRAY32 ? 4u : (t == ONC_XDR_ARRAY64 ? 8u : 1u));
        return Bytes(payloads[r].ptr + pos, size_t(len));
    }

private:
    const onc_xdr_field& field(size_t f) const {
        if (f >= fields.size() || (fields[f].type_flags & ONC_XDR_NO_COLUMN)) throw CodecError("UnpackedArgs: no such column");
        return fields[f];
    }
};

namespace detail {

// onc_xdr_unpack of n payloads inside `wire` (payload-relative positions),
// inputs and outputs through the codec's stage; one synchronisation.
inline UnpackedArgs unpack_payloads(Codec& codec, const uint8_t* wire, size_t wire_len, const std::vector<Bytes>& payloads,
                                    const std::vector<int32_t>& status, const onc_msg* skeletons, const XdrSchema& schema,
                                    uint32_t flags) {
    const size_t n = payloads.size();
    UnpackedArgs out;
    out.n = n;
    out.payloads = payloads;
    uint64_t cap = 0;
    out.fields = schema.layout(n, &cap);
    Carve c{codec.stage(need<uint8_t>(wire_len) + 2 * need<onc_msg>(n) + need<int32_t>(n) + need<uint8_t>(size_t(cap)) +
                        3 * need<uint32_t>(n) + need<uint64_t>(n) + need<uint64_t>(4))};
    const auto w = c.take<uint8_t>(wire_len);
    const auto dm = c.take<onc_msg>(n);
    const auto st = c.take<int32_t>(n);
    const auto cols = c.take<uint8_t>(size_t(cap));
    const auto xs = c.take<uint32_t>(n);
    const auto pr = c.take<uint64_t>(n);
    const auto rp = c.take<uint32_t>(n);
    const auto rl = c.take<uint32_t>(n);
    const auto rep = c.take<onc_msg>(n);
    const auto res = c.take<uint64_t>(4);
    if (wire_len) std::memcpy(w.host, wire, wire_len);
    for (size_t r = 0; r < n; ++r) {
        onc_msg& d = dm.host[r];
        std::memset(&d, 0, sizeof(d));
        st.host[r] = status[r];
        if (status[r] != ONC_OK) continue;
        const Bytes& p = payloads[r];
        if (p.len && (p.ptr < wire || p.ptr + p.len > wire + wire_len)) throw CodecError("unpack_args: a payload outside the wire");
        d.msg_type = ONC_MSG_CALL;
        d.payload_len = uint32_t(p.len);
        d.payload_off = p.len ? uint64_t(p.ptr - wire) : 0;
    }
    if (n && skeletons) std::memcpy(rep.host, skeletons, sizeof(onc_msg) * n);
    else if (n) std::memset(rep.host, 0, sizeof(onc_msg) * n);
    codec.check(onc_xdr_unpack(codec.get(), w.dev, wire_len, dm.dev, st.dev, n, nullptr, 0, out.fields.data(),
                               uint32_t(out.fields.size()), flags, cols.dev, cap, xs.dev, pr.dev, rp.dev, rl.dev, rep.dev,
                               res.dev),
                "onc_xdr_unpack");
    codec.sync();
    out.cols.assign(cols.host, cols.host + cap);
    out.xstat.assign(xs.host, xs.host + n);
    out.present.assign(pr.host, pr.host + n);
    out.rest_pos.assign(rp.host, rp.host + n);
    out.rest_len.assign(rl.host, rl.host + n);
    out.replies.assign(rep.host, rep.host + n);
    out.n_ok = size_t(res.host[0]);
    out.n_garbage = size_t(res.host[1]);
    out.n_other = size_t(res.host[2]);
    return out;
}

inline Bytes args_of(const Decoded& d, int32_t* status) {
    *status = d.status;
    if (!d.ok()) return Bytes();
    if (const CallBody* cb = d.message->call_body()) return cb->payload();
    *status = ONC_ERR_INVALID_MESSAGE_TYPE;     // (not a Call: skipped, as a failed record is)
    return Bytes();
}

}  // namespace detail

// The arguments of one handler's Calls (a span of route_calls' result) parsed
// against the schema on the device. `results` and `wire` are what the span's
// indices and the decoded payloads point into. The span's reply skeletons come
// back with GARBAGE_ARGS (RFC 5531 §9) set where the arguments do not parse.
inline UnpackedArgs unpack_args(Codec& codec, const uint8_t* wire, size_t wire_len, const std::vector<Decoded>& results,
                                const RoutedCalls::Span& calls, const XdrSchema& schema, uint32_t flags = 0) {
    std::vector<Bytes> payloads(calls.n);
    std::vector<int32_t> status(calls.n);
    for (size_t k = 0; k < calls.n; ++k) payloads[k] = detail::args_of(results[calls.index[k]], &status[k]);
    return detail::unpack_payloads(codec, wire, wire_len, payloads, status, calls.replies, schema, flags);
}

// ... of every record of a decoded list (records that are no Calls, and failed
// ones, are skipped); the replies are Success skeletons with the Calls' xids.
inline UnpackedArgs unpack_args(Codec& codec, const uint8_t* wire, size_t wire_len, const std::vector<Decoded>& results,
                                const XdrSchema& schema, uint32_t flags = 0) {
    const size_t n = results.size();
    std::vector<Bytes> payloads(n);
    std::vector<int32_t> status(n);
    std::vector<onc_msg> skel(n);
    for (size_t r = 0; r < n; ++r) {
        payloads[r] = detail::args_of(results[r], &status[r]);
        std::memset(&skel[r], 0, sizeof(onc_msg));
        if (status[r] != ONC_OK) continue;
        skel[r].xid = results[r].message->xid();
        skel[r].msg_type = ONC_MSG_REPLY;
    }
    return detail::unpack_payloads(codec, wire, wire_len, payloads, status, skel.data(), schema, flags);
}

// ---------------------------------------------------------------------------
// Replies paired with the Calls they answer (onc_match_replies)
// ---------------------------------------------------------------------------
// A client's Calls that wait for their Replies, in the order they were sent:
// add() one per Call with the connection it went out on and a tag of the
// caller's (a request slot, a send time). The same (conn, xid) may be pending
// more than once: its Replies answer the entries first sent, first matched.
class PendingCalls {
public:
    PendingCalls() = default;
    explicit PendingCalls(std::vector<onc_pending> list) : list_(std::move(list)) {}
    PendingCalls& add(uint32_t conn, uint32_t xid, uint64_t tag = 0) {
        if (list_.size() + 1 >= ONC_MATCH_MAX) throw CodecError("PendingCalls: too many entries");
        list_.push_back(onc_pending{conn, xid, tag});
        return *this;
    }
    const std::vector<onc_pending>& list() const { return list_; }
    size_t size() const { return list_.size(); }
    bool empty() const { return list_.empty(); }

private:
    std::vector<onc_pending> list_;
};

// What match_replies returns. match[r]: the pending entry record r answers, or
// ONC_MATCH_UNKNOWN / _DUPLICATE / _NOT_REPLY / _FAILED; tag[r]: that entry's
// tag (0 for a record that answers none); hit[p]: the record that answers
// entry p, or ONC_MATCH_NONE.
struct MatchedReplies {
    std::vector<uint32_t> match;           // n
    std::vector<uint64_t> tag;             // n
    std::vector<uint32_t> hit;             // np
    size_t n_matched = 0, n_unknown = 0, n_duplicate = 0, n_not_reply = 0, n_failed = 0;

    bool matched(size_t r) const { return match[r] < ONC_MATCH_FAILED; }
    bool answered(size_t p) const { return hit[p] != ONC_MATCH_NONE; }
    // The entries nobody answered, in list order: followed by the Calls sent
    // since, the pending list of the next batch.
    const PendingCalls& still() const { return still_; }

private:
    PendingCalls still_;
    friend MatchedReplies match_replies(Codec&, const std::vector<Decoded>&, const std::vector<uint32_t>&,
                                        const PendingCalls&);
};

// onc_match_replies over a BatchDecoder result: record r arrived on connection
// conns[r] (what try_from_streams' segments say; an empty `conns`: every record
// on connection 0). Inputs and outputs go through the codec's stage; one
// synchronisation.
inline MatchedReplies match_replies(Codec& codec, const std::vector<Decoded>& results,
                                    const std::vector<uint32_t>& conns, const PendingCalls& pending) {
    using detail::need;
    const size_t n = results.size(), np = pending.size();
    if (!conns.empty() && conns.size() != n) throw CodecError("match_replies: a connection per record");
    if (n >= ONC_MATCH_MAX || np >= ONC_MATCH_MAX) throw CodecError("match_replies: too many records");
    detail::Carve c{codec.stage(need<onc_msg>(n) + need<int32_t>(n) + 2 * need<uint32_t>(n) + 2 * need<onc_pending>(np) +
                                need<uint32_t>(np) + need<uint64_t>(n) + need<uint64_t>(6))};
    const auto dm = c.take<onc_msg>(n);
    const auto st = c.take<int32_t>(n);
    const auto rc = c.take<uint32_t>(n);
    const auto pd = c.take<onc_pending>(np);
    const auto sl = c.take<onc_pending>(np);
    const auto mt = c.take<uint32_t>(n);
    const auto ht = c.take<uint32_t>(np);
    const auto tg = c.take<uint64_t>(n);
    const auto res = c.take<uint64_t>(6);
    for (size_t r = 0; r < n; ++r) {
        onc_msg& d = dm.host[r];
        std::memset(&d, 0, sizeof(d));
        st.host[r] = results[r].status;
        rc.host[r] = conns.empty() ? 0u : conns[r];
        if (!results[r].ok()) continue;
        const RpcMessage& m = *results[r].message;
        d.xid = m.xid();
        d.msg_type = m.call_body() ? ONC_MSG_CALL : ONC_MSG_REPLY;
    }
    if (np) std::memcpy(pd.host, pending.list().data(), sizeof(onc_pending) * np);
    codec.check(onc_match_replies(codec.get(), dm.dev, st.dev, conns.empty() ? nullptr : rc.dev, n, pd.dev, np, mt.dev,
                                  ht.dev, tg.dev, sl.dev, res.dev),
                "onc_match_replies");
    codec.sync();
    MatchedReplies out;
    out.match.assign(mt.host, mt.host + n);
    out.tag.assign(tg.host, tg.host + n);
    out.hit.assign(ht.host, ht.host + np);
    out.n_matched = size_t(res.host[0]);
    out.n_unknown = size_t(res.host[1]);
    out.n_duplicate = size_t(res.host[2]);
    out.n_not_reply = size_t(res.host[3]);
    out.n_failed = size_t(res.host[4]);
    out.still_ = PendingCalls(std::vector<onc_pending>(sl.host, sl.host + size_t(res.host[5])));
    return out;
}

// ---------------------------------------------------------------------------
// A send batch grouped by connection (onc_group_by_conn, onc_conn_extents)
// ---------------------------------------------------------------------------
// What group_by_conn returns: the items sorted stably by connection, as
// positions in `order`; connection c's items are order[conn_first[c] ..
// conn_first[c + 1]), in the order they were given, and the items of no
// connection (an id of nconn or more) come last. msgs[j] is the descriptor of
// item order[j] when descriptors were given: msgs[0 .. n_sent) encodes as it
// stands into one contiguous stream per connection.
struct GroupedSends {
    struct Span {
        const uint32_t* index = nullptr;   // n positions in the batch as given
        const onc_msg* msgs = nullptr;     // their descriptors, or nullptr
        size_t n = 0;
    };
    uint32_t nconn = 0;
    std::vector<uint32_t> order;           // n
    std::vector<uint64_t> conn_first;      // nconn + 2
    std::vector<onc_msg> msgs;             // n, or empty
    size_t n_sent = 0, n_dropped = 0, n_active = 0;

    Span group(uint32_t g) const {
        const size_t lo = size_t(conn_first[g]);
        return Span{order.data() + lo, msgs.empty() ? nullptr : msgs.data() + lo, size_t(conn_first[g + 1]) - lo};
    }
    Span of(uint32_t c) const {
        if (c >= nconn) throw CodecError("GroupedSends: no such connection");
        return group(c);
    }
    Span dropped() const { return group(nconn); }
    size_t active() const { return n_active; }     // connections with an item

    // onc_conn_extents: connection c's bytes of the stream that msgs[0 ..
    // nrec) encoded to with the offsets rec_off (nrec + 1 of them: the whole
    // batch, or only its first n_sent records) are [first, second) of entry
    // c; entry nconn is the dropped group's range (empty when those were not
    // encoded).
    std::vector<std::pair<uint64_t, uint64_t>> connection_streams(Codec& codec, const std::vector<uint64_t>& rec_off) const {
        using detail::need;
        if (rec_off.empty()) throw CodecError("connection_streams: rec_off holds nrec + 1 offsets");
        const size_t ne = size_t(nconn) + 2;
        detail::Carve c{codec.stage(need<uint64_t>(rec_off.size()) + 2 * need<uint64_t>(ne))};
        const auto ro = c.take<uint64_t>(rec_off.size());
        const auto cf = c.take<uint64_t>(ne);
        const auto co = c.take<uint64_t>(ne);
        std::memcpy(ro.host, rec_off.data(), 8 * rec_off.size());
        std::memcpy(cf.host, conn_first.data(), 8 * ne);
        codec.check(onc_conn_extents(codec.get(), ro.dev, rec_off.size() - 1, cf.dev, nconn, co.dev), "onc_conn_extents");
        codec.sync();
        std::vector<std::pair<uint64_t, uint64_t>> out(size_t(nconn) + 1);
        for (size_t g = 0; g <= nconn; ++g) out[g] = {co.host[g], co.host[g + 1]};
        return out;
    }
};

// onc_group_by_conn: item k goes out on connection conn_of[via[k]] (an empty
// `via`: conn_of[k]); an id of nconn or more, or an index outside conn_of,
// marks an item that is not sent. `msgs`, when given, holds a descriptor per
// item and comes back in connection order. Inputs and outputs go through the
// codec's stage; one synchronisation.
inline GroupedSends group_by_conn(Codec& codec, const std::vector<uint32_t>& conn_of, const std::vector<uint32_t>& via,
                                  uint32_t nconn, const std::vector<onc_msg>& msgs = {}) {
    using detail::need;
    const size_t nsrc = conn_of.size(), n = via.empty() ? nsrc : via.size();
    if (nconn > ONC_GROUP_CONN_MAX) throw CodecError("group_by_conn: too many connections");
    if (n >= (uint64_t(1) << 32)) throw CodecError("group_by_conn: too many items");
    if (!msgs.empty() && msgs.size() != n) throw CodecError("group_by_conn: a descriptor per item");
    const size_t nm = msgs.size(), ne = size_t(nconn) + 2;
    detail::Carve c{codec.stage(need<uint32_t>(nsrc) + 2 * need<uint32_t>(n) + need<uint64_t>(ne) + 2 * need<onc_msg>(nm) +
                                need<uint64_t>(3))};
    const auto rc = c.take<uint32_t>(nsrc);
    const auto vi = c.take<uint32_t>(via.size());
    const auto od = c.take<uint32_t>(n);
    const auto cf = c.take<uint64_t>(ne);
    const auto mi = c.take<onc_msg>(nm);
    const auto mo = c.take<onc_msg>(nm);
    const auto res = c.take<uint64_t>(3);
    if (nsrc) std::memcpy(rc.host, conn_of.data(), 4 * nsrc);
    if (!via.empty()) std::memcpy(vi.host, via.data(), 4 * via.size());
    if (nm) std::memcpy(mi.host, msgs.data(), sizeof(onc_msg) * nm);
    codec.check(onc_group_by_conn(codec.get(), rc.dev, nsrc, via.empty() ? nullptr : vi.dev, n, nconn, od.dev, cf.dev,
                                  nm ? mi.dev : nullptr, nm ? mo.dev : nullptr, res.dev),
                "onc_group_by_conn");
    codec.sync();
    GroupedSends out;
    out.nconn = nconn;
    out.order.assign(od.host, od.host + n);
    out.conn_first.assign(cf.host, cf.host + ne);
    if (nm) out.msgs.assign(mo.host, mo.host + nm);
    out.n_sent = size_t(res.host[0]);
    out.n_dropped = size_t(res.host[1]);
    out.n_active = size_t(res.host[2]);
    return out;
}

inline FragmentedHeads BatchDecoder::try_from_fragmented_heads(Codec& codec, const uint8_t* wire, size_t wire_len,
                                                               const std::vector<Segment>& segments, DecodeMode mode,
                                                               uint32_t head_len) {
    using detail::need;
    constexpr uint32_t kFull = (ONC_HEAD_SPAN_MAX + 15u) & ~15u;    // 736: every header fits
    FragmentedHeads f;
    f.wire = wire;
    for (;;) {
        f.heads = reassemble_heads(codec, wire, wire_len, segments, head_len, &f.segments);
        const size_t n = f.heads.n();
        f.results.clear();
        f.payload_pos.assign(n, 0);
        f.payload_len.assign(n, 0);
        if (!n) return f;
        detail::Carve c{codec.stage(need<uint8_t>(n * head_len) + need<uint32_t>(n) + out_bytes(n))};
        const auto h = c.take<uint8_t>(n * head_len);
        std::memcpy(h.host, f.heads.heads.data(), n * head_len);
        const auto l = c.take<uint32_t>(n);
        std::memcpy(l.host, f.heads.rec_len.data(), n * 4);
        const Out o = take_out(c, n);
        const onc_decoded d = o.dev();
        codec.check(onc_decode_heads(codec.get(), h.dev, head_len, l.dev, n, int(mode), &d), "onc_decode_heads");
        codec.sync();
        bool head_short = false;
        for (size_t i = 0; i < n; ++i)
            head_short = head_short || (o.status.host[i] == ONC_DEC_BAD_EXTENT && o.aux0.host[i] == ONC_EXTENT_HEAD_SHORT);
        if (head_short && head_len < kFull) {
            head_len = kFull;
            f.retried = true;
            continue;
        }
        f.descriptors.assign(o.msgs.host, o.msgs.host + n);
        f.status.assign(o.status.host, o.status.host + n);
        // the messages' own payload views end with the head
        for (size_t i = 0; i < n; ++i) {
            if (o.status.host[i] != ONC_OK) continue;
            onc_msg& m = o.msgs.host[i];
            const bool pay = m.msg_type == ONC_MSG_CALL ||
                             (m.reply_stat == ONC_REPLY_ACCEPTED && m.stat == ONC_ACCEPT_SUCCESS);
            if (!pay) continue;
            const uint64_t pos = m.payload_off - uint64_t(i) * head_len;
            f.payload_pos[i] = pos;
            f.payload_len[i] = m.payload_len;
            const uint64_t present = std::min<uint64_t>(f.heads.rec_len[i], head_len);
            m.payload_len = uint32_t(std::min<uint64_t>(m.payload_len, present > pos ? present - pos : 0));
        }
        f.results = results(o, n, f.heads.heads.data());
        return f;
    }
}

inline MixedStreams BatchDecoder::try_from_mixed_streams(Codec& codec, const uint8_t* wire, size_t wire_len,
                                                         const std::vector<Segment>& segments, DecodeMode mode) {
    MixedStreams m;
    const size_t nseg = segments.size();
    m.per_connection.resize(nseg);
    std::vector<Decoded> plain = try_from_streams(codec, wire, wire_len, segments, &m.segments, mode);
    std::vector<Segment> rests;      // of the segments that stopped at a fragmented mark
    std::vector<size_t> whose;
    for (size_t i = 0; i < nseg; ++i) {
        SegmentResult& g = m.segments[i];
        auto from = plain.begin() + std::ptrdiff_t(g.first);
        m.per_connection[i].assign(std::make_move_iterator(from), std::make_move_iterator(from + std::ptrdiff_t(g.n)));
        if (g.status == ONC_ERR_FRAGMENTED) {
            rests.push_back(Segment{segments[i].off + g.consumed, segments[i].len - g.consumed});
            whose.push_back(i);
        }
    }
    if (rests.empty()) return m;
    std::vector<SegmentRecords> per;
    ReassembledStreams r = reassemble_streams(codec, wire, wire_len, rests, &per);
    m.reassembled = std::move(r.bytes);          // the views below point into it
    const size_t n = r.rec_off.size() - 1;
    std::vector<uint32_t> rec_len(n);
    for (size_t k = 0; k < n; ++k) rec_len[k] = uint32_t(r.rec_off[k + 1] - r.rec_off[k]);
    std::vector<Decoded> rebuilt = try_from(codec, m.reassembled.data(), m.reassembled.size(), rec_len, mode);
    for (size_t j = 0; j < rests.size(); ++j) {
        SegmentResult& g = m.segments[whose[j]];
        std::vector<Decoded>& list = m.per_connection[whose[j]];
        auto from = rebuilt.begin() + std::ptrdiff_t(per[j].first_rec);
        list.insert(list.end(), std::make_move_iterator(from),
                    std::make_move_iterator(from + std::ptrdiff_t(per[j].n_rec)));
        g.n = list.size();
        g.consumed += per[j].consumed;
        g.status = per[j].status;
        g.aux0 = per[j].aux0;
        g.aux1 = per[j].aux1;
    }
    return m;
}

// The send side: a packed stream of single-fragment records (what
// BatchEncoder::serialise_into writes) cut on the device into fragments of at
// most max_frag body bytes (onc_frame_stream + onc_fragment), as a sender
// flushing a bounded buffer or a peer that caps the fragment size needs them.
// reassemble_stream of `bytes` gives the input back.
struct Fragmented {
    std::vector<uint8_t> bytes;      // the fragmented stream (out_off.back() bytes)
    std::vector<uint64_t> out_off;   // n + 1 offsets into bytes: where record i's fragments start
    std::vector<int32_t> status;     // per record: ONC_OK
    size_t n_frags = 0;              // fragments written
    size_t n_multi = 0;              // records cut into more than one fragment
    std::optional<Error> stop;       // why framing stopped before the buffer's end, if it did
};

inline Fragmented fragment_stream(Codec& codec, const uint8_t* stream, size_t len, uint32_t max_frag) {
    using detail::need;
    if (max_frag < 1 || max_frag > 0x7FFFFFFFu) throw CodecError("fragment_stream: max_frag outside 1 .. 0x7FFFFFFF");
    Fragmented r;
    r.out_off.assign(1, 0);
    const size_t max_records = len / 4 + 1;
    detail::Carve c{codec.stage(need<uint8_t>(len) + need<uint64_t>(max_records + 1) + need<uint64_t>(5))};
    const auto w = c.take<uint8_t>(len);
    if (len) std::memcpy(w.host, stream, len);
    const size_t rec_at = c.off;
    const auto rec = c.take<uint64_t>(max_records + 1);
    const auto fres = c.take<uint64_t>(5);
    codec.check(onc_frame_stream(codec.get(), w.dev, len, rec.dev, max_records, fres.dev), "onc_frame_stream");
    codec.sync();
    uint64_t f[5];
    std::memcpy(f, fres.host, sizeof(f));
    if (int32_t(f[2]) != ONC_OK) r.stop = Error(int32_t(f[2]), uint32_t(f[3]), uint32_t(f[4]));
    const size_t n = size_t(f[0]);
    if (!n) return r;
    // every record is at least its mark: a mark more per further fragment
    size_t cap = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t body = rec.host[i + 1] - rec.host[i] - 4;
        const uint64_t k = body / max_frag + (body % max_frag ? 1 : 0);
        cap += size_t(body + 4 * (k ? k : 1));
    }
    // the outputs after what is staged (a stage that grows keeps it)
    const size_t mark = c.off;
    c.s = codec.stage(mark + need<uint8_t>(cap) + need<uint64_t>(n + 1) + need<int32_t>(n) + need<uint64_t>(3), mark);
    const auto out = c.take<uint8_t>(cap);
    const auto off = c.take<uint64_t>(n + 1);
    const auto st = c.take<int32_t>(n);
    const auto res = c.take<uint64_t>(3);
    codec.check(onc_fragment(codec.get(), c.s.dev, reinterpret_cast<const uint64_t*>(c.s.dev + rec_at), n, max_frag,
                             out.dev, cap, off.dev, st.dev, res.dev),
                "onc_fragment");
    codec.sync();
    uint64_t d[3];
    std::memcpy(d, res.host, sizeof(d));
    r.bytes.assign(out.host, out.host + std::min<uint64_t>(d[1], cap));
    r.out_off.assign(off.host, off.host + n + 1);
    r.status.assign(st.host, st.host + n);
    r.n_frags = size_t(d[0]);
    r.n_multi = size_t(d[2]);
    return r;
}

// ----------------------------------------------------------------------------
// RpcMessage single-message forms (batches of one)
// ----------------------------------------------------------------------------
inline uint32_t RpcMessage::serialised_len(Codec& codec) const {
    BatchEncoder e;
    e.push(*this);
    std::vector<int32_t> st;
    const uint32_t n = e.serialised_lens(codec, &st)[0];
    raise_encode_status(st[0]);
    return n;
}

inline void RpcMessage::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const {
    BatchEncoder e;
    e.push(*this);
    raise_encode_status(e.serialise_into(codec, buf)[0]);
}

inline std::vector<uint8_t> RpcMessage::serialise(Codec& codec) const {
    std::vector<uint8_t> v;
    serialise_into(codec, v);
    return v;
}

inline RpcMessage RpcMessage::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    BatchDecoder d;
    std::vector<Decoded> r = d.try_from(codec, buf.ptr, buf.len, {uint32_t(buf.len)}, mode);
    if (!r[0].ok()) throw r[0].error();
    return std::move(*r[0].message);
}

// ----------------------------------------------------------------------------
// Body-level types (ONC_ROOT_*): TryFrom / serialise_into / serialised_len of
// one type of the message tree, on the GPU (onc_decode_body /
// onc_encode_body, batches of one like RpcMessage's single forms).
// ----------------------------------------------------------------------------
namespace detail {

// One record decoded as `root`; throws the reference's Error on failure.
struct BodyView {
    onc_msg d{};
    onc_unix_params unix[2]{};
};

inline BodyView decode_root(Codec& codec, int root, Bytes buf, DecodeMode mode, uint32_t param) {
    Carve c{codec.stage(need<uint8_t>(buf.len) + need<uint64_t>(2) + need<uint32_t>(1) + need<onc_msg>(1) +
                        need<onc_unix_params>(2) + 3 * need<uint32_t>(1))};
    const auto w = c.take<uint8_t>(buf.len);
    const auto o = c.take<uint64_t>(2);
    const auto p = c.take<uint32_t>(1);
    const auto m = c.take<onc_msg>(1);
    const auto u = c.take<onc_unix_params>(2);
    const auto s = c.take<int32_t>(1);
    const auto a0 = c.take<uint32_t>(1);
    const auto a1 = c.take<uint32_t>(1);
    if (buf.len) std::memcpy(w.host, buf.ptr, buf.len);
    o.host[0] = 0;
    o.host[1] = buf.len;
    p.host[0] = param;
    onc_decoded out{m.dev, u.dev, s.dev, a0.dev, a1.dev};
    codec.check(onc_decode_body(codec.get(), root, w.dev, o.dev, 1, int(mode), p.dev, &out, nullptr), "onc_decode_body");
    codec.sync();
    if (s.host[0] != ONC_OK) throw Error(s.host[0], a0.host[0], a1.host[0]);
    BodyView v;
    v.d = m.host[0];
    std::memcpy(v.unix, u.host, sizeof(v.unix));
    return v;
}

inline AcceptedStatus status_view(const onc_msg& d, const uint8_t* wire) {
    if (d.stat == ONC_ACCEPT_SUCCESS) return AcceptedStatus::success(Bytes(wire + d.payload_off, d.payload_len));
    if (d.stat == ONC_ACCEPT_PROG_MISMATCH) return AcceptedStatus::program_mismatch(d.u.mismatch.low, d.u.mismatch.high);
    return AcceptedStatus::of(AcceptedStatus::Kind(d.stat));
}

inline RejectedReply rejected_view(const onc_msg& d) {
    return d.stat == ONC_REJECT_RPC_MISMATCH ? RejectedReply::rpc_version_mismatch(d.u.mismatch.low, d.u.mismatch.high)
                                             : RejectedReply::auth_error(AuthError(d.auth_stat));
}

// serialised_len / serialise_into of one value pushed into a BatchEncoder.
template <class T>
inline uint32_t root_len(Codec& codec, const T& v) {
    BatchEncoder e;
    e.push(v);
    std::vector<int32_t> st;
    const uint32_t n = e.serialised_lens(codec, &st)[0];
    RpcMessage::raise_encode_status(st[0]);
    return n;
}

template <class T>
inline void root_into(Codec& codec, const T& v, std::vector<uint8_t>& buf) {
    BatchEncoder e;
    e.push(v);
    RpcMessage::raise_encode_status(e.serialise_into(codec, buf)[0]);
}

}  // namespace detail

inline MessageType MessageType::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    const detail::BodyView v = detail::decode_root(codec, ONC_ROOT_MESSAGE_TYPE, buf, mode, 0);
    return detail::message_view(v.d, v.unix, buf.ptr).message();
}
inline void MessageType::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t MessageType::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

inline CallBody CallBody::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    const detail::BodyView v = detail::decode_root(codec, ONC_ROOT_CALL_BODY, buf, mode, 0);
    return *detail::message_view(v.d, v.unix, buf.ptr).call_body();
}
inline void CallBody::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t CallBody::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

inline ReplyBody ReplyBody::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    const detail::BodyView v = detail::decode_root(codec, ONC_ROOT_REPLY_BODY, buf, mode, 0);
    return *detail::message_view(v.d, v.unix, buf.ptr).reply_body();
}
inline void ReplyBody::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t ReplyBody::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

inline AcceptedReply AcceptedReply::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    const detail::BodyView v = detail::decode_root(codec, ONC_ROOT_ACCEPTED_REPLY, buf, mode, 0);
    return AcceptedReply(detail::auth_view(v.d.verf, v.unix, buf.ptr), detail::status_view(v.d, buf.ptr));
}
inline void AcceptedReply::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t AcceptedReply::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

inline AcceptedStatus AcceptedStatus::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    const detail::BodyView v = detail::decode_root(codec, ONC_ROOT_ACCEPTED_STATUS, buf, mode, 0);
    return detail::status_view(v.d, buf.ptr);
}
inline void AcceptedStatus::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t AcceptedStatus::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

inline RejectedReply RejectedReply::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    return detail::rejected_view(detail::decode_root(codec, ONC_ROOT_REJECTED_REPLY, buf, mode, 0).d);
}
inline void RejectedReply::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t RejectedReply::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

inline AuthError auth_error_try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    return AuthError(detail::decode_root(codec, ONC_ROOT_AUTH_ERROR, buf, mode, 0).d.auth_stat);
}
inline void serialise_into(Codec& codec, AuthError e, std::vector<uint8_t>& buf) { detail::root_into(codec, e, buf); }

inline AuthFlavor AuthFlavor::try_from(Codec& codec, Bytes buf, DecodeMode mode) {
    const detail::BodyView v = detail::decode_root(codec, ONC_ROOT_AUTH_FLAVOR, buf, mode, 0);
    return detail::auth_view(v.d.cred, v.unix, buf.ptr);
}
inline void AuthFlavor::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t AuthFlavor::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

inline AuthUnixParams AuthUnixParams::from_cursor(Codec& codec, Bytes buf, uint32_t expected_len) {
    const detail::BodyView v =
        detail::decode_root(codec, ONC_ROOT_AUTH_UNIX_PARAMS, buf, DecodeMode::Slice, expected_len);
    return detail::auth_view(v.d.cred, v.unix, buf.ptr).unix_params();
}
inline AuthUnixParams AuthUnixParams::try_from(Codec& codec, Bytes buf) {
    const detail::BodyView v = detail::decode_root(codec, ONC_ROOT_AUTH_UNIX_PARAMS, buf, DecodeMode::Bytes, 0);
    return detail::auth_view(v.d.cred, v.unix, buf.ptr).unix_params();
}
inline void AuthUnixParams::serialise_into(Codec& codec, std::vector<uint8_t>& buf) const { detail::root_into(codec, *this, buf); }
inline uint32_t AuthUnixParams::serialised_len(Codec& codec) const { return detail::root_len(codec, *this); }

}  // namespace onc_rpc
