"""ctypes binding of the gfx950 codec library (libonc_rpc_amd.so, C ABI in
include/onc_rpc.h) with torch tensors as the device memory.

This is plumbing for tests/bench: all codec work runs in the HIP kernels.
There is no CPU fallback — loading fails loudly when the library is
missing, and every call that returns a non-zero rc raises.
"""
from __future__ import annotations

import ctypes as C
import mmap
import os

import numpy as np

from . import layout as L

_LIB = None
LIB_PATH = os.environ.get("ONC_RPC_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libonc_rpc_amd.so")

K_NAMES = ["enc_len_kernel", "scan_tiles_kernel", "enc_emit_kernel", "decode_kernel",
           "len_tiles_kernel", "len_apply_kernel", "iov_len_kernel", "iov_emit_kernel",
           "frame_chunks_kernel", "frame_write_kernel", "frame_walk_kernel",
           "frame_counts_kernel", "frame_guess_kernel", "compact_kernels",
           "defrag_plan_kernels", "defrag_copy_kernel"]
(K_ENC_LEN, K_SCAN_TILES, K_ENC_EMIT, K_DEC_PARSE, K_LEN_TILES, K_LEN_APPLY, K_IOV_LEN,
 K_IOV_EMIT, K_FRAME, K_FRAME_WRITE, K_FRAME_WALK, K_FRAME_COUNTS, K_FRAME_GUESS, K_COMPACT,
 K_DEFRAG_PLAN, K_DEFRAG_COPY) = range(16)
ABI_VERSION = 8
K_COUNT = len(K_NAMES)

# every symbol include/onc_rpc.h declares
EXPORTED = [
    "onc_abi_version", "onc_codec_create", "onc_codec_destroy", "onc_codec_set_stream",
    "onc_codec_sync", "onc_codec_reserve", "onc_codec_last_error", "onc_status_str",
    "onc_codec_enable_timing", "onc_codec_kernel_stats", "onc_codec_reset_stats",
    "onc_kernel_name", "onc_encode_lengths", "onc_encode", "onc_decode", "onc_scan_lengths",
    "onc_expected_message_len", "onc_encode_iov", "onc_frame_stream", "onc_encode_plan", "onc_encode_emit",
    "onc_decode_lengths", "onc_decode_body", "onc_encode_body", "onc_encode_body_lengths",
    "onc_codec_create_ex", "onc_codec_set_decode_policy", "onc_host_register", "onc_host_unregister",
    "onc_compact", "onc_compact_iov",
    "onc_decode_bounded", "onc_decode_lengths_bounded", "onc_decode_body_bounded",
    "onc_frame_fragments", "onc_defragment",
    "onc_frame_streams", "onc_decode_extents",
    "onc_fragment", "onc_fragment_iov",
    "onc_frame_fragment_streams", "onc_defragment_extents",
    "onc_defragment_heads", "onc_decode_heads",
    "onc_piece_offsets", "onc_gather_pieces",
    "onc_payload_slots", "onc_place_payloads",
    "onc_route_calls",
    "onc_xdr_schema_check", "onc_xdr_unpack",
    "onc_match_replies",
    "onc_group_by_conn", "onc_conn_extents",
]

# onc_codec_options (include/onc_rpc.h)
DECODE_POLICY_AUTO, DECODE_POLICY_STANDARD, DECODE_POLICY_LINE = 0, 1, 2
OPT_FORCE_SCAN = 0x1
VARIANT_EMIT_WS, VARIANT_EMIT_TILE = 0x200, 0x400
VARIANT_WS_NO_INTERIOR, VARIANT_WS_NO_FULL, VARIANT_WS_PIPELINE = 0x4000, 0x8000, 0x10000
VARIANT_EMIT_REPLAN, VARIANT_WHOLE_PLAN = 0x20000, 0x40000
VARIANT_MATCH_ONE_CHAIN = 0x80000
VARIANT_COPY_ONE_GROUP = 0x100000   # the copy kernels in one workgroup: runs of tiles per wave at test sizes
# options every Codec() gets unless it is given its own (bench.py --variant)
DEFAULT_OPTIONS: dict = {}


class OncBatch(C.Structure):
    _fields_ = [("n", C.c_uint64), ("msgs", C.c_void_p), ("unix_params", C.c_void_p),
                ("auth_arena", C.c_void_p), ("payload_arena", C.c_void_p),
                ("unix_count", C.c_uint64), ("auth_len", C.c_uint64), ("payload_len", C.c_uint64)]


class OncCodecOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("decode_policy", C.c_int32), ("variant", C.c_uint32),
                ("enc_chunk", C.c_uint64), ("frame_chunk", C.c_uint64)]


class OncDecoded(C.Structure):
    _fields_ = [("msgs", C.c_void_p), ("unix_params", C.c_void_p), ("status", C.c_void_p),
                ("aux0", C.c_void_p), ("aux1", C.c_void_p)]


class OncGatherSrc(C.Structure):
    """onc_gather_src: the three sources of a piece list, by ONC_PIECE_*."""
    _fields_ = [("base", C.c_void_p * 3), ("len", C.c_uint64 * 3)]


class CodecError(RuntimeError):
    pass


def load_library(path=LIB_PATH):
    """Load libonc_rpc_amd.so (raises if it has not been built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise CodecError(f"HIP codec library missing: {path} (run __graft_entry__.build())")
    lib = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    lib.onc_abi_version.restype = i32
    lib.onc_codec_create.argtypes = [C.POINTER(vp), i32, vp]
    lib.onc_codec_create_ex.argtypes = [C.POINTER(vp), i32, vp, C.POINTER(OncCodecOptions)]
    lib.onc_codec_set_decode_policy.argtypes = [vp, i32]
    lib.onc_codec_destroy.argtypes = [vp]
    lib.onc_codec_set_stream.argtypes = [vp, vp]
    lib.onc_codec_sync.argtypes = [vp]
    lib.onc_codec_reserve.argtypes = [vp, u64]
    lib.onc_codec_last_error.argtypes = [vp]
    lib.onc_codec_last_error.restype = C.c_char_p
    lib.onc_status_str.argtypes = [C.c_int32]
    lib.onc_status_str.restype = C.c_char_p
    lib.onc_codec_enable_timing.argtypes = [vp, i32]
    lib.onc_codec_kernel_stats.argtypes = [vp, vp, vp]
    lib.onc_codec_reset_stats.argtypes = [vp]
    lib.onc_kernel_name.argtypes = [i32]
    lib.onc_kernel_name.restype = C.c_char_p
    lib.onc_encode_lengths.argtypes = [vp, C.POINTER(OncBatch), vp, vp]
    lib.onc_encode.argtypes = [vp, C.POINTER(OncBatch), vp, u64, vp, vp, vp]
    lib.onc_encode_plan.argtypes = [vp, C.POINTER(OncBatch), vp, vp]
    lib.onc_encode_emit.argtypes = [vp, C.POINTER(OncBatch), vp, u64, vp, vp]
    lib.onc_decode.argtypes = [vp, vp, vp, u64, i32, C.POINTER(OncDecoded)]
    lib.onc_decode_lengths.argtypes = [vp, vp, vp, u64, u64, i32, vp, C.POINTER(OncDecoded)]
    lib.onc_scan_lengths.argtypes = [vp, vp, u64, u64, vp]
    lib.onc_frame_stream.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.onc_encode_iov.argtypes = [vp, C.POINTER(OncBatch), vp, u64, vp, vp, vp]
    lib.onc_expected_message_len.argtypes = [C.c_char_p, u64, C.POINTER(C.c_uint32)]
    lib.onc_expected_message_len.restype = C.c_int32
    lib.onc_decode_body.argtypes = [vp, i32, vp, vp, u64, i32, vp, C.POINTER(OncDecoded), vp]
    lib.onc_encode_body.argtypes = [vp, i32, C.POINTER(OncBatch), vp, u64, vp, vp, vp]
    lib.onc_encode_body_lengths.argtypes = [vp, i32, C.POINTER(OncBatch), vp, vp]
    lib.onc_host_register.argtypes = [vp, vp, u64, C.POINTER(vp)]
    lib.onc_host_unregister.argtypes = [vp, vp]
    lib.onc_compact.argtypes = [vp, vp, vp, vp, u64, C.POINTER(C.c_uint64)]
    lib.onc_compact_iov.argtypes = [vp, vp, vp, u64, vp]
    lib.onc_decode_bounded.argtypes = [vp, vp, u64, vp, u64, i32, C.POINTER(OncDecoded)]
    lib.onc_decode_lengths_bounded.argtypes = [vp, vp, u64, vp, u64, u64, i32, vp, C.POINTER(OncDecoded)]
    lib.onc_decode_body_bounded.argtypes = [vp, i32, vp, u64, vp, u64, i32, vp, C.POINTER(OncDecoded), vp]
    lib.onc_frame_fragments.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.onc_defragment.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp]
    lib.onc_frame_streams.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp]
    lib.onc_fragment.argtypes = [vp, vp, vp, u64, C.c_uint32, vp, u64, vp, vp, vp]
    lib.onc_fragment_iov.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, u64, vp, u64, vp, vp, vp, vp]
    lib.onc_decode_extents.argtypes = [vp, vp, u64, vp, vp, u64, i32, C.POINTER(OncDecoded)]
    lib.onc_frame_fragment_streams.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp]
    lib.onc_defragment_extents.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, vp, vp]
    lib.onc_defragment_heads.argtypes = [vp, vp, vp, vp, u64, C.c_uint32, vp, u64, vp, vp, vp, vp, vp]
    lib.onc_decode_heads.argtypes = [vp, vp, C.c_uint32, vp, u64, i32, C.POINTER(OncDecoded)]
    lib.onc_piece_offsets.argtypes = [vp, vp, u64, C.POINTER(OncGatherSrc), vp, vp]
    lib.onc_gather_pieces.argtypes = [vp, vp, vp, u64, C.POINTER(OncGatherSrc), u64, u64, vp]
    lib.onc_payload_slots.argtypes = [vp, vp, vp, u64, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp]
    lib.onc_place_payloads.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, vp, u64]
    lib.onc_route_calls.argtypes = [vp, vp, vp, u64, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.onc_xdr_schema_check.argtypes = [vp, C.c_uint32, u64, u64]
    lib.onc_xdr_unpack.argtypes = [vp, vp, u64, vp, vp, u64, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, u64, vp, vp,
                                   vp, vp, vp, vp]
    lib.onc_match_replies.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp]
    lib.onc_group_by_conn.argtypes = [vp, vp, u64, vp, u64, C.c_uint32, vp, vp, vp, vp, vp]
    lib.onc_conn_extents.argtypes = [vp, vp, u64, vp, C.c_uint32, vp]
    for name in EXPORTED:
        getattr(lib, name).restype = getattr(lib, name).restype or i32
    # a stale library would read a differently laid out onc_batch and label
    # the kernel timings wrongly: refuse it
    abi = lib.onc_abi_version()
    if abi != ABI_VERSION:
        raise CodecError(f"{path}: ABI {abi}, this binding expects {ABI_VERSION} (rebuild: __graft_entry__.build())")
    _LIB = lib
    return lib


def expected_message_len(buf: bytes):
    """expected_message_len (src/rpc_message.rs:343-367) -> (status, length)."""
    lib = load_library()
    out = C.c_uint32(0)
    st = lib.onc_expected_message_len(buf, len(buf), C.byref(out))
    return st, out.value


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _torch():
    import torch
    return torch


def to_device(arr, device):
    """numpy array -> uint8 CUDA tensor holding its bytes."""
    torch = _torch()
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if raw.size == 0:
        raw = np.zeros(16, np.uint8)
    return torch.from_numpy(raw.copy()).to(device)


class DeviceBatch:
    """Descriptor batch resident in HBM (torch uint8 tensors). The arena
    sizes handed to the codec (onc_batch bounds) are the tensors' sizes
    unless given."""

    def __init__(self, n, msgs, unix, auth_arena, payload_arena, unix_count=None, auth_len=None,
                 payload_len=None):
        self.n = n
        self.msgs = msgs
        self.unix = unix
        self.auth_arena = auth_arena
        self.payload_arena = payload_arena
        self.unix_count = unix.numel() // 96 if unix_count is None else unix_count
        self.auth_len = auth_arena.numel() if auth_len is None else auth_len
        self.payload_len = payload_arena.numel() if payload_len is None else payload_len

    @classmethod
    def from_host(cls, hb: L.HostBatch, device="cuda"):
        return cls(hb.n, to_device(hb.msgs, device), to_device(hb.unix, device),
                   to_device(hb.auth_arena, device), to_device(hb.payload_arena, device))

    def c_struct(self):
        return OncBatch(self.n, self.msgs.data_ptr(), self.unix.data_ptr(),
                        self.auth_arena.data_ptr(), self.payload_arena.data_ptr(),
                        self.unix_count, self.auth_len, self.payload_len)


def codec_options(variant=0, force_scan=False, enc_chunk=0, frame_chunk=0, decode_policy=DECODE_POLICY_AUTO):
    """onc_codec_options (include/onc_rpc.h) from keyword arguments."""
    return OncCodecOptions(C.sizeof(OncCodecOptions), OPT_FORCE_SCAN if force_scan else 0, decode_policy, variant,
                           enc_chunk, frame_chunk)


class Codec:
    """One onc_codec handle bound to a device and (by default) torch's
    current stream on that device. `options`: keyword arguments of
    codec_options (default: DEFAULT_OPTIONS)."""

    def __init__(self, device=0, stream=None, **options):
        torch = _torch()
        self.lib = load_library()
        self.device = device
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        self.stream = stream
        h = C.c_void_p()
        opt = codec_options(**(options or DEFAULT_OPTIONS))
        rc = self.lib.onc_codec_create_ex(C.byref(h), device, C.c_void_p(stream), C.byref(opt))
        if rc != 0:
            raise CodecError(f"onc_codec_create_ex rc={rc}")
        self.h = h

    def set_stream(self, stream):
        """Bind the handle to another HIP stream (an int hipStream_t or a torch stream)."""
        self.stream = getattr(stream, "cuda_stream", stream)
        self._check(self.lib.onc_codec_set_stream(self.h, C.c_void_p(self.stream)), "onc_codec_set_stream")

    def set_decode_policy(self, policy):
        self._check(self.lib.onc_codec_set_decode_policy(self.h, policy), "onc_codec_set_decode_policy")

    def close(self):
        if self.h:
            self.lib.onc_codec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            err = self.lib.onc_codec_last_error(self.h).decode()
            raise CodecError(f"{what} rc={rc} {err}")

    def sync(self):
        self._check(self.lib.onc_codec_sync(self.h), "onc_codec_sync")

    def reserve(self, n):
        self._check(self.lib.onc_codec_reserve(self.h, n), "onc_codec_reserve")

    def enable_timing(self, on=True, kernels=None):
        """Bracket launches with HIP events: every kernel (on=True), none
        (on=False), or only the ids in `kernels` (K_* constants)."""
        mask = -1 if on else 0
        if on and kernels is not None:
            mask = 0
            for k in kernels:
                mask |= 1 << k
        self._check(self.lib.onc_codec_enable_timing(self.h, mask), "enable_timing")

    def kernel_stats(self):
        ms = (C.c_double * K_COUNT)()
        cnt = (C.c_uint64 * K_COUNT)()
        self._check(self.lib.onc_codec_kernel_stats(self.h, C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p)),
                    "kernel_stats")
        return {K_NAMES[k]: (ms[k], cnt[k]) for k in range(K_COUNT)}

    def reset_stats(self):
        self._check(self.lib.onc_codec_reset_stats(self.h), "reset_stats")

    # -- encode -----------------------------------------------------------
    def encode_lengths(self, batch: DeviceBatch, rec_len, status):
        b = batch.c_struct()
        self._check(self.lib.onc_encode_lengths(self.h, C.byref(b), _ptr(rec_len), _ptr(status)),
                    "onc_encode_lengths")

    def encode(self, batch: DeviceBatch, out, rec_off, status, rec_len=None, out_cap=None):
        b = batch.c_struct()
        cap = out.numel() if out_cap is None else out_cap
        self._check(self.lib.onc_encode(self.h, C.byref(b), _ptr(out), cap, _ptr(rec_off), _ptr(status),
                                        _ptr(rec_len)), "onc_encode")

    def encode_plan(self, batch: DeviceBatch, status, rec_len=None):
        """Phase 1 of onc_encode (enc_len): lengths, validation, placement totals."""
        b = batch.c_struct()
        self._check(self.lib.onc_encode_plan(self.h, C.byref(b), _ptr(status), _ptr(rec_len)), "onc_encode_plan")

    def encode_emit(self, batch: DeviceBatch, out, rec_off, status, out_cap=None):
        """Phase 2 of onc_encode (enc_emit) of the batch last planned on this handle."""
        b = batch.c_struct()
        cap = out.numel() if out_cap is None else out_cap
        self._check(self.lib.onc_encode_emit(self.h, C.byref(b), _ptr(out), cap, _ptr(rec_off), _ptr(status)),
                    "onc_encode_emit")

    def encode_iov(self, batch: DeviceBatch, hdr_out, iov, status, totals=None, hdr_cap=None):
        """Vectored encode: headers into hdr_out, one onc_iov_rec (32 B) per record in iov."""
        b = batch.c_struct()
        cap = hdr_out.numel() if hdr_cap is None else hdr_cap
        self._check(self.lib.onc_encode_iov(self.h, C.byref(b), _ptr(hdr_out), cap, _ptr(iov), _ptr(status),
                                            _ptr(totals)), "onc_encode_iov")

    def frame_stream(self, wire, length, rec_off, max_records, result):
        """Frame a stream of back-to-back records (device buffers)."""
        self._check(self.lib.onc_frame_stream(self.h, _ptr(wire), length, _ptr(rec_off), max_records,
                                              _ptr(result)), "onc_frame_stream")

    def frame_fragments(self, wire, length, frag_off, max_frags, result):
        """onc_frame_fragments: frame_stream at fragment level (every mark
        starts a fragment, whatever its last-fragment bit)."""
        self._check(self.lib.onc_frame_fragments(self.h, _ptr(wire), length, _ptr(frag_off), max_frags,
                                                 _ptr(result)), "onc_frame_fragments")

    def defragment(self, wire, frag_off, nfrag, out, rec_off, status, result, out_cap=None):
        """onc_defragment: the framed fragments rebuilt as a packed stream of
        single-fragment records in `out` (any byte address: a tensor or an
        int device pointer with out_cap); result = 6 words."""
        cap = out.numel() if out_cap is None else out_cap
        optr = C.c_void_p(out) if isinstance(out, int) else _ptr(out)
        self._check(self.lib.onc_defragment(self.h, _ptr(wire), _ptr(frag_off), nfrag, optr, cap, _ptr(rec_off),
                                            _ptr(status), _ptr(result)), "onc_defragment")

    def fragment(self, wire, rec_off, n, max_frag, out, out_off, status, result, out_cap=None):
        """onc_fragment: the records wire[rec_off[i], rec_off[i+1]) cut into
        fragments of at most max_frag body bytes in `out` (any byte address:
        a tensor or an int device pointer with out_cap); out_off = n + 1
        words, result = 3 words."""
        cap = out.numel() if out_cap is None else out_cap
        optr = C.c_void_p(out) if isinstance(out, int) else _ptr(out)
        self._check(self.lib.onc_fragment(self.h, _ptr(wire), _ptr(rec_off), n, max_frag, optr, cap, _ptr(out_off),
                                          _ptr(status), _ptr(result)), "onc_fragment")

    def fragment_iov(self, iov, n, max_frag, marks, pieces, out_off, piece_off, status, result, rec_max_frag=None,
                     marks_cap=None, max_pieces=None):
        """onc_fragment_iov: the records of onc_encode_iov's list cut into
        fragments of at most max_frag (or rec_max_frag[i]) body bytes with
        nothing copied: 4 bytes per fragment into `marks` and 16-byte pieces
        (layout.FRAG_PIECE_DTYPE) into `pieces` (uint8 tensors, None or int
        device pointers with a capacity); out_off and piece_off = n + 1
        words, result = 4 words."""
        def arg(t, cap, unit):
            if t is None:
                return None, (0 if cap is None else cap)
            if isinstance(t, int):
                return C.c_void_p(t), cap
            return _ptr(t), (t.numel() * t.element_size() // unit if cap is None else cap)
        mp, mcap = arg(marks, marks_cap, 1)
        pp, pcap = arg(pieces, max_pieces, 16)
        self._check(self.lib.onc_fragment_iov(self.h, _ptr(iov), n, max_frag, _ptr(rec_max_frag), mp, mcap, pp, pcap,
                                              _ptr(out_off), _ptr(piece_off), _ptr(status), _ptr(result)),
                    "onc_fragment_iov")

    def piece_offsets(self, pieces, npieces, src, piece_pos, result):
        """onc_piece_offsets: where every piece of the list starts in the
        stream (piece_pos = npieces + 1 words) and result = {stream bytes, bad
        pieces, first bad piece}. `src`: gather_src(marks, hdr, payload)."""
        self._check(self.lib.onc_piece_offsets(self.h, _ptr(pieces), npieces, C.byref(src), _ptr(piece_pos),
                                               _ptr(result)), "onc_piece_offsets")

    def gather_pieces(self, pieces, piece_pos, npieces, src, start, count, out):
        """onc_gather_pieces: stream bytes [start, start + count) of the piece
        list into `out` (any byte address: a tensor or an int device pointer,
        device or mapped host memory)."""
        optr = C.c_void_p(out) if isinstance(out, int) else _ptr(out)
        self._check(self.lib.onc_gather_pieces(self.h, _ptr(pieces), _ptr(piece_pos), npieces, C.byref(src), start,
                                               count, optr), "onc_gather_pieces")

    def payload_slots(self, msgs, status, n, align, pay_pos, pay_len, slot_off, result, head_len=0, rec_start=None,
                      msgs_out=None):
        """onc_payload_slots: per decoded record where its payload is in the
        record (pay_pos, pay_len) and the `align`-aligned slot it goes to
        (slot_off = n + 1 words); result = {records with a payload, payload
        bytes, destination bytes needed}. The heads form (head_len) unless
        rec_start gives onc_decode_extents' offsets; msgs_out (may be msgs):
        the descriptors with payload_off rebased to the slots."""
        self._check(self.lib.onc_payload_slots(self.h, _ptr(msgs), _ptr(status), n, head_len, _ptr(rec_start), align,
                                               _ptr(pay_pos), _ptr(pay_len), _ptr(slot_off), _ptr(msgs_out),
                                               _ptr(result)), "onc_payload_slots")

    def place_payloads(self, wire, frag_start, frag_len, nfrag, rec_frag, frag_pre, rec_len, pay_pos, pay_len,
                       slot_off, n, dst, dst_cap=None):
        """onc_place_payloads: every OK slice (pay_pos, pay_len) of record r,
        gathered from its fragments, into dst[slot_off[r], +pay_len[r])
        (`dst`: a tensor, or an int device pointer with dst_cap). rec_frag =
        frag_pre = None: record r is fragment r."""
        cap = dst.numel() if dst_cap is None else dst_cap
        dptr = C.c_void_p(dst) if isinstance(dst, int) else _ptr(dst)
        self._check(self.lib.onc_place_payloads(self.h, _ptr(wire), _ptr(frag_start), _ptr(frag_len), nfrag,
                                                _ptr(rec_frag), _ptr(frag_pre), _ptr(rec_len), _ptr(pay_pos),
                                                _ptr(pay_len), _ptr(slot_off), n, dptr, cap), "onc_place_payloads")

    def route_calls(self, msgs, status, n, table, ntab, nh, route, order, bin_first, result, calls_out=None,
                    replies=None):
        """onc_route_calls: every decoded record classified against the route
        table (L.ROUTE_DTYPE rows, sorted) into one of nh + 3 bins (route[n]),
        the records grouped stably by bin (order[n], bin_first[nh + 4]), and
        optionally the descriptors (calls_out) and the reply descriptors
        (replies) in that order; result = {Calls served, Calls rejected, other
        records, first bad table entry + 1}."""
        self._check(self.lib.onc_route_calls(self.h, _ptr(msgs), _ptr(status), n, _ptr(table), ntab, nh, _ptr(route),
                                             _ptr(order), _ptr(bin_first), _ptr(calls_out), _ptr(replies),
                                             _ptr(result)), "onc_route_calls")

    def xdr_unpack(self, wire, wire_len, msgs, status, n, fields, cols, xstat, result, flags=0, rec_start=None,
                   head_len=0, present=None, rest_pos=None, rest_len=None, replies=None, cols_cap=None):
        """onc_xdr_unpack: the payload of every payload-carrying record parsed
        against the schema `fields` (a host L.XDR_FIELD_DTYPE array) into one
        column per field inside `cols`, a parse status per record (xstat[n]),
        optionally the present bits, the unparsed rest and the GARBAGE_ARGS
        patch of `replies`; result = {OK records, garbage arguments, other
        records, 0}. `wire`: a tensor, or an int device pointer."""
        f = np.ascontiguousarray(fields, L.XDR_FIELD_DTYPE)
        cap = (cols.numel() * cols.element_size() if cols is not None else 0) if cols_cap is None else cols_cap
        wptr = C.c_void_p(wire) if isinstance(wire, int) else _ptr(wire)
        fptr = C.c_void_p(f.ctypes.data) if len(f) else None
        self._check(self.lib.onc_xdr_unpack(self.h, wptr, wire_len, _ptr(msgs), _ptr(status), n, _ptr(rec_start),
                                            head_len, fptr, len(f), flags, _ptr(cols), cap, _ptr(xstat),
                                            _ptr(present), _ptr(rest_pos), _ptr(rest_len), _ptr(replies),
                                            _ptr(result)), "onc_xdr_unpack")

    def match_replies(self, msgs, status, rec_conn, n, pending, npend, match, hit, result, tag_out=None, still=None):
        """onc_match_replies: every decoded record paired with the pending Call
        (L.PENDING_DTYPE rows) whose (conn, xid) it answers: match[n] (the
        entry's index or a MATCH_* sentinel), hit[npend] (the record, or
        MATCH_NONE), optionally the entries' tags per record (tag_out) and the
        entries still waiting, in list order (still); result = {matched,
        unknown, duplicate, not_reply, failed, still waiting}. rec_conn may be
        None: every record on connection 0."""
        self._check(self.lib.onc_match_replies(self.h, _ptr(msgs), _ptr(status), _ptr(rec_conn), n, _ptr(pending),
                                               npend, _ptr(match), _ptr(hit), _ptr(tag_out), _ptr(still),
                                               _ptr(result)), "onc_match_replies")

    def group_by_conn(self, rec_conn, nsrc, via, n, nconn, order, conn_first, result, msgs=None, msgs_out=None):
        """onc_group_by_conn: item k's connection is rec_conn[via[k]] (via
        None: rec_conn[k]), ids of nconn or more and indices of nsrc or more
        meaning "not sent"; the items sorted stably by connection (order[n]),
        every connection's first position (conn_first[nconn + 2]; the dropped
        items are group nconn) and optionally the descriptors in that order
        (msgs_out[j] = msgs[order[j]]); result = {items sent, items dropped,
        connections with an item}."""
        self._check(self.lib.onc_group_by_conn(self.h, _ptr(rec_conn), nsrc, _ptr(via), n, nconn, _ptr(order),
                                               _ptr(conn_first), _ptr(msgs), _ptr(msgs_out), _ptr(result)),
                    "onc_group_by_conn")

    def conn_extents(self, rec_off, nrec, conn_first, nconn, conn_off):
        """onc_conn_extents: conn_off[c] = rec_off[min(conn_first[c], nrec)]
        for c in 0 .. nconn + 1: connection c's bytes of the encoded stream
        are [conn_off[c], conn_off[c + 1])."""
        self._check(self.lib.onc_conn_extents(self.h, _ptr(rec_off), nrec, _ptr(conn_first), nconn, _ptr(conn_off)),
                    "onc_conn_extents")

    def frame_streams(self, wire, seg_off, seg_len, nseg, rec_start, rec_len, rec_seg, max_records, seg_result,
                      result):
        """onc_frame_streams: segment s = wire[seg_off[s], +seg_len[s]) framed
        on its own, all in one call (rec_seg may be None); seg_result = 6
        words per segment, result = 3 words."""
        self._check(self.lib.onc_frame_streams(self.h, _ptr(wire), _ptr(seg_off), _ptr(seg_len), nseg,
                                               _ptr(rec_start), _ptr(rec_len), _ptr(rec_seg), max_records,
                                               _ptr(seg_result), _ptr(result)), "onc_frame_streams")

    def frame_fragment_streams(self, wire, seg_off, seg_len, nseg, frag_start, frag_len, frag_seg, max_frags,
                               seg_result, result):
        """onc_frame_fragment_streams: frame_streams at fragment level — the
        fragments of every segment's complete records as extents (frag_seg
        may be None); seg_result = 8 words per segment, result = 4 words."""
        self._check(self.lib.onc_frame_fragment_streams(self.h, _ptr(wire), _ptr(seg_off), _ptr(seg_len), nseg,
                                                        _ptr(frag_start), _ptr(frag_len), _ptr(frag_seg), max_frags,
                                                        _ptr(seg_result), _ptr(result)),
                    "onc_frame_fragment_streams")

    def defragment_extents(self, wire, frag_start, frag_len, nfrag, out, rec_off, status, result, out_cap=None):
        """onc_defragment_extents: defragment of the fragments
        wire[frag_start[j], +frag_len[j]) (`out`: a tensor or an int device
        pointer with out_cap); result = 6 words, result[1] counts fragments."""
        cap = out.numel() if out_cap is None else out_cap
        optr = C.c_void_p(out) if isinstance(out, int) else _ptr(out)
        self._check(self.lib.onc_defragment_extents(self.h, _ptr(wire), _ptr(frag_start), _ptr(frag_len), nfrag, optr,
                                                    cap, _ptr(rec_off), _ptr(status), _ptr(result)),
                    "onc_defragment_extents")

    def defragment_heads(self, wire, frag_start, frag_len, nfrag, head_len, heads, max_records, rec_len, rec_frag,
                         frag_pre, status, result):
        """onc_defragment_heads: the first head_len bytes of every record of
        the fragments wire[frag_start[j], +frag_len[j]) into fixed-stride
        slots (`heads`: a tensor or an int device pointer); rec_frag /
        frag_pre locate the rest; result = 6 words, result[2] the heads bytes
        the batch needs."""
        hptr = C.c_void_p(heads) if isinstance(heads, int) else _ptr(heads)
        self._check(self.lib.onc_defragment_heads(self.h, _ptr(wire), _ptr(frag_start), _ptr(frag_len), nfrag, head_len,
                                                  hptr, max_records, _ptr(rec_len), _ptr(rec_frag), _ptr(frag_pre),
                                                  _ptr(status), _ptr(result)), "onc_defragment_heads")

    # -- decode -----------------------------------------------------------
    def decode_heads(self, heads, head_len, rec_len, n, mode, msgs, unix, status, aux0, aux1):
        """onc_decode_heads: record i has rec_len[i] bytes, of which the first
        min(rec_len[i], head_len) are at heads + i * head_len; offsets in the
        outputs are relative to `heads` (a tensor or an int device pointer)."""
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        hptr = C.c_void_p(heads) if isinstance(heads, int) else _ptr(heads)
        self._check(self.lib.onc_decode_heads(self.h, hptr, head_len, _ptr(rec_len), n, mode, C.byref(d)),
                    "onc_decode_heads")

    def decode_extents(self, wire, wire_len, rec_start, rec_len, n, mode, msgs, unix, status, aux0, aux1):
        """onc_decode_extents: record i = wire[rec_start[i], +rec_len[i]), in
        any order, bounded by wire_len (2**64 - 1: the extents are trusted)."""
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        self._check(self.lib.onc_decode_extents(self.h, _ptr(wire), wire_len, _ptr(rec_start), _ptr(rec_len), n, mode,
                                                C.byref(d)), "onc_decode_extents")

    def decode(self, wire, rec_off, n, mode, msgs, unix, status, aux0, aux1):
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        self._check(self.lib.onc_decode(self.h, _ptr(wire), _ptr(rec_off), n, mode, C.byref(d)),
                    "onc_decode")

    def decode_lengths(self, wire, rec_len, n, base, mode, msgs, unix, status, aux0, aux1, rec_off=None):
        """onc_decode_lengths: offsets from rec_len inside the decode (rec_off
        optional: receives them, n + 1 entries)."""
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        self._check(self.lib.onc_decode_lengths(self.h, _ptr(wire), _ptr(rec_len), n, base, mode,
                                                _ptr(rec_off) if rec_off is not None else None, C.byref(d)),
                    "onc_decode_lengths")

    # -- body-level roots (ONC_ROOT_*) ---------------------------------------
    def decode_body(self, root, wire, rec_off, n, mode, msgs, unix, status, aux0, aux1, param=None, consumed=None):
        """onc_decode_body: each record decoded as `root`'s TryFrom."""
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        self._check(self.lib.onc_decode_body(self.h, root, _ptr(wire), _ptr(rec_off), n, mode, _ptr(param),
                                             C.byref(d), _ptr(consumed)), "onc_decode_body")

    # -- bounded decode: the three above with the wire's readable length ------
    # (a record whose extent leaves [0, wire_len) is L.DEC_BAD_EXTENT, unread)
    def decode_bounded(self, wire, wire_len, rec_off, n, mode, msgs, unix, status, aux0, aux1):
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        self._check(self.lib.onc_decode_bounded(self.h, _ptr(wire), wire_len, _ptr(rec_off), n, mode, C.byref(d)),
                    "onc_decode_bounded")

    def decode_lengths_bounded(self, wire, wire_len, rec_len, n, base, mode, msgs, unix, status, aux0, aux1,
                               rec_off=None):
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        self._check(self.lib.onc_decode_lengths_bounded(self.h, _ptr(wire), wire_len, _ptr(rec_len), n, base, mode,
                                                        _ptr(rec_off) if rec_off is not None else None, C.byref(d)),
                    "onc_decode_lengths_bounded")

    def decode_body_bounded(self, root, wire, wire_len, rec_off, n, mode, msgs, unix, status, aux0, aux1,
                            param=None, consumed=None):
        d = OncDecoded(msgs.data_ptr(), unix.data_ptr(), status.data_ptr(), aux0.data_ptr(),
                       aux1.data_ptr())
        self._check(self.lib.onc_decode_body_bounded(self.h, root, _ptr(wire), wire_len, _ptr(rec_off), n, mode,
                                                     _ptr(param), C.byref(d), _ptr(consumed)),
                    "onc_decode_body_bounded")

    def encode_body_lengths(self, root, batch: DeviceBatch, rec_len, status):
        b = batch.c_struct()
        self._check(self.lib.onc_encode_body_lengths(self.h, root, C.byref(b), _ptr(rec_len), _ptr(status)),
                    "onc_encode_body_lengths")

    def encode_body(self, root, batch: DeviceBatch, out, rec_off, status, rec_len=None, out_cap=None):
        b = batch.c_struct()
        cap = out.numel() if out_cap is None else out_cap
        self._check(self.lib.onc_encode_body(self.h, root, C.byref(b), _ptr(out), cap, _ptr(rec_off), _ptr(status),
                                             _ptr(rec_len)), "onc_encode_body")

    def compact(self, out, rec_off, status, n):
        """onc_compact: the extents of records with status != OK dropped from
        an encoded buffer in place (rec_off rewritten); returns the new
        rec_off[n]."""
        total = C.c_uint64(0)
        self._check(self.lib.onc_compact(self.h, _ptr(out), _ptr(rec_off), _ptr(status), n, C.byref(total)),
                    "onc_compact")
        return total.value

    def compact_iov(self, iov, status, n, totals=None):
        """onc_compact_iov: failing records' iovecs emptied, wire_off re-placed."""
        self._check(self.lib.onc_compact_iov(self.h, _ptr(iov), _ptr(status), n, _ptr(totals)), "onc_compact_iov")

    def scan_lengths(self, rec_len, n, base, rec_off):
        self._check(self.lib.onc_scan_lengths(self.h, _ptr(rec_len), n, base, _ptr(rec_off)),
                    "onc_scan_lengths")


class HostMapped:
    """A host buffer the kernels read and write in place (onc_host_register):
    page-aligned anonymous memory, as a socket buffer would be. `host` is its
    numpy byte view (typed views: view(dtype)); data_ptr() is the device
    address, so it goes wherever a device tensor goes in this binding
    (Codec calls, DeviceBatch fields). close() unregisters it."""

    # bytes registered through HostMapped in this process, now and at most
    # (bench.py reports the pinned host memory a run holds)
    live_bytes = 0
    peak_bytes = 0

    def __init__(self, codec: "Codec", nbytes: int):
        self.nbytes = int(nbytes)
        self._dev = None
        self._mm = mmap.mmap(-1, max(self.nbytes, 4096))
        self.host = np.frombuffer(self._mm, np.uint8, count=self.nbytes)
        self._addr = self.host.ctypes.data if self.nbytes else np.frombuffer(self._mm, np.uint8).ctypes.data
        self._codec = codec
        dev = C.c_void_p()
        codec._check(codec.lib.onc_host_register(codec.h, C.c_void_p(self._addr), max(self.nbytes, 4096),
                                                  C.byref(dev)), "onc_host_register")
        self._dev = dev.value
        HostMapped.live_bytes += max(self.nbytes, 4096)
        HostMapped.peak_bytes = max(HostMapped.peak_bytes, HostMapped.live_bytes)

    @classmethod
    def from_array(cls, codec, arr):
        """A mapped copy of a numpy array's bytes."""
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        m = cls(codec, raw.size)
        m.host[:] = raw
        return m

    def data_ptr(self):
        return self._dev

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def view(self, dtype):
        return self.host.view(dtype)

    def close(self):
        # unregistered whether or not its codec is still open (a pinned range
        # belongs to the process: onc_host_unregister takes a NULL codec), so
        # the pages are unpinned before the mapping is freed
        if self._dev is not None:
            self._codec.lib.onc_host_unregister(self._codec.h or None, C.c_void_p(self._addr))
            HostMapped.live_bytes -= max(self.nbytes, 4096)
        self._dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_device_pointer(codec: "Codec", t):
    """Device address of a pinned host tensor (torch pin_memory =
    hipHostMalloc): onc_host_register maps it without registering it again."""
    dev = C.c_void_p()
    codec._check(codec.lib.onc_host_register(codec.h, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(),
                                             C.byref(dev)), "onc_host_register")
    return dev.value


class MappedHostBatch:
    """A HostBatch whose arrays live in mapped host memory (HostMapped): an
    onc_batch the kernels read in place — descriptors, AUTH_UNIX table and
    arenas never copied to the device."""

    def __init__(self, codec, hb: L.HostBatch):
        self.n = hb.n
        self.msgs = HostMapped.from_array(codec, hb.msgs)
        self.unix = HostMapped.from_array(codec, hb.unix if hb.unix.size else np.zeros(1, L.UNIX_DTYPE))
        self.auth_arena = HostMapped.from_array(codec, hb.auth_arena if hb.auth_arena.size else np.zeros(16, np.uint8))
        self.payload_arena = HostMapped.from_array(codec, hb.payload_arena if hb.payload_arena.size
                                                   else np.zeros(16, np.uint8))
        self.unix_count = hb.unix.size
        self.auth_len = hb.auth_arena.size
        self.payload_len = hb.payload_arena.size

    def c_struct(self):
        return OncBatch(self.n, self.msgs.data_ptr(), self.unix.data_ptr(), self.auth_arena.data_ptr(),
                        self.payload_arena.data_ptr(), self.unix_count, self.auth_len, self.payload_len)

    def close(self):
        for m in (self.msgs, self.unix, self.auth_arena, self.payload_arena):
            m.close()


class DecodeBuffers:
    """Device output buffers for a decode of n records."""

    def __init__(self, n, device="cuda"):
        torch = _torch()
        self.n = n
        m = max(n, 1)
        self.msgs = torch.empty(m * 64, dtype=torch.uint8, device=device)
        self.unix = torch.empty(2 * m * 96, dtype=torch.uint8, device=device)
        self.status = torch.empty(m, dtype=torch.int32, device=device)
        self.aux0 = torch.empty(m, dtype=torch.int32, device=device)
        self.aux1 = torch.empty(m, dtype=torch.int32, device=device)

    def to_host(self):
        msgs = self.msgs.cpu().numpy().view(L.MSG_DTYPE)[: self.n]
        unix = self.unix.cpu().numpy().view(L.UNIX_DTYPE)[: 2 * self.n]
        return (msgs, unix, self.status.cpu().numpy()[: self.n].copy(),
                self.aux0.cpu().numpy().view(np.uint32)[: self.n].copy(),
                self.aux1.cpu().numpy().view(np.uint32)[: self.n].copy())


def encode_host_batch(codec: Codec, hb: L.HostBatch, device="cuda", out_cap=None):
    """Convenience: host batch -> GPU encode -> (wire bytes, rec_off, status, rec_len) on host."""
    torch = _torch()
    db = DeviceBatch.from_host(hb, device)
    n = hb.n
    lens = codec_lengths(codec, db)
    total = int(lens.sum())
    cap = total if out_cap is None else out_cap
    out = torch.zeros(max(16, (cap + 15) // 16 * 16), dtype=torch.uint8, device=device)
    rec_off = torch.empty(n + 1, dtype=torch.int64, device=device)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    rec_len = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    codec.encode(db, out, rec_off, status, rec_len, out_cap=cap)
    codec.sync()
    return (out.cpu().numpy()[:min(total, cap)].tobytes(), rec_off.cpu().numpy().view(np.uint64).copy(),
            status.cpu().numpy()[:n].copy(), rec_len.cpu().numpy().view(np.uint32)[:n].copy())


def frame_host_stream(codec: Codec, buf: bytes, max_records=None, device="cuda"):
    """Convenience: host stream bytes -> GPU framing -> (rec_off[n+1], n, consumed, status, aux0, aux1)."""
    torch = _torch()
    w = to_device(np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8), device)
    m = len(buf) // 4 + 1 if max_records is None else max_records
    off = torch.zeros(m + 1, dtype=torch.int64, device=device)
    res = torch.zeros(5, dtype=torch.int64, device=device)
    codec.frame_stream(w, len(buf), off, m, res)
    codec.sync()
    r = res.cpu().numpy()
    n = int(r[0])
    return (off.cpu().numpy().view(np.uint64)[:n + 1].copy(), n, int(r[1]), int(r[2]), int(np.uint32(r[3])),
            int(np.uint32(r[4])))


def frame_host_fragments(codec: Codec, buf: bytes, max_frags=None, device="cuda"):
    """frame_host_stream at fragment level -> (frag_off[n+1], n, consumed, status, aux0, aux1)."""
    torch = _torch()
    w = to_device(np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8), device)
    m = len(buf) // 4 + 1 if max_frags is None else max_frags
    off = torch.zeros(m + 1, dtype=torch.int64, device=device)
    res = torch.zeros(5, dtype=torch.int64, device=device)
    codec.frame_fragments(w, len(buf), off, m, res)
    codec.sync()
    r = res.cpu().numpy()
    n = int(r[0])
    return (off.cpu().numpy().view(np.uint64)[:n + 1].copy(), n, int(r[1]), int(r[2]), int(np.uint32(r[3])),
            int(np.uint32(r[4])))


def frame_host_streams(codec: Codec, slab, seg_off, seg_len, max_records=None, device="cuda", with_seg=True):
    """Convenience: a host slab and its segments -> onc_frame_streams ->
    (rec_start[n], rec_len[n], rec_seg[n] or None, seg_result[nseg, 6],
    result[3]) on the host. max_records None: room for every mark the
    segments can hold."""
    torch = _torch()
    w = to_device(np.frombuffer(bytes(slab) + b"\0" * 16, np.uint8), device)
    so = np.ascontiguousarray(seg_off, np.uint64)
    sl = np.ascontiguousarray(seg_len, np.uint64)
    nseg = len(so)
    m = int(sl.sum()) // 4 + 1 if max_records is None else max_records
    d_so = torch.from_numpy(np.append(so, np.uint64(0)).view(np.int64).copy()).to(device)
    d_sl = torch.from_numpy(np.append(sl, np.uint64(0)).view(np.int64).copy()).to(device)
    start = torch.full((m + 1,), -1, dtype=torch.int64, device=device)
    rlen = torch.full((m + 1,), -1, dtype=torch.int32, device=device)
    rseg = torch.full((m + 1,), -1, dtype=torch.int32, device=device) if with_seg else None
    rows = torch.full((6 * nseg + 1,), -1, dtype=torch.int64, device=device)
    res = torch.full((3,), -1, dtype=torch.int64, device=device)
    codec.frame_streams(w, d_so, d_sl, nseg, start, rlen, rseg, m, rows, res)
    codec.sync()
    r = res.cpu().numpy().view(np.uint64).copy()
    n = int(r[0])
    return (start.cpu().numpy().view(np.uint64)[:n].copy(), rlen.cpu().numpy().view(np.uint32)[:n].copy(),
            rseg.cpu().numpy().view(np.uint32)[:n].copy() if with_seg else None,
            rows.cpu().numpy().view(np.uint64)[:6 * nseg].reshape(nseg, 6).copy(), r)


def frame_host_fragment_streams(codec: Codec, slab, seg_off, seg_len, max_frags=None, device="cuda", with_seg=True):
    """Convenience: a host slab and its segments -> onc_frame_fragment_streams
    -> (frag_start[n], frag_len[n], frag_seg[n] or None, seg_result[nseg, 8],
    result[4]) on the host. max_frags None: room for every mark the segments
    can hold."""
    torch = _torch()
    w = to_device(np.frombuffer(bytes(slab) + b"\0" * 16, np.uint8), device)
    so = np.ascontiguousarray(seg_off, np.uint64)
    sl = np.ascontiguousarray(seg_len, np.uint64)
    nseg = len(so)
    m = int(sl.sum()) // 4 + 1 if max_frags is None else max_frags
    d_so = torch.from_numpy(np.append(so, np.uint64(0)).view(np.int64).copy()).to(device)
    d_sl = torch.from_numpy(np.append(sl, np.uint64(0)).view(np.int64).copy()).to(device)
    start = torch.full((m + 1,), -1, dtype=torch.int64, device=device)
    flen = torch.full((m + 1,), -1, dtype=torch.int32, device=device)
    fseg = torch.full((m + 1,), -1, dtype=torch.int32, device=device) if with_seg else None
    rows = torch.full((8 * nseg + 1,), -1, dtype=torch.int64, device=device)
    res = torch.full((4,), -1, dtype=torch.int64, device=device)
    codec.frame_fragment_streams(w, d_so, d_sl, nseg, start, flen, fseg, m, rows, res)
    codec.sync()
    r = res.cpu().numpy().view(np.uint64).copy()
    n = int(r[0])
    return (start.cpu().numpy().view(np.uint64)[:n].copy(), flen.cpu().numpy().view(np.uint32)[:n].copy(),
            fseg.cpu().numpy().view(np.uint32)[:n].copy() if with_seg else None,
            rows.cpu().numpy().view(np.uint64)[:8 * nseg].reshape(nseg, 8).copy(), r)


def defragment_host_extents(codec: Codec, wire, frag_start, frag_len, out_cap=None, shift=0, device="cuda"):
    """Convenience: host wire bytes and fragment extents ->
    onc_defragment_extents -> (the out_cap bytes from `out` on (out_cap None:
    the bytes the batch needs), rec_off[n+1], status[n], result[6]) on the
    host. `out` starts `shift` bytes past a 16-byte aligned address and is
    zero-filled before the call."""
    torch = _torch()
    fs = np.ascontiguousarray(frag_start, np.uint64)
    fl = np.ascontiguousarray(frag_len, np.uint32)
    nfrag = len(fs)
    w = to_device(np.frombuffer(bytes(wire) + b"\0" * 16, np.uint8), device)
    d_fs = torch.from_numpy(np.append(fs, np.uint64(0)).view(np.int64).copy()).to(device)
    d_fl = torch.from_numpy(np.append(fl, np.uint32(0)).view(np.int32).copy()).to(device)
    cap = int(fl.sum()) if out_cap is None else out_cap      # a reassembled record is never longer than its fragments
    base = torch.zeros(16 + shift + cap + 16, dtype=torch.uint8, device=device)
    lo = (-base.data_ptr()) % 16 + shift
    rec_off = torch.zeros(nfrag + 1, dtype=torch.int64, device=device)
    status = torch.zeros(max(nfrag, 1), dtype=torch.int32, device=device)
    res = torch.zeros(6, dtype=torch.int64, device=device)
    codec.defragment_extents(w, d_fs, d_fl, nfrag, base.data_ptr() + lo, rec_off, status, res, out_cap=cap)
    codec.sync()
    r = res.cpu().numpy().view(np.uint64).copy()
    n = int(r[0])
    size = min(int(r[2]), cap) if out_cap is None else cap
    return (base.cpu().numpy()[lo:lo + size].tobytes(), rec_off.cpu().numpy().view(np.uint64)[:n + 1].copy(),
            status.cpu().numpy()[:n].copy(), r)


def reassemble_host_streams(codec: Codec, slab, seg_off, seg_len, device="cuda"):
    """Convenience: a host slab and its segments -> onc_frame_fragment_streams
    + onc_defragment_extents -> (reassembled bytes, rec_off[n+1], status[n],
    seg_result[nseg, 8], framing result[4], defragment result[6]) on the host.
    The reassembled bytes are a packed stream of single-fragment records:
    records [first_rec, first_rec + n_rec) of it are segment s's."""
    start, flen, _, rows, fres = frame_host_fragment_streams(codec, slab, seg_off, seg_len, device=device,
                                                              with_seg=False)
    out, rec_off, status, res = defragment_host_extents(codec, slab, start, flen, device=device)
    return out, rec_off, status, rows, fres, res


def decode_host_extents(codec: Codec, wire: np.ndarray, rec_start, rec_len, mode, wire_len=None, device="cuda"):
    """Convenience: a host wire and extents -> onc_decode_extents -> host
    arrays (wire_len None: the wire's size)."""
    torch = _torch()
    n = len(rec_start)
    w = to_device(wire, device)
    st = torch.from_numpy(np.append(np.asarray(rec_start, np.uint64), np.uint64(0)).view(np.int64).copy()).to(device)
    ln = torch.from_numpy(np.append(np.asarray(rec_len, np.uint32), np.uint32(0)).view(np.int32).copy()).to(device)
    bufs = DecodeBuffers(n, device)
    codec.decode_extents(w, len(wire) if wire_len is None else wire_len, st, ln, n, mode, bufs.msgs, bufs.unix,
                         bufs.status, bufs.aux0, bufs.aux1)
    codec.sync()
    return bufs.to_host()


def aligned_bytes(nbytes, fill=0, device="cuda"):
    """(tensor, lo): a uint8 device tensor whose element lo is 16-byte aligned
    with nbytes usable bytes from there and 16 bytes behind them, every byte
    `fill`."""
    torch = _torch()
    base = torch.full((16 + nbytes + 16,), fill, dtype=torch.uint8, device=device)
    return base, (-base.data_ptr()) % 16


def defragment_host_heads(codec: Codec, wire, frag_start, frag_len, head_len, max_records=None, fill=0, device="cuda"):
    """Convenience: host wire bytes and fragment extents ->
    onc_defragment_heads -> a dict of host arrays: heads (max_records *
    head_len bytes, `fill` where nothing was written; max_records None: one
    slot per fragment), rec_len[n], rec_frag[n+1], frag_pre[nfrag], status[n],
    result[6], and `raw`: the whole output arrays, pre-filled with sentinels
    (-1; heads `fill`), so that a caller can see what was left alone."""
    torch = _torch()
    fs = np.ascontiguousarray(frag_start, np.uint64)
    fl = np.ascontiguousarray(frag_len, np.uint32)
    nfrag = len(fs)
    w = to_device(np.frombuffer(bytes(wire) + b"\0" * 16, np.uint8), device)
    d_fs = torch.from_numpy(np.append(fs, np.uint64(0)).view(np.int64).copy()).to(device)
    d_fl = torch.from_numpy(np.append(fl, np.uint32(0)).view(np.int32).copy()).to(device)
    slots = nfrag if max_records is None else max_records
    base, lo = aligned_bytes(slots * head_len + head_len, fill, device)     # one slot more: a stray write shows
    rec_len = torch.full((nfrag + 1,), -1, dtype=torch.int32, device=device)
    rec_frag = torch.full((nfrag + 2,), -1, dtype=torch.int64, device=device)
    frag_pre = torch.full((nfrag + 1,), -1, dtype=torch.int64, device=device)
    status = torch.full((nfrag + 1,), -1, dtype=torch.int32, device=device)
    res = torch.full((6,), -1, dtype=torch.int64, device=device)
    codec.defragment_heads(w, d_fs, d_fl, nfrag, head_len, base.data_ptr() + lo, slots, rec_len, rec_frag, frag_pre,
                           status, res)
    codec.sync()
    r = res.cpu().numpy().view(np.uint64).copy()
    n = int(r[0])
    raw = {"heads": base.cpu().numpy()[lo:lo + slots * head_len + head_len].copy(),
           "rec_len": rec_len.cpu().numpy().view(np.uint32).copy(),
           "rec_frag": rec_frag.cpu().numpy().view(np.uint64).copy(),
           "frag_pre": frag_pre.cpu().numpy().view(np.uint64).copy(), "status": status.cpu().numpy().copy()}
    return {"heads": raw["heads"][:slots * head_len], "rec_len": raw["rec_len"][:n], "rec_frag": raw["rec_frag"][:n + 1],
            "frag_pre": raw["frag_pre"][:nfrag], "status": raw["status"][:n], "result": r, "raw": raw}


def decode_host_heads(codec: Codec, heads, head_len, rec_len, mode, device="cuda"):
    """Convenience: host heads (n * head_len bytes) and record lengths ->
    onc_decode_heads -> host arrays, as decode_host_wire."""
    torch = _torch()
    ln = np.ascontiguousarray(rec_len, np.uint32)
    n = len(ln)
    raw = np.frombuffer(bytes(heads), np.uint8)
    assert len(raw) >= n * head_len
    base, lo = aligned_bytes(max(len(raw), 16), 0, device)
    if len(raw):
        base[lo:lo + len(raw)] = torch.from_numpy(raw.copy()).to(device)
    d_ln = torch.from_numpy(np.append(ln, np.uint32(0)).view(np.int32).copy()).to(device)
    bufs = DecodeBuffers(n, device)
    codec.decode_heads(base.data_ptr() + lo, head_len, d_ln, n, mode, bufs.msgs, bufs.unix, bufs.status, bufs.aux0,
                       bufs.aux1)
    codec.sync()
    return bufs.to_host()


def _dev_words(arr, dtype, view, device, extra=1):
    """A host array as a device tensor of `view` words, `extra` zero words behind it."""
    torch = _torch()
    a = np.ascontiguousarray(arr, dtype)
    return torch.from_numpy(np.append(a, np.zeros(extra, dtype)).view(view).copy()).to(device)


def payload_slots_host(codec: Codec, msgs, status, align, head_len=0, rec_start=None, msgs_out=None, extra=4,
                       device="cuda"):
    """Convenience: host descriptors (L.MSG_DTYPE) and statuses ->
    onc_payload_slots -> a dict of host arrays: pay_pos[n], pay_len[n],
    slot_off[n + 1], result[3], msgs_out[n] (None unless msgs_out is
    "separate" or "inplace": written to msgs itself), and `raw`: the whole
    output arrays with `extra` words behind them, pre-filled with sentinels
    (-1; descriptors 0xA5), so that a caller can see what was left alone."""
    torch = _torch()
    m = np.ascontiguousarray(msgs, L.MSG_DTYPE)
    n = len(m)
    d_msgs = torch.full(((n + extra) * 64,), 0xA5, dtype=torch.uint8, device=device)
    if n:
        d_msgs[:n * 64] = torch.from_numpy(m.view(np.uint8).reshape(-1).copy()).to(device)
    d_st = _dev_words(status, np.int32, np.int32, device)
    d_rs = None if rec_start is None else _dev_words(rec_start, np.uint64, np.int64, device)
    pay_pos = torch.full((n + extra,), -1, dtype=torch.int32, device=device)
    pay_len = torch.full((n + extra,), -1, dtype=torch.int32, device=device)
    slot_off = torch.full((n + 1 + extra,), -1, dtype=torch.int64, device=device)
    res = torch.full((3 + extra,), -1, dtype=torch.int64, device=device)
    d_out = None
    if msgs_out == "separate":
        d_out = torch.full(((n + extra) * 64,), 0xA5, dtype=torch.uint8, device=device)
    elif msgs_out == "inplace":
        d_out = d_msgs
    codec.payload_slots(d_msgs, d_st, n, align, pay_pos, pay_len, slot_off, res, head_len=head_len, rec_start=d_rs,
                        msgs_out=d_out)
    codec.sync()
    raw = {"pay_pos": pay_pos.cpu().numpy().view(np.uint32).copy(), "pay_len": pay_len.cpu().numpy().view(np.uint32).copy(),
           "slot_off": slot_off.cpu().numpy().view(np.uint64).copy(), "result": res.cpu().numpy().view(np.uint64).copy(),
           "msgs": d_msgs.cpu().numpy().copy(), "msgs_out": None if d_out is None else d_out.cpu().numpy().copy()}
    return {"pay_pos": raw["pay_pos"][:n], "pay_len": raw["pay_len"][:n], "slot_off": raw["slot_off"][:n + 1],
            "result": raw["result"][:3],
            "msgs_out": None if d_out is None else raw["msgs_out"][:n * 64].view(L.MSG_DTYPE), "raw": raw}


ROUTE_TILE = 1024           # ONC_ROUTE_TILE: records per workgroup of onc_route_calls' kernels
ROUTE_TABLE_MAX, ROUTE_HANDLERS_MAX, ROUTE_ONE_HANDLER = 1024, 253, 1


def route_table(rows):
    """(program, version, proc_first, proc_count, handler_first, flags) rows ->
    an L.ROUTE_DTYPE array, as given (onc_route_calls wants them sorted)."""
    t = np.zeros(len(rows), L.ROUTE_DTYPE)
    for i, row in enumerate(rows):
        t[i] = tuple(row)
    return t


def route_calls_host(codec: Codec, msgs, status, table, nh, calls_out=True, replies=True, extra=4, device="cuda"):
    """Convenience: host descriptors (L.MSG_DTYPE), statuses and a route table
    (L.ROUTE_DTYPE) -> onc_route_calls -> a dict of host arrays: route[n],
    order[n], bin_first[nh + 4], result[4], calls_out[n] and replies[n] (None
    when not asked for), and `raw`: the whole output arrays with `extra` words
    behind them, pre-filled with sentinels (-1; descriptors 0xA5), so that a
    caller can see what was left alone."""
    torch = _torch()
    m = np.ascontiguousarray(msgs, L.MSG_DTYPE)
    t = np.ascontiguousarray(table, L.ROUTE_DTYPE)
    n = len(m)
    d_msgs = to_device(m, device)
    d_st = _dev_words(status, np.int32, np.int32, device)
    d_tab = to_device(t, device) if len(t) else None
    route = torch.full((n + extra,), -1, dtype=torch.int32, device=device)
    order = torch.full((n + extra,), -1, dtype=torch.int32, device=device)
    bin_first = torch.full((nh + 4 + extra,), -1, dtype=torch.int64, device=device)
    res = torch.full((4 + extra,), -1, dtype=torch.int64, device=device)
    d_calls = torch.full(((n + extra) * 64,), 0xA5, dtype=torch.uint8, device=device) if calls_out else None
    d_rep = torch.full(((n + extra) * 64,), 0xA5, dtype=torch.uint8, device=device) if replies else None
    codec.route_calls(d_msgs, d_st, n, d_tab, len(t), nh, route, order, bin_first, res, calls_out=d_calls,
                      replies=d_rep)
    codec.sync()
    raw = {"route": route.cpu().numpy().view(np.uint32).copy(), "order": order.cpu().numpy().view(np.uint32).copy(),
           "bin_first": bin_first.cpu().numpy().view(np.uint64).copy(), "result": res.cpu().numpy().view(np.uint64).copy(),
           "calls_out": None if d_calls is None else d_calls.cpu().numpy().copy(),
           "replies": None if d_rep is None else d_rep.cpu().numpy().copy()}
    return {"route": raw["route"][:n], "order": raw["order"][:n], "bin_first": raw["bin_first"][:nh + 4],
            "result": raw["result"][:4],
            "calls_out": None if d_calls is None else raw["calls_out"][:n * 64].view(L.MSG_DTYPE),
            "replies": None if d_rep is None else raw["replies"][:n * 64].view(L.MSG_DTYPE), "raw": raw}


XDR_TILE = 256              # ONC_XDR_TILE: records per workgroup of onc_xdr_unpack's kernel
XDR_FIELDS_MAX = 64
XDR_U32, XDR_U64, XDR_BOOL, XDR_OPAQUE_FIXED, XDR_OPAQUE_VAR, XDR_ARRAY32, XDR_ARRAY64 = range(7)
XDR_SELECT, XDR_IF, XDR_NO_COLUMN = 0x100, 0x200, 0x400
XDR_EXACT = 0x1
(XDR_OK, XDR_SKIPPED, XDR_BAD_EXTENT, XDR_SHORT, XDR_BAD_BOOL, XDR_TOO_LONG, XDR_TRAILING,
 XDR_HEAD_SHORT) = range(8)


def xdr_col_width(type_flags):
    """Bytes a record takes in the column of a field of this type."""
    return 4 if (type_flags & 0xFF) in (XDR_U32, XDR_BOOL, XDR_OPAQUE_FIXED) else 8


def xdr_schema(specs, n):
    """(type_flags, arg, cond_val) rows -> (an L.XDR_FIELD_DTYPE array with the
    columns of n records laid out back to back in field order, every column
    8-byte aligned; the bytes they take). A NO_COLUMN field takes none."""
    f = np.zeros(len(specs), L.XDR_FIELD_DTYPE)
    off = 0
    for i, (tf, arg, cond) in enumerate(specs):
        f[i]["type_flags"], f[i]["arg"], f[i]["cond_val"] = tf, arg, cond
        if not tf & XDR_NO_COLUMN:
            f[i]["col_off"] = off
            off += (xdr_col_width(tf) * n + 7) & ~7
    return f, off


def xdr_schema_check(fields, n, cols_cap):
    """onc_xdr_schema_check: 0, the first bad field + 1, or ONC_RC_EINVAL."""
    lib = load_library()
    f = np.ascontiguousarray(fields, L.XDR_FIELD_DTYPE)
    return lib.onc_xdr_schema_check(C.c_void_p(f.ctypes.data) if len(f) else None, len(f), n, cols_cap)


def xdr_unpack_host(codec: Codec, wire, msgs, status, fields, cols_cap, flags=0, rec_start=None, head_len=0,
                    present=True, rest=True, replies=None, wire_len=None, extra=4, device="cuda"):
    """Convenience: a host wire (uint8 array; or a (tensor-or-int pointer,
    wire_len) already on the device), host descriptors (L.MSG_DTYPE), statuses
    and a schema -> onc_xdr_unpack -> a dict of host arrays: cols[cols_cap]
    (bytes), xstat[n], present[n], rest_pos[n], rest_len[n], replies[n] (None
    when not asked for; `replies`: the host skeletons to patch), result[4], and
    `raw`: the whole output arrays with `extra` words (cols: 8 `extra` bytes)
    behind them, pre-filled with sentinels (-1; cols 0xA5), so that a caller
    can see what was left alone."""
    torch = _torch()
    m = np.ascontiguousarray(msgs, L.MSG_DTYPE)
    n = len(m)
    if isinstance(wire, np.ndarray):
        d_wire = to_device(np.append(wire, np.zeros(16, np.uint8)), device)
        wlen = len(wire) if wire_len is None else wire_len
    else:
        d_wire, wlen = wire, wire_len
    d_msgs = to_device(m, device)
    d_st = _dev_words(status, np.int32, np.int32, device)
    d_rs = None if rec_start is None else _dev_words(rec_start, np.uint64, np.int64, device)
    cols = torch.full((cols_cap + 8 * extra,), 0xA5, dtype=torch.uint8, device=device)
    xstat = torch.full((n + extra,), -1, dtype=torch.int32, device=device)
    d_pres = torch.full((n + extra,), -1, dtype=torch.int64, device=device) if present else None
    d_rp = torch.full((n + extra,), -1, dtype=torch.int32, device=device) if rest else None
    d_rl = torch.full((n + extra,), -1, dtype=torch.int32, device=device) if rest else None
    res = torch.full((4 + extra,), -1, dtype=torch.int64, device=device)
    d_rep = None
    if replies is not None:
        d_rep = torch.full(((n + extra) * 64,), 0xA5, dtype=torch.uint8, device=device)
        if n:
            rp = np.ascontiguousarray(replies, L.MSG_DTYPE)
            d_rep[:n * 64] = torch.from_numpy(rp.view(np.uint8).reshape(-1).copy()).to(device)
    codec.xdr_unpack(d_wire, wlen, d_msgs, d_st, n, fields, cols, xstat, res, flags=flags, rec_start=d_rs,
                     head_len=head_len, present=d_pres, rest_pos=d_rp, rest_len=d_rl, replies=d_rep,
                     cols_cap=cols_cap)
    codec.sync()

    def words(t, dt):
        return None if t is None else t.cpu().numpy().view(dt).copy()
    raw = {"cols": cols.cpu().numpy().copy(), "xstat": words(xstat, np.uint32), "present": words(d_pres, np.uint64),
           "rest_pos": words(d_rp, np.uint32), "rest_len": words(d_rl, np.uint32), "result": words(res, np.uint64),
           "replies": None if d_rep is None else d_rep.cpu().numpy().copy()}
    return {"cols": raw["cols"][:cols_cap], "xstat": raw["xstat"][:n],
            "present": None if d_pres is None else raw["present"][:n],
            "rest_pos": None if d_rp is None else raw["rest_pos"][:n],
            "rest_len": None if d_rl is None else raw["rest_len"][:n],
            "replies": None if d_rep is None else raw["replies"][:n * 64].view(L.MSG_DTYPE),
            "result": raw["result"][:4], "raw": raw}


MATCH_TILE = 1024           # ONC_MATCH_TILE: records / entries per workgroup of onc_match_replies' kernels
MATCH_UNKNOWN, MATCH_DUPLICATE, MATCH_NOT_REPLY, MATCH_FAILED = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
MATCH_NONE, MATCH_MAX = 0xFFFFFFFF, 0xFFFFFFF0


def pending_calls(rows):
    """(conn, xid, tag) rows -> an L.PENDING_DTYPE array, as given."""
    t = np.zeros(len(rows), L.PENDING_DTYPE)
    for i, row in enumerate(rows):
        t[i] = tuple(row)
    return t


def match_replies_host(codec: Codec, msgs, status, rec_conn, pending, tag_out=True, still=True, extra=4,
                       device="cuda"):
    """Convenience: host descriptors (L.MSG_DTYPE), statuses, the records'
    connections (or None) and a pending list (L.PENDING_DTYPE) ->
    onc_match_replies -> a dict of host arrays: match[n], hit[np], result[6],
    tag_out[n] (None when not asked for), still[k] (k = result[5]; None when
    not asked for), and `raw`: the whole output arrays with `extra` elements
    behind them, pre-filled with sentinels (0xA5 bytes), so that a caller can
    see what was left alone."""
    torch = _torch()
    m = np.ascontiguousarray(msgs, L.MSG_DTYPE)
    pd = np.ascontiguousarray(pending, L.PENDING_DTYPE)
    n, npend = len(m), len(pd)
    d_msgs = to_device(m, device)
    d_st = _dev_words(status, np.int32, np.int32, device)
    d_conn = None if rec_conn is None else _dev_words(rec_conn, np.uint32, np.int32, device)
    d_pend = to_device(pd, device)
    fill = lambda count, width: torch.full(((count + extra) * width,), 0xA5, dtype=torch.uint8, device=device)
    match, hit, res = fill(n, 4), fill(npend, 4), fill(6, 8)
    d_tag = fill(n, 8) if tag_out else None
    d_still = fill(npend, 16) if still else None
    codec.match_replies(d_msgs, d_st, d_conn, n, d_pend, npend, match, hit, res, tag_out=d_tag, still=d_still)
    codec.sync()
    raw = {"match": match.cpu().numpy().view(np.uint32).copy(), "hit": hit.cpu().numpy().view(np.uint32).copy(),
           "result": res.cpu().numpy().view(np.uint64).copy(),
           "tag_out": None if d_tag is None else d_tag.cpu().numpy().view(np.uint64).copy(),
           "still": None if d_still is None else d_still.cpu().numpy().view(L.PENDING_DTYPE).copy()}
    k = int(raw["result"][5])
    return {"match": raw["match"][:n], "hit": raw["hit"][:npend], "result": raw["result"][:6],
            "tag_out": None if d_tag is None else raw["tag_out"][:n],
            "still": None if d_still is None else raw["still"][:min(k, npend)], "raw": raw}


GROUP_TILE = 1024           # ONC_GROUP_TILE: items per workgroup of onc_group_by_conn's kernels
GROUP_CONN_MAX = 0x00FFFFFF


def group_by_conn_host(codec: Codec, rec_conn, via, nconn, msgs=None, n=None, extra=4, device="cuda"):
    """Convenience: the connections (uint32), an optional `via` (uint32; None:
    item k is rec_conn[k]) and optional host descriptors (L.MSG_DTYPE, one per
    item) -> onc_group_by_conn -> a dict of host arrays: order[n],
    conn_first[nconn + 2], result[3], msgs_out[n] (None without msgs), and
    `raw`: the whole output arrays with `extra` elements behind them,
    pre-filled with sentinels (0xA5 bytes), so that a caller can see what was
    left alone. rec_conn is uploaded with `extra` words of connection 0 behind
    it: an item whose index is outside rec_conn and is read all the same lands
    in group 0 instead of the dropped group."""
    torch = _torch()
    rc = np.ascontiguousarray(rec_conn, np.uint32)
    nsrc = len(rc)
    if n is None:
        n = nsrc if via is None else len(via)
    d_conn = _dev_words(rc, np.uint32, np.int32, device, extra=extra)
    d_via = None if via is None else _dev_words(via, np.uint32, np.int32, device)
    d_msgs = None if msgs is None else to_device(np.ascontiguousarray(msgs, L.MSG_DTYPE), device)
    fill = lambda count, width: torch.full(((count + extra) * width,), 0xA5, dtype=torch.uint8, device=device)
    order, conn_first, res = fill(n, 4), fill(nconn + 2, 8), fill(3, 8)
    d_out = None if msgs is None else fill(n, 64)
    codec.group_by_conn(d_conn, nsrc, d_via, n, nconn, order, conn_first, res, msgs=d_msgs, msgs_out=d_out)
    codec.sync()
    raw = {"order": order.cpu().numpy().view(np.uint32).copy(),
           "conn_first": conn_first.cpu().numpy().view(np.uint64).copy(),
           "result": res.cpu().numpy().view(np.uint64).copy(),
           "msgs_out": None if d_out is None else d_out.cpu().numpy().copy()}
    return {"order": raw["order"][:n], "conn_first": raw["conn_first"][:nconn + 2], "result": raw["result"][:3],
            "msgs_out": None if d_out is None else raw["msgs_out"][:n * 64].view(L.MSG_DTYPE), "raw": raw}


def conn_extents_host(codec: Codec, rec_off, conn_first, nconn, nrec=None, extra=4, device="cuda"):
    """Convenience: host offsets (nrec + 1; nrec None: all but the last entry
    of rec_off) and conn_first (nconn + 2) -> onc_conn_extents -> (conn_off[
    nconn + 2], raw): raw is the whole output with `extra` words of 0xA5 bytes
    behind it. rec_off is uploaded with `extra` words of 2^63 behind it, which
    no offset equals."""
    torch = _torch()
    ro = np.ascontiguousarray(rec_off, np.uint64)
    if nrec is None:
        nrec = len(ro) - 1
    d_ro = torch.from_numpy(np.append(ro, np.full(extra, 1 << 63, np.uint64)).view(np.int64).copy()).to(device)
    d_cf = _dev_words(conn_first, np.uint64, np.int64, device)
    conn_off = torch.full(((nconn + 2 + extra) * 8,), 0xA5, dtype=torch.uint8, device=device)
    codec.conn_extents(d_ro, nrec, d_cf, nconn, conn_off)
    codec.sync()
    raw = conn_off.cpu().numpy().view(np.uint64).copy()
    return raw[:nconn + 2], raw


def place_payloads_host(codec: Codec, wire, frag_start, frag_len, rec_frag, frag_pre, rec_len, pay_pos, pay_len,
                        slot_off, dst_cap, shift=0, fill=0xA5, guard=64, device="cuda"):
    """Convenience: a host wire, its fragment extents, onc_defragment_heads'
    rec_frag / frag_pre / rec_len (rec_frag = frag_pre = None: the identity
    form) and the slices -> onc_place_payloads into a destination `shift`
    bytes past a 16-byte boundary -> the `guard` bytes before dst, its dst_cap
    bytes and the `guard` bytes behind them as one host array, `fill` where
    nothing was written."""
    torch = _torch()
    n = len(pay_len)
    w = to_device(np.frombuffer(bytes(wire) + b"\0" * 16, np.uint8), device)
    d_fs = _dev_words(frag_start, np.uint64, np.int64, device)
    d_fl = _dev_words(frag_len, np.uint32, np.int32, device)
    d_rf = None if rec_frag is None else _dev_words(rec_frag, np.uint64, np.int64, device)
    d_fp = None if frag_pre is None else _dev_words(frag_pre, np.uint64, np.int64, device)
    d_rl = _dev_words(rec_len, np.uint32, np.int32, device)
    d_pp = _dev_words(pay_pos, np.uint32, np.int32, device)
    d_pl = _dev_words(pay_len, np.uint32, np.int32, device)
    d_so = _dev_words(slot_off, np.uint64, np.int64, device)
    assert guard % 16 == 0 and 0 <= shift < 16
    base, lo = aligned_bytes(guard + dst_cap + guard + 16, fill, device)
    at = lo + guard + shift
    codec.place_payloads(w, d_fs, d_fl, len(frag_start), d_rf, d_fp, d_rl, d_pp, d_pl, d_so, n, base.data_ptr() + at,
                         dst_cap=dst_cap)
    codec.sync()
    return base.cpu().numpy()[at - guard:at + dst_cap + guard].copy()


def reassemble_host_stream(codec: Codec, buf: bytes, device="cuda"):
    """Convenience: host bytes of a stream of (possibly multi-fragment)
    records -> onc_frame_fragments + onc_defragment -> (reassembled bytes,
    rec_off[n+1], status[n], result[6], framing (n_frags, consumed, status,
    aux0, aux1)), all on the host. The reassembled bytes are a packed stream
    of single-fragment records: frame_host_stream / decode_host_wire take
    them as they are."""
    torch = _torch()
    w = to_device(np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8), device)
    m = len(buf) // 4 + 1
    frag_off = torch.zeros(m + 1, dtype=torch.int64, device=device)
    fres = torch.zeros(5, dtype=torch.int64, device=device)
    codec.frame_fragments(w, len(buf), frag_off, m, fres)
    codec.sync()
    fr = fres.cpu().numpy()
    nfrag = int(fr[0])
    # a reassembled record is never longer than its fragments
    out = torch.zeros(max(16, (int(fr[1]) + 15) // 16 * 16), dtype=torch.uint8, device=device)
    rec_off = torch.zeros(nfrag + 1, dtype=torch.int64, device=device)
    status = torch.zeros(max(nfrag, 1), dtype=torch.int32, device=device)
    res = torch.zeros(6, dtype=torch.int64, device=device)
    codec.defragment(w, frag_off, nfrag, out, rec_off, status, res)
    codec.sync()
    r = res.cpu().numpy().view(np.uint64).copy()
    n = int(r[0])
    return (out.cpu().numpy()[:int(r[2])].tobytes(), rec_off.cpu().numpy().view(np.uint64)[:n + 1].copy(),
            status.cpu().numpy()[:n].copy(), r,
            (nfrag, int(fr[1]), int(fr[2]), int(np.uint32(fr[3])), int(np.uint32(fr[4]))))


def fragment_host(codec: Codec, wire_bytes, rec_off, max_frag, out_cap=None, shift=0, device="cuda"):
    """Convenience: host bytes of a packed stream and its offsets ->
    onc_fragment -> (the out_cap bytes from `out` on (out_cap None: the bytes
    the batch needs), out_off[n+1], status[n], result[3]) on the host. `out`
    starts `shift` bytes past a 16-byte aligned address and is zero-filled
    before the call."""
    torch = _torch()
    ro = np.ascontiguousarray(rec_off, np.uint64)
    n = len(ro) - 1
    w = to_device(np.frombuffer(bytes(wire_bytes) + b"\0" * 16, np.uint8), device)
    d_ro = torch.from_numpy(ro.view(np.int64).copy()).to(device)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=device)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
    res = torch.zeros(3, dtype=torch.int64, device=device)
    cap = out_cap
    if cap is None:                      # plan only: out_off[n] is what the batch needs
        codec.fragment(w, d_ro, n, max_frag, 0, out_off, status, res, out_cap=0)
        codec.sync()
        cap = int(res.cpu().numpy().view(np.uint64)[1])
    base = torch.zeros(16 + shift + cap + 16, dtype=torch.uint8, device=device)
    lo = (-base.data_ptr()) % 16 + shift
    codec.fragment(w, d_ro, n, max_frag, base.data_ptr() + lo, out_off, status, res, out_cap=cap)
    codec.sync()
    return (base.cpu().numpy()[lo:lo + cap].tobytes(), out_off.cpu().numpy().view(np.uint64).copy(),
            status.cpu().numpy()[:n].copy(), res.cpu().numpy().view(np.uint64).copy())


def fragment_iov_host(codec: Codec, iov, max_frag, rec_max_frag=None, marks_cap=None, max_pieces=None, device="cuda"):
    """Convenience: a host array of onc_iov_rec (layout.IOV_DTYPE) ->
    onc_fragment_iov -> (marks uint8[marks_cap], pieces
    FRAG_PIECE_DTYPE[max_pieces], out_off[n+1], piece_off[n+1], status[n],
    result[4]) on the host. A capacity left None is what the batch needs (a
    plan-only call with both capacities 0 finds it); both buffers are
    zero-filled before the call."""
    torch = _torch()
    e = np.ascontiguousarray(iov, L.IOV_DTYPE)
    n = len(e)
    d_iov = to_device(e, device)
    d_lim = None
    if rec_max_frag is not None:
        d_lim = torch.from_numpy(np.append(np.asarray(rec_max_frag, np.uint32), np.uint32(0)).view(np.int32).copy()
                                 ).to(device)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=device)
    piece_off = torch.zeros(n + 1, dtype=torch.int64, device=device)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
    res = torch.zeros(4, dtype=torch.int64, device=device)
    if marks_cap is None or max_pieces is None:
        codec.fragment_iov(d_iov, n, max_frag, None, None, out_off, piece_off, status, res, rec_max_frag=d_lim)
        codec.sync()
        r = res.cpu().numpy().view(np.uint64)
        marks_cap = 4 * int(r[0]) if marks_cap is None else marks_cap
        max_pieces = int(r[3]) if max_pieces is None else max_pieces
    marks = torch.zeros(marks_cap + 16, dtype=torch.uint8, device=device)
    pieces = torch.zeros(16 * max_pieces + 16, dtype=torch.uint8, device=device)
    codec.fragment_iov(d_iov, n, max_frag, marks, pieces, out_off, piece_off, status, res, rec_max_frag=d_lim,
                       marks_cap=marks_cap, max_pieces=max_pieces)
    codec.sync()
    return (marks.cpu().numpy()[:marks_cap].copy(),
            pieces.cpu().numpy()[:16 * max_pieces].view(L.FRAG_PIECE_DTYPE).copy(),
            out_off.cpu().numpy().view(np.uint64).copy(), piece_off.cpu().numpy().view(np.uint64).copy(),
            status.cpu().numpy()[:n].copy(), res.cpu().numpy().view(np.uint64).copy())


def gather_src(*sources):
    """onc_gather_src of up to three sources, in ONC_PIECE_* order: each a
    uint8 tensor (its length is the tensor's), a (tensor or int device
    pointer, length) pair, or None (NULL, length 0)."""
    src = OncGatherSrc()
    for k, s in enumerate(sources):
        ln = None
        if isinstance(s, tuple):
            s, ln = s
        if s is None:
            continue
        src.base[k] = s if isinstance(s, int) else s.data_ptr()
        src.len[k] = s.numel() if ln is None else ln
    return src


def gather_pieces(pieces, marks, hdr, payload_arena):
    """The byte stream a writev() of `pieces` sends: every piece's slice of
    its source (host arrays: onc_fragment_iov's marks, onc_encode_iov's
    hdr_out, the batch's payload arena), in order."""
    ln = pieces["len"].astype(np.int64)
    at = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln) + np.repeat(pieces["off"].astype(np.int64), ln)
    which = np.repeat(pieces["src"], ln)
    out = np.empty(len(at), np.uint8)
    for s, a in enumerate((marks, hdr, payload_arena)):
        m = which == s
        if m.any():
            out[m] = np.asarray(a, np.uint8)[at[m]]
    return out.tobytes()


def codec_lengths(codec: Codec, db: DeviceBatch):
    torch = _torch()
    n = db.n
    rec_len = torch.empty(max(n, 1), dtype=torch.int32, device=db.msgs.device)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=db.msgs.device)
    if n:
        codec.encode_lengths(db, rec_len, status)
        codec.sync()
    return rec_len.cpu().numpy().view(np.uint32)[:n].astype(np.uint64)


def decode_host_wire(codec: Codec, wire: np.ndarray, rec_off: np.ndarray, mode, device="cuda"):
    """Convenience: packed wire + offsets (host) -> GPU decode -> host arrays."""
    torch = _torch()
    n = len(rec_off) - 1
    w = to_device(wire, device)
    off = torch.from_numpy(rec_off.astype(np.uint64).view(np.int64).copy()).to(device)
    bufs = DecodeBuffers(n, device)
    codec.decode(w, off, n, mode, bufs.msgs, bufs.unix, bufs.status, bufs.aux0, bufs.aux1)
    codec.sync()
    return bufs.to_host()


def encode_body_host_batch(codec: Codec, root, hb: L.HostBatch, device="cuda", out_cap=None):
    """Convenience: host batch -> GPU onc_encode_body -> (wire bytes, rec_off, status, rec_len) on host."""
    torch = _torch()
    db = DeviceBatch.from_host(hb, device)
    n = hb.n
    rec_len = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    if n:
        codec.encode_body_lengths(root, db, rec_len, status)
        codec.sync()
    total = int(rec_len.cpu().numpy().view(np.uint32)[:n].astype(np.uint64).sum())
    cap = total if out_cap is None else out_cap
    out = torch.zeros(max(16, (cap + 15) // 16 * 16), dtype=torch.uint8, device=device)
    rec_off = torch.empty(n + 1, dtype=torch.int64, device=device)
    codec.encode_body(root, db, out, rec_off, status, rec_len, out_cap=cap)
    codec.sync()
    return (out.cpu().numpy()[:min(total, cap)].tobytes(), rec_off.cpu().numpy().view(np.uint64).copy(),
            status.cpu().numpy()[:n].copy(), rec_len.cpu().numpy().view(np.uint32)[:n].copy())


def decode_body_host_wire(codec: Codec, root, wire: np.ndarray, rec_off: np.ndarray, mode, param=None, device="cuda"):
    """Convenience: packed records + offsets (host) -> GPU onc_decode_body ->
    (msgs, unix, status, aux0, aux1, consumed) on host."""
    torch = _torch()
    n = len(rec_off) - 1
    w = to_device(wire, device)
    off = torch.from_numpy(rec_off.astype(np.uint64).view(np.int64).copy()).to(device)
    bufs = DecodeBuffers(n, device)
    prm = None if param is None else torch.from_numpy(np.asarray(param, np.uint32).view(np.int32).copy()).to(device)
    consumed = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    codec.decode_body(root, w, off, n, mode, bufs.msgs, bufs.unix, bufs.status, bufs.aux0, bufs.aux1,
                      param=prm, consumed=consumed)
    codec.sync()
    return bufs.to_host() + (consumed.cpu().numpy().view(np.uint32)[:n].copy(),)
