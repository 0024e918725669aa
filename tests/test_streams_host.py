"""CPU tests of onc_frame_streams and onc_decode_extents: the symbols, the
header's promises (ABI 8, sixteen timing ids, both functions declared and
documented) and the argument checks that are made before any GPU call."""
import ctypes as C
import os
import re

import onc_rpc_amd.layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL = -1
NAMES = ("onc_frame_streams", "onc_decode_extents")


def test_symbols_exported_and_bound():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    raw = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in R.EXPORTED
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.onc_frame_streams.argtypes) == 11 and len(lib.onc_decode_extents.argtypes) == 8
    for meth in ("frame_streams", "decode_extents"):
        assert callable(getattr(R.Codec, meth))
    assert callable(R.frame_host_streams) and callable(R.decode_host_extents)


def test_header_keeps_abi_and_timing_ids():
    import onc_rpc_amd.runtime as R
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and R.load_library().onc_abi_version() == 8
    assert re.search(r"#define ONC_K_COUNT\s+16\b", hdr) and R.K_COUNT == 16
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int %s\(onc_codec\* codec," % name, code, flags=re.M), name
    # the ids the new launches report under are written down next to the id list
    ids = hdr[hdr.index("Per-kernel event timing"):hdr.index("#define ONC_K_ENC_LEN")]
    for word in ("onc_frame_streams", "onc_decode_extents", "ONC_K_FRAME,", "ONC_K_FRAME_WRITE", "ONC_K_LEN_TILES",
                 "ONC_K_DEC_PARSE"):
        assert word in ids, word
    # the serial loop is in the header
    assert "seg_result[6s ..] = {first, k - first, p, st, aux0, aux1}" in hdr


def test_argument_checks_before_any_gpu_call():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    out = R.OncDecoded(8, 8, 8, 8, 8)
    nul = R.OncDecoded(0, 0, 0, 0, 0)
    fake = C.c_void_p(8)                             # never dereferenced: the checks below come first
    p = C.c_void_p(16)                               # a non-NULL array, never dereferenced either
    fs, de = lib.onc_frame_streams, lib.onc_decode_extents
    # onc_frame_streams: NULL codec, NULL result, NULL segment arrays / rows / record arrays with counts
    assert fs(None, p, p, p, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, p, p, p, 1, p, None) == RC_EINVAL
    assert fs(fake, p, None, p, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, None, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, p, p, p, 1, None, p) == RC_EINVAL
    assert fs(fake, None, p, p, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, None, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, p, None, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1 << 32, p, p, p, 1, p, p) == RC_EINVAL      # rec_seg is 32 bits wide
    # onc_decode_extents: as its siblings
    assert de(None, p, 0, p, p, 1, L.DECODE_SLICE, C.byref(out)) == RC_EINVAL
    assert de(fake, p, 0, p, p, 1, L.DECODE_SLICE, None) == RC_EINVAL
    assert de(fake, p, 0, p, p, 1, 7, C.byref(out)) == RC_EINVAL
    assert de(fake, p, 0, p, p, 0, 7, C.byref(out)) == RC_EINVAL          # a bad mode even with n = 0
    assert de(fake, p, 0, None, p, 1, L.DECODE_BYTES, C.byref(out)) == RC_EINVAL
    assert de(fake, p, 0, p, None, 1, L.DECODE_BYTES, C.byref(out)) == RC_EINVAL
    assert de(fake, p, 0, p, p, 1, L.DECODE_BYTES, C.byref(nul)) == RC_EINVAL
    assert de(fake, None, 0, None, None, 0, L.DECODE_SLICE, C.byref(nul)) == 0   # n = 0: nothing to do
