"""CPU tests of onc_frame_fragment_streams and onc_defragment_extents: the
symbols, the header's promises (ABI 8, sixteen timing ids, both functions
declared and documented, the serial loop written down) and the argument
checks that are made before any GPU call."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL = -1
NAMES = ("onc_frame_fragment_streams", "onc_defragment_extents")


def test_symbols_exported_and_bound():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    raw = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in R.EXPORTED
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.onc_frame_fragment_streams.argtypes) == 11 and len(lib.onc_defragment_extents.argtypes) == 10
    for meth in ("frame_fragment_streams", "defragment_extents"):
        assert callable(getattr(R.Codec, meth))
    for fn in ("frame_host_fragment_streams", "defragment_host_extents", "reassemble_host_streams"):
        assert callable(getattr(R, fn))


def test_header_keeps_abi_and_timing_ids():
    import onc_rpc_amd.runtime as R
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and R.load_library().onc_abi_version() == 8
    assert re.search(r"#define ONC_K_COUNT\s+16\b", hdr) and R.K_COUNT == 16 == len(R.K_NAMES)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int %s\(onc_codec\* codec," % name, code, flags=re.M), name
    # the ids the new launches report under are written down next to the id list
    ids = hdr[hdr.index("Per-kernel event timing"):hdr.index("#define ONC_K_ENC_LEN")]
    for word in NAMES + ("fragstreams_chase", "fragstreams_write", "fragstreams_result"):
        assert word in ids, word
    # the serial loop is in the header
    assert ("seg_result[8s ..] = {first, k - first, consumed, cut ? ONC_OK : st, cut ? 0 : aux0, cut ? 0 : aux1, "
            "first_rec, r - first_rec}") in hdr
    assert "result = {k, needed, r, stopped}" in hdr
    assert "seg_result[8s ..] = {max_frags, 0, 0, ONC_OK, 0, 0, 0, 0}" in hdr


def test_argument_checks_before_any_gpu_call():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    fake = C.c_void_p(8)                             # never dereferenced: the checks below come first
    p = C.c_void_p(16)                               # a non-NULL array, never dereferenced either
    fs, de = lib.onc_frame_fragment_streams, lib.onc_defragment_extents
    # onc_frame_fragment_streams: NULL codec, NULL result, NULL segment arrays / rows / fragment arrays with counts
    assert fs(None, p, p, p, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, p, p, p, 1, p, None) == RC_EINVAL
    assert fs(fake, p, p, p, 0, p, p, p, 1, p, None) == RC_EINVAL
    assert fs(fake, p, None, p, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, None, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, p, p, p, 1, None, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, p, p, p, 0, None, p) == RC_EINVAL         # rows are written with max_frags 0 too
    assert fs(fake, None, p, p, 1, p, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, None, p, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1, p, None, p, 1, p, p) == RC_EINVAL
    assert fs(fake, p, p, p, 1 << 32, p, p, p, 1, p, p) == RC_EINVAL      # frag_seg is 32 bits wide
    # onc_defragment_extents: NULL codec, rec_off or result whatever nfrag is
    assert de(None, p, p, p, 1, p, 64, p, p, p) == RC_EINVAL
    assert de(fake, p, p, p, 1, p, 64, None, p, p) == RC_EINVAL
    assert de(fake, p, p, p, 1, p, 64, p, p, None) == RC_EINVAL
    assert de(fake, p, p, p, 0, p, 64, None, p, p) == RC_EINVAL
    assert de(fake, p, p, p, 0, p, 64, p, p, None) == RC_EINVAL
    # with fragments: NULL wire, frag_start, frag_len, status, or out with a capacity
    assert de(fake, None, p, p, 1, p, 64, p, p, p) == RC_EINVAL
    assert de(fake, p, None, p, 1, p, 64, p, p, p) == RC_EINVAL
    assert de(fake, p, p, None, 1, p, 64, p, p, p) == RC_EINVAL
    assert de(fake, p, p, p, 1, p, 64, p, None, p) == RC_EINVAL
    assert de(fake, p, p, p, 1, None, 64, p, p, p) == RC_EINVAL


def test_nfrag_zero_is_accepted_by_the_argument_checks():
    """nfrag == 0 needs no wire, extents, status or out: the call gets past
    its argument checks and returns 0 (on a machine without a GPU no handle
    can be made, and a NULL one is refused first)."""
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    h = C.c_void_p()
    if lib.onc_codec_create(C.byref(h), 0, None) == 0:
        import torch
        rec_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        assert lib.onc_defragment_extents(h, None, None, None, 0, None, 0, C.c_void_p(rec_off.data_ptr()), None,
                                          C.c_void_p(res.data_ptr())) == 0
        lib.onc_codec_sync(h)
        assert rec_off.item() == 0 and not res.cpu().numpy().any()
        lib.onc_codec_destroy(h)
    else:
        assert lib.onc_defragment_extents(None, None, None, None, 0, None, 0, C.c_void_p(16), None,
                                          C.c_void_p(16)) == RC_EINVAL


def test_cpp_mirror_program_compiles():
    """reassemble_streams and BatchDecoder's mixed flow (include/onc_rpc.hpp)
    build against the C ABI (build() compiles tests/cpp_fragment_streams)."""
    exe = os.path.join(ROOT, "tests", "cpp_fragment_streams", "test_fragment_streams")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
