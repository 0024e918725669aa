"""CPU tests of onc_payload_slots / onc_place_payloads (decoded payloads
placed in aligned slots on the device): the symbols and their argument checks,
and the arithmetic the kernels call (onc-rpc_amd/csrc/payload_plan.h) in a
stand-alone host program — which slices may be copied at the mark, at a
record's end and near 2^32, which slots fit near 2^64, round_up at every
alignment, and the slots' scan at every blocking of a short list."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4


def test_payload_symbols_and_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbols by linking
    assert R.K_COUNT == 16 and len(R.K_NAMES) == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    raw = C.CDLL(LIB)
    for name in ("onc_payload_slots", "onc_place_payloads"):
        assert hasattr(raw, name) and name in R.EXPORTED and name in hdr
    assert hasattr(R.Codec, "payload_slots") and hasattr(R.Codec, "place_payloads")
    assert hasattr(R, "payload_slots_host") and hasattr(R, "place_payloads_host")
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p = C.c_void_p(64)
    ps, pl = lib.onc_payload_slots, lib.onc_place_payloads

    # -- onc_payload_slots(codec, msgs, status, n, head_len, rec_start, align, pay_pos, pay_len, slot_off, msgs_out, result)
    def slots(codec=fake, msgs=p, status=p, n=1, head_len=160, rec_start=None, align=16, pay_pos=p, pay_len=p,
              slot_off=p, msgs_out=None, result=p):
        return ps(codec, msgs, status, n, head_len, rec_start, align, pay_pos, pay_len, slot_off, msgs_out, result)

    for n in (0, 1):
        # NULL codec, result or slot_off, whatever n is
        assert slots(codec=None, n=n) == RC_EINVAL
        assert slots(result=None, n=n) == RC_EINVAL
        assert slots(slot_off=None, n=n) == RC_EINVAL
        # align: a power of two in [1, 2^20]
        for align in (0, 3, 24, (1 << 20) + 1, 1 << 21, 1 << 31, 0xFFFFFFFF):
            assert slots(align=align, n=n) == RC_EINVAL
            assert slots(align=align, n=n, rec_start=p) == RC_EINVAL
        # the heads form: head_len a multiple of 16 in [64, 4096]; ignored with rec_start
        for head_len in (0, 48, 63, 72, 4097, 4112, 1 << 20):
            assert slots(head_len=head_len, n=n) == RC_EINVAL
            assert slots(head_len=head_len, n=n, rec_start=p, slot_off=C.c_void_p(4)) == RC_EALIGN   # got past it
    # with records: NULL msgs, status, pay_pos or pay_len
    for k in ("msgs", "status", "pay_pos", "pay_len"):
        assert slots(**{k: None}) == RC_EINVAL
        assert slots(**{k: None}, rec_start=p) == RC_EINVAL
    # alignment: msgs and msgs_out 16 bytes, slot_off 8
    for a in (8, 24, 36, 17):
        assert slots(msgs=C.c_void_p(a)) == RC_EALIGN
        assert slots(msgs_out=C.c_void_p(a)) == RC_EALIGN
        assert slots(msgs=C.c_void_p(a), n=0) == RC_EALIGN
    for a in (4, 12, 17, 20):
        assert slots(slot_off=C.c_void_p(a)) == RC_EALIGN
        assert slots(slot_off=C.c_void_p(a), n=0) == RC_EALIGN
    # the pointer checks come before the alignment checks
    assert slots(msgs=C.c_void_p(8), result=None) == RC_EINVAL
    assert slots(msgs=C.c_void_p(8), pay_len=None) == RC_EINVAL
    assert slots(slot_off=C.c_void_p(4), status=None) == RC_EINVAL
    assert slots(msgs_out=C.c_void_p(8), align=3) == RC_EINVAL

    # -- onc_place_payloads(codec, wire, frag_start, frag_len, nfrag, rec_frag, frag_pre, rec_len, pay_pos, pay_len,
    #                       slot_off, n, dst, dst_cap)
    names = ("wire", "frag_start", "frag_len", "rec_len", "pay_pos", "pay_len", "slot_off", "dst")

    def place(codec=fake, nfrag=4, rec_frag=p, frag_pre=p, n=1, dst_cap=64, **kw):
        a = {k: kw.get(k, p) for k in names}
        return pl(codec, a["wire"], a["frag_start"], a["frag_len"], nfrag, rec_frag, frag_pre, a["rec_len"],
                  a["pay_pos"], a["pay_len"], a["slot_off"], n, a["dst"], dst_cap)

    for n in (0, 1):
        assert place(codec=None, n=n) == RC_EINVAL
        assert place(codec=None, n=n, rec_frag=None, frag_pre=None) == RC_EINVAL
        # one of rec_frag / frag_pre without the other
        assert place(rec_frag=None, n=n) == RC_EINVAL
        assert place(frag_pre=None, n=n) == RC_EINVAL
    for k in names:
        assert place(**{k: None}) == RC_EINVAL
        assert place(**{k: None}, rec_frag=None, frag_pre=None) == RC_EINVAL
    # the identity form: record r is fragment r
    assert place(rec_frag=None, frag_pre=None, nfrag=0, n=1) == RC_EINVAL
    assert place(rec_frag=None, frag_pre=None, nfrag=6, n=7) == RC_EINVAL


def test_no_records():
    """n == 0 needs no arrays. With a GPU: slot_off[0] = 0, a zero result and
    a placement that writes nothing. Without one no handle can be made, and a
    NULL one is refused first: the calls get past every other argument
    check."""
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    h = C.c_void_p()
    if lib.onc_codec_create(C.byref(h), 0, None) == 0:          # a GPU is here: the real thing
        import torch
        off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
        op, rp, dp = (C.c_void_p(t.data_ptr()) for t in (off, res, out))
        assert lib.onc_payload_slots(h, None, None, 0, 160, None, 16, None, None, op, None, rp) == 0
        assert lib.onc_payload_slots(h, None, None, 0, 0, op, 1, None, None, op, None, rp) == 0
        assert lib.onc_place_payloads(h, None, None, None, 0, None, None, None, None, None, None, 0, dp, 64) == 0
        assert lib.onc_place_payloads(h, None, None, None, 0, None, None, None, None, None, None, 0, None, 0) == 0
        lib.onc_codec_sync(h)
        assert off.tolist() == [0, -1] and res.tolist() == [0, 0, 0, -1]
        assert (out == 0xA5).all().item()
        lib.onc_codec_destroy(h)
    else:
        p = C.c_void_p(16)
        assert lib.onc_payload_slots(None, None, None, 0, 160, None, 16, None, None, p, None, p) == RC_EINVAL
        assert lib.onc_place_payloads(None, None, None, None, 0, None, None, None, None, None, None, 0, None,
                                      0) == RC_EINVAL


def test_plan_arithmetic_extremes():
    """payload_plan.h compiled by the host compiler into a stand-alone program
    (tests/cpp_payload/plan_probe.cpp), with the undefined-behaviour sanitizer
    where the toolchain links it: ok() at pay_pos = 3 and 4, at pay_pos =
    rec_len with pay_len 0 and 1, at pay_pos + pay_len wrapping 2^32, at
    slot_off = dst_cap with pay_len 0 and 1 and at slot_off + pay_len wrapping
    2^64; round_up at every power of two up to 2^20; the scan at every
    blocking of a short list."""
    src = os.path.join(ROOT, "tests", "cpp_payload", "plan_probe.cpp")
    inc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plan_probe")
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o", exe]
        san = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"],
                             capture_output=True, text=True)
        if san.returncode != 0:                      # no sanitizer runtime here: the plain build
            subprocess.run(base, check=True, capture_output=True, text=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "payload plan ok"


def test_cpp_mirror_program_compiles():
    """FragmentedHeads::place_payloads and PlacedPayloads (include/onc_rpc.hpp)
    build against the C ABI (build() compiles tests/cpp_payload)."""
    exe = os.path.join(ROOT, "tests", "cpp_payload", "test_payload")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
    assert "onc_place_payloads" in hpp and "onc_payload_slots" in hpp and "place_payloads" in hpp
