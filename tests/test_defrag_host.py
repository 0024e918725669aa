"""CPU tests of multi-fragment reassembly (onc_frame_fragments,
onc_defragment): the symbols and their argument checks, the timing ids, and
the record arithmetic the kernels call (onc-rpc_amd/csrc/defrag_plan.h) at the
extremes of its 64-bit arguments — a record of 2^31 body bytes would need a
2 GiB wire on the GPU, so that status is checked here, in a stand-alone host
program."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL = -1


def test_fragment_symbols_and_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8               # additive: callers find the symbols by linking
    for name in ("onc_frame_fragments", "onc_defragment"):
        assert hasattr(C.CDLL(LIB), name), name
        assert name in R.EXPORTED
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p = C.c_void_p(16)
    # onc_frame_fragments: NULL codec, offsets, result, or wire with a length — as onc_frame_stream
    assert lib.onc_frame_fragments(None, p, 8, p, 4, p) == RC_EINVAL
    assert lib.onc_frame_fragments(fake, p, 8, None, 4, p) == RC_EINVAL
    assert lib.onc_frame_fragments(fake, p, 8, p, 4, None) == RC_EINVAL
    assert lib.onc_frame_fragments(fake, None, 8, p, 4, p) == RC_EINVAL
    assert lib.onc_frame_stream(fake, p, 8, None, 4, p) == RC_EINVAL
    # onc_defragment: NULL codec, rec_off or result whatever nfrag is
    assert lib.onc_defragment(None, p, p, 1, p, 64, p, p, p) == RC_EINVAL
    assert lib.onc_defragment(fake, p, p, 1, p, 64, None, p, p) == RC_EINVAL
    assert lib.onc_defragment(fake, p, p, 1, p, 64, p, p, None) == RC_EINVAL
    assert lib.onc_defragment(fake, p, p, 0, p, 64, None, p, p) == RC_EINVAL
    assert lib.onc_defragment(fake, p, p, 0, p, 64, p, p, None) == RC_EINVAL
    # with fragments: NULL wire, offsets, status, or out with a capacity
    assert lib.onc_defragment(fake, None, p, 1, p, 64, p, p, p) == RC_EINVAL
    assert lib.onc_defragment(fake, p, None, 1, p, 64, p, p, p) == RC_EINVAL
    assert lib.onc_defragment(fake, p, p, 1, p, 64, p, None, p) == RC_EINVAL
    assert lib.onc_defragment(fake, p, p, 1, None, 64, p, p, p) == RC_EINVAL


def test_nfrag_zero_is_accepted_by_the_argument_checks():
    """nfrag == 0 needs no wire, offsets, status or out: the call gets past
    its argument checks (on a machine without a GPU it then fails selecting
    the device, which is not EINVAL)."""
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    h = C.c_void_p()
    if lib.onc_codec_create(C.byref(h), 0, None) == 0:          # a GPU is here: the real thing
        import torch
        rec_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        assert lib.onc_defragment(h, None, None, 0, None, 0, C.c_void_p(rec_off.data_ptr()), None,
                                  C.c_void_p(res.data_ptr())) == 0
        lib.onc_codec_sync(h)
        assert rec_off.item() == 0 and not res.cpu().numpy().any()
        lib.onc_codec_destroy(h)
    else:
        # no device: a handle cannot be made, and a NULL one is refused first
        assert lib.onc_defragment(None, None, None, 0, None, 0, C.c_void_p(16), None, C.c_void_p(16)) == RC_EINVAL


def test_timing_ids():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_K_DEFRAG_PLAN  14" in hdr and "#define ONC_K_DEFRAG_COPY  15" in hdr
    assert "#define ONC_K_COUNT        16" in hdr
    assert R.K_COUNT == 16 == len(R.K_NAMES) and (R.K_DEFRAG_PLAN, R.K_DEFRAG_COPY) == (14, 15)
    for k, name in enumerate(R.K_NAMES):             # the binding's names are the library's, id by id
        assert lib.onc_kernel_name(k) == name.encode(), k
    assert lib.onc_kernel_name(16) == b"?"


def test_copy_one_group_switch():
    """ONC_VARIANT_COPY_ONE_GROUP: the header, the binding and the walk model
    agree; it is a bit of its own among the variant bits; the ABI and the
    options struct are what they were; and each of the six copy launchers
    takes its workgroup limit from copy_max_groups, which gives its kernel's
    own maximum with the bit clear."""
    import re
    import onc_rpc_amd.runtime as R
    import tile_walk_model as TW
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_VARIANT_COPY_ONE_GROUP   0x%xu" % R.VARIANT_COPY_ONE_GROUP in hdr
    bits = [int(v, 16) for v in re.findall(r"#define ONC_VARIANT_\w+\s+(0x[0-9a-fA-F]+)u", hdr)]
    assert R.VARIANT_COPY_ONE_GROUP in bits and len(set(bits)) == len(bits)
    assert all(b & (b - 1) == 0 for b in bits), "one bit each"
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and R.ABI_VERSION == 8
    assert C.sizeof(R.OncCodecOptions) == 32
    assert [f[0] for f in R.OncCodecOptions._fields_] == ["size", "flags", "decode_policy", "variant", "enc_chunk",
                                                          "frame_chunk"]
    assert TW.ONE_GROUP == 4 and TW.MAX_BLOCKS == 2048
    csrc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    kh = open(os.path.join(csrc, "kernels.h")).read()
    assert "return (variant & ONC_VARIANT_COPY_ONE_GROUP) ? 1 : max_blocks;" in kh
    for src, kernel, most in (("defrag.hip", "defrag_copy", "kDfMaxBlocks"), ("fragment.hip", "frag_copy", "kFgMaxBlocks"),
                              ("gather.hip", "gather_copy", "kGaMaxBlocks"), ("payload.hip", "place_copy", "kPlMaxBlocks"),
                              ("fragment_iov.hip", "fragiov_fill", "kFvMaxBlocks"),
                              ("defrag_heads.hip", "heads_gather", "kDhMaxBlocks")):
        text = open(os.path.join(csrc, src)).read()
        body = text[text.index(f"hipError_t launch_{kernel}("):]
        body = body[:body.index("\n}\n")]
        assert f"const uint64_t most = copy_max_groups(variant, {most});" in body, src
        assert f"ONC_LAUNCH({kernel}_kernel, dim3(uint32_t(wgs < most ? wgs : most))" in body, src
        assert f"onc::launch_{kernel}(" in open(os.path.join(csrc, "codec.hip")).read()
    assert open(os.path.join(csrc, "codec.hip")).read().count("c->stream, c->variant)") == 6


def test_plan_arithmetic_extremes():
    """defrag_plan.h compiled by the host compiler into a stand-alone program
    (tests/cpp_defrag/plan_probe.cpp), with the undefined-behaviour sanitizer
    where the toolchain links it: B_r = 2^31 - 1 (OK, mark ff ff ff ff) and
    2^31 (TOO_LONG, no bytes), out_cap = 0, offsets near 2^64 against the
    capacity (no wrap), a record of only empty fragments, pending fragments,
    and the plan's scan at every blocking of the fragments."""
    src = os.path.join(ROOT, "tests", "cpp_defrag", "plan_probe.cpp")
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
    assert r.stdout.strip() == "defrag plan ok"


def test_cpp_mirror_program_compiles():
    """reassemble_stream (include/onc_rpc.hpp) builds against the C ABI
    (build() compiles tests/cpp_defrag)."""
    exe = os.path.join(ROOT, "tests", "cpp_defrag", "test_reassemble")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
