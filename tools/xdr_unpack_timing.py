"""Call time of decoding Call arguments into columns on the device.

The records are configs[2]'s (1M mixed Call/Reply records, payloads
64..4096 B, about 1.9 GB of wire: the bench's c2 workload) with the head of
every Call's payload overwritten by NFSv3 WRITE-shaped arguments: a 32-byte file
handle (opaque<64>), offset (hyper), count, stable, and the length word of a data
opaque that takes the rest of the payload — 56 bytes, of which the call reads the
five words outside the handle. The Replies keep configs[2]'s random payloads:
a Success reply's does not parse (its first word is no handle length) and costs
one granule; the other records are skipped. The wire is encoded and decoded
(onc_decode) once, outside the timed calls; onc_xdr_unpack runs on the decode's
output over all records, in the rec_start form, with present and rest_pos /
rest_len on and no replies.

Measured beside the call, alternating in one process:
  (extents) onc_decode_extents over the same records: the sibling with the same
            access shape, one or two scattered lines per record and line-sized
            outputs;
  (copy)    a device-to-device copy of the bytes the call must move (the tool
            computes and prints the count): per record the status word; per OK
            record 32 bytes of descriptor; per parsed record the 16-byte
            granules that hold the words it reads; the columns, xstat, present,
            rest_pos and rest_len written;
  (host)    the route taken before: the descriptors, statuses and the wire
            copied to pinned host memory, one thread's C++ loop
            (tools/xdr_host_loop.cpp: the same parse), the columns and per-record
            outputs copied back. Host clock around the whole, ending in a
            synchronise.

The call's times are device-event times around the whole call (its two
launches), medians and min-max of --reps warm repetitions after --warmup, in
microseconds. The first repetition's outputs are compared with the host loop's.
One run. The report goes to stdout and to profiles/xdr_unpack_timing.log.

    python tools/xdr_unpack_timing.py [--records N] [--reps 7] [--warmup 3] [--log PATH]
"""
import argparse
import ctypes as C
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _onc_pkg  # noqa: E402

_onc_pkg.load()
import onc_rpc_amd.layout as L  # noqa: E402
import onc_rpc_amd.runtime as R  # noqa: E402
import onc_rpc_amd.synth as S  # noqa: E402

ARGS = 56           # fh length, 32 handle bytes, offset, count, stable, data length
LOG = []


def say(text):
    print(text, flush=True)
    LOG.append(text)


def write_args(hb, seed):
    """WRITE3args at the head of every Call's payload, the data opaque taking the rest."""
    rng = np.random.default_rng(seed)
    m = hb.msgs
    idx = np.nonzero(m["msg_type"] == L.MSG_CALL)[0]
    plen = m["payload_len"][idx].astype(np.int64)
    assert (plen >= ARGS).all()
    k = len(idx)
    head = np.zeros((k, ARGS), np.uint8)
    head[:, 0:4] = np.frombuffer(struct.pack(">I", 32), np.uint8)
    head[:, 4:36] = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    head[:, 36:44] = rng.integers(0, 1 << 40, k).astype(">u8").view(np.uint8).reshape(k, 8)
    data_len = ((plen - ARGS) & ~3).astype(np.uint32)
    head[:, 44:48] = data_len.astype(">u4").view(np.uint8).reshape(k, 4)        # count = the data's length
    head[:, 48:52] = rng.integers(0, 3, k).astype(">u4").view(np.uint8).reshape(k, 4)
    head[:, 52:56] = data_len.astype(">u4").view(np.uint8).reshape(k, 4)
    at = m["payload_off"][idx].astype(np.int64)[:, None] + np.arange(ARGS)[None, :]
    hb.payload_arena[at] = head
    return k


def timed(fn, reps, warmup):
    import torch
    out = []
    for rep in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= warmup:
            out.append(1e3 * a.elapsed_time(b))
    return np.array(out)


def line(name, t, extra=""):
    say(f"{name:74s} us: median {np.median(t):10.2f}  min {t.min():10.2f}  max {t.max():10.2f}{extra}")


def host_loop_library(tmp):
    so = os.path.join(tmp, "xdr_host_loop.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "onc-rpc_amd", "csrc"),
                    os.path.join(ROOT, "tools", "xdr_host_loop.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.xdr_host_loop.argtypes = [vp, u64, vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    lib.xdr_host_loop.restype = None
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "xdr_unpack_timing.log"))
    args = ap.parse_args()
    import torch

    n = args.records
    hb = S.mixed(n, seed=2)
    calls = write_args(hb, seed=7)
    codec = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    codec.reserve(n)
    tmp = tempfile.TemporaryDirectory()
    host = host_loop_library(tmp.name)
    say(f"configs[2]: {n} mixed records, {calls} Calls with WRITE-shaped arguments at the head of their payloads; "
        f"{args.reps} timed repetitions after {args.warmup} warm-up; device-event time of whole calls (the host route: "
        f"host clock); one run")

    db = R.DeviceBatch.from_host(hb, "cuda")
    rec_len = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    codec.encode_lengths(db, rec_len, st)
    codec.sync()
    total = int(rec_len.cpu().numpy().view(np.uint32).astype(np.int64).sum())
    wire = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode(db, wire, off, st, rec_len)
    codec.sync()
    assert int((st != 0).sum()) == 0
    del db
    bufs = R.DecodeBuffers(n)
    codec.decode(wire, off, n, L.DECODE_SLICE, bufs.msgs, bufs.unix, bufs.status, bufs.aux0, bufs.aux1)
    codec.sync()
    assert int((bufs.status[:n] != 0).sum()) == 0
    rec_start = off[:n].contiguous()

    fields, cap = R.xdr_schema([(R.XDR_OPAQUE_VAR, 64, 0), (R.XDR_U64, 0, 0), (R.XDR_U32, 0, 0), (R.XDR_U32, 0, 0),
                                (R.XDR_OPAQUE_VAR, 0xFFFFFFFF, 0)], n)
    assert R.xdr_schema_check(fields, n, cap) == 0
    cols = torch.empty(cap, dtype=torch.uint8, device="cuda")
    xstat = torch.empty(n, dtype=torch.int32, device="cuda")
    present = torch.empty(n, dtype=torch.int64, device="cuda")
    rest_pos = torch.empty(n, dtype=torch.int32, device="cuda")
    rest_len = torch.empty(n, dtype=torch.int32, device="cuda")
    res = torch.empty(4, dtype=torch.int64, device="cuda")

    def call():
        codec.xdr_unpack(wire, total, bufs.msgs, bufs.status, n, fields, cols, xstat, res, rec_start=rec_start,
                         present=present, rest_pos=rest_pos, rest_len=rest_len)

    bufs2 = R.DecodeBuffers(n)

    def extents():
        codec.decode_extents(wire, total, rec_start, rec_len, n, L.DECODE_SLICE, bufs2.msgs, bufs2.unix, bufs2.status,
                             bufs2.aux0, bufs2.aux1)

    # the route taken before
    h_wire = torch.empty(total, dtype=torch.uint8).pin_memory()
    h_msgs = torch.empty(n * 64, dtype=torch.uint8).pin_memory()
    h_st = torch.empty(n, dtype=torch.int32).pin_memory()
    h_rs = rec_start.cpu()
    h_cols = torch.empty(cap, dtype=torch.uint8).pin_memory()
    h_xstat = torch.empty(n, dtype=torch.int32).pin_memory()
    h_present = torch.empty(n, dtype=torch.int64).pin_memory()
    h_rp = torch.empty(n, dtype=torch.int32).pin_memory()
    h_rl = torch.empty(n, dtype=torch.int32).pin_memory()
    h_res = torch.empty(4, dtype=torch.int64)
    back = [torch.empty_like(t, device="cuda") for t in (h_cols, h_xstat, h_present, h_rp, h_rl)]

    def before():
        t0 = time.perf_counter()
        h_msgs.copy_(bufs.msgs[:n * 64], non_blocking=True)
        h_st.copy_(bufs.status[:n], non_blocking=True)
        h_wire.copy_(wire[:total], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host.xdr_host_loop(h_wire.data_ptr(), total, h_msgs.data_ptr(), h_st.data_ptr(), n, h_rs.data_ptr(),
                           fields.ctypes.data, len(fields), 0, h_cols.data_ptr(), h_xstat.data_ptr(),
                           h_present.data_ptr(), h_rp.data_ptr(), h_rl.data_ptr(), h_res.data_ptr())
        t2 = time.perf_counter()
        for d, h in zip(back, (h_cols, h_xstat, h_present, h_rp, h_rl)):
            d.copy_(h, non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return 1e6 * np.array([t3 - t0, t1 - t0, t2 - t1, t3 - t2])

    t_call, t_ext, t_copy, t_host = [], [], [], []
    src = dst = None
    for rep in range(args.warmup + args.reps):
        a = timed(call, 1, 0)
        if rep == 0:
            h = before()
            got = res.cpu().numpy().tolist()
            assert got == h_res.numpy().tolist() and got[0] + got[1] + got[2] == n and got[0] == calls, (got, calls)
            assert torch.equal(cols.cpu(), h_cols) and torch.equal(xstat.cpu(), h_xstat)
            assert torch.equal(present.cpu(), h_present) and torch.equal(rest_pos.cpu(), h_rp)
            assert torch.equal(rest_len.cpu(), h_rl)
            # the bytes the call must move
            xs = h_xstat.numpy().view(np.uint32) & 0xFF
            ok_status = n                                                # every record decoded
            parsed = int(((xs != R.XDR_SKIPPED) & (xs != R.XDR_BAD_EXTENT)).sum())
            o = bufs.msgs[:n * 64].cpu().numpy().view(L.MSG_DTYPE)["payload_off"].astype(np.int64)
            okr = xs == R.XDR_OK
            words = [0, 36, 40, 44, 48, 52]                              # the words an OK record reads
            g = np.stack([(o[okr] + w) // 16 for w in words] + [(o[okr] + w + 3) // 16 for w in words], axis=1)
            g.sort(axis=1)
            granules = int((np.diff(g, axis=1) != 0).sum() + len(g)) + (parsed - int(okr.sum()))
            moved = 4 * n + 32 * ok_status + 16 * granules + cap + 4 * n + 8 * n + 8 * n
            say(f"{got[0]} records parsed OK, {got[1]} with arguments that do not parse, {got[2]} skipped (checked against "
                f"the host loop); bytes the call must move: {moved} ({4 * n} status, {32 * ok_status} descriptors, "
                f"{16 * granules} wire granules, {cap + 20 * n} outputs)")
            src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        b = timed(extents, 1, 0)
        c = timed(lambda: dst.copy_(src), 1, 0)
        h = before()
        if rep >= args.warmup:
            t_call.append(a[0])
            t_ext.append(b[0])
            t_copy.append(c[0])
            t_host.append(h)
    t_call, t_ext, t_copy, t_host = np.array(t_call), np.array(t_ext), np.array(t_copy), np.array(t_host)
    line("  onc_xdr_unpack, present and rest on", t_call,
         f"  ({np.median(t_call) / np.median(t_copy):.2f}x the device copy, {np.median(t_call) / np.median(t_ext):.2f}x "
         f"onc_decode_extents, {np.median(t_host[:, 0]) / np.median(t_call):.1f}x faster than the host route)")
    line("  (extents) onc_decode_extents over the same records", t_ext)
    line("  (copy) device copy of the bytes the call must move (half read, half written)", t_copy)
    line("  (host) D2H + one thread's loop + H2D, host clock", t_host[:, 0],
         f"  (medians: D2H {np.median(t_host[:, 1]):.0f}, loop {np.median(t_host[:, 2]):.0f}, "
         f"H2D {np.median(t_host[:, 3]):.0f})")
    codec.close()
    tmp.cleanup()
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
