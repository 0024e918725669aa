"""Call time of pairing decoded Replies with pending Calls on the device.

The records are configs[2]'s descriptors (1M mixed records: the bench's c2
workload) redrawn as Replies: every descriptor's msg_type becomes Reply and
its xid one of the pending list's, the other words stay as configs[2] draws
them. onc_match_replies reads a record's status and the first 16-byte granule
of its descriptor only, so the descriptors are used as they are built, without
an encode and a decode in between. The pending list: one entry per record on
29 366 connections (the streams benchmark's count), the xids of a connection
counting up from a random start, tags random; the Replies arrive shuffled.

Three shapes: 1M Replies over 1M entries, all answered; 1M over a list of 4M
(the table is built over the list, not the batch); 1M over 1M with every tenth
Reply unknown. Each with and without tag_out / still.

Measured beside the call, alternating in one process:
  (copy)  a device-to-device copy of the bytes the call must move with both
          outputs on: per record the status, the granule, rec_conn, match and
          tag_out (4 + 16 + 4 + 4 + 8), per entry the key read by the insert,
          hit written, the entry read and (where it waits) written (8 + 4 + 16
          + 16 k / np);
  (host)  the route taken today: the descriptors, statuses and connections
          copied to pinned host memory, one thread's C++ loop
          (tools/match_host_loop.cpp: std::unordered_map over the same list),
          match and hit copied back. Host clock around the whole, ending in a
          synchronise.

The call's times are device-event times around the whole call, medians and
min-max of --reps warm repetitions after --warmup, in microseconds. The first
repetition is checked: match, hit and result against the host loop's, still
against the list. --launches makes the calls alone, for a kernel trace of its
own (one row per dispatch); --trace FILE reads such a trace's CSV and prints
the median and min-max of every match_* kernel. One run.

    python tools/match_timing.py [--records N] [--reps 7] [--warmup 3]
"""
import argparse
import csv
import ctypes as C
import os
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

NCONN = 29366


def pending_list(npend, seed):
    """npend entries over NCONN connections, a connection's xids counting up from a random start."""
    rng = np.random.default_rng(seed)
    p = np.zeros(npend, L.PENDING_DTYPE)
    conn = rng.integers(0, NCONN, npend).astype(np.uint32)
    start = rng.integers(0, 1 << 32, NCONN, dtype=np.uint64)
    order = np.argsort(conn, kind="stable")
    first = np.searchsorted(conn[order], np.arange(NCONN))
    nth = np.empty(npend, np.uint64)
    nth[order] = np.arange(npend, dtype=np.uint64) - first[conn[order]].astype(np.uint64)
    p["conn"] = conn
    p["xid"] = ((start[conn] + nth) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    p["tag"] = rng.integers(0, 1 << 64, npend, dtype=np.uint64)
    return p


def redraw_replies(msgs, pend, unknown_every, seed):
    """Every record a Reply to a different entry, shuffled; every unknown_every-th to a connection nobody uses."""
    rng = np.random.default_rng(seed)
    n = len(msgs)
    pick = rng.permutation(len(pend))[:n]
    msgs["msg_type"] = L.MSG_REPLY
    msgs["xid"] = pend["xid"][pick]
    conn = pend["conn"][pick].copy()
    if unknown_every:
        conn[::unknown_every] = NCONN + 7
    return conn


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
    print(f"{name:74s} us: median {np.median(t):10.2f}  min {t.min():10.2f}  max {t.max():10.2f}{extra}", flush=True)


def host_loop_library(tmp):
    so = os.path.join(tmp, "match_host_loop.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "onc-rpc_amd", "csrc"),
                    os.path.join(ROOT, "tools", "match_host_loop.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.match_host_loop.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
    lib.match_host_loop.restype = None
    return lib


def trace_medians(path):
    """A kernel trace's CSV (one row per dispatch) -> the match_* kernels' times."""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0].split("::")[-1]
            if name.startswith("match_"):
                start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                rows.setdefault(name, []).append((start, (end - start) / 1e3))
    print(f"kernel trace {os.path.basename(path)}: every dispatch of the --launches run, per shape (1: 1M over 1M, 2: 1M "
          f"over 4M, 3: every tenth unknown)", flush=True)
    for name in ("match_clear_kernel", "match_insert_kernel", "match_probe_kernel", "match_resolve_kernel",
                 "match_scan_kernel", "match_compact_kernel"):
        t = np.array([d for _, d in sorted(rows.get(name, [(0, 0.0)]))])       # in dispatch order
        # the --launches run makes its calls shape by shape: as many dispatches of a kernel for each
        for i, part in enumerate(np.array_split(t, 3) if len(t) >= 3 else [t]):
            if name == "match_compact_kernel" or len(part) < 2:
                line(f"  {name}, shape {i + 1} ({len(part)} dispatches)", part)
            else:                                                    # (the calls alternate: outputs on, then off)
                line(f"  {name}, shape {i + 1}, outputs on ({len(part[0::2])} dispatches)", part[0::2])
                line(f"  {name}, shape {i + 1}, outputs off ({len(part[1::2])} dispatches)", part[1::2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", action="store_true", help="the calls alone, for a kernel trace")
    ap.add_argument("--trace", help="a kernel trace's CSV to summarise")
    args = ap.parse_args()
    if args.trace:
        trace_medians(args.trace)
        return
    import torch

    n = args.records
    hb = S.mixed(n, seed=2)
    msgs = hb.msgs.copy()
    shapes = (("1M Replies over 1M entries, all answered", n, 0), ("1M Replies over a list of 4M", 4 * n, 0),
              ("1M Replies over 1M entries, every tenth unknown", n, 10))
    codec = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    codec.reserve(4 * n)
    tmp = tempfile.TemporaryDirectory()
    host = None if args.launches else host_loop_library(tmp.name)
    if not args.launches:
        print(f"configs[2]: {n} descriptors redrawn as Replies, {NCONN} connections; {args.reps} timed repetitions after "
              f"{args.warmup} warm-up; device-event time of whole calls (the host route: host clock); one run", flush=True)

    for name, npend, unknown_every in shapes:
        pend = pending_list(npend, seed=npend % 1000 + unknown_every)
        conn = redraw_replies(msgs, pend, unknown_every, seed=unknown_every + 1)
        d_msgs = R.to_device(msgs, "cuda")
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_conn = torch.from_numpy(conn.view(np.int32).copy()).cuda()
        d_pend = R.to_device(pend, "cuda")
        match = torch.empty(n, dtype=torch.int32, device="cuda")
        hit = torch.empty(npend, dtype=torch.int32, device="cuda")
        tag = torch.empty(n, dtype=torch.int64, device="cuda")
        still = torch.empty(npend * 16, dtype=torch.uint8, device="cuda")
        res = torch.empty(6, dtype=torch.int64, device="cuda")

        def call(outputs):
            return lambda: codec.match_replies(d_msgs, d_st, d_conn, n, d_pend, npend, match, hit, res,
                                               tag_out=tag if outputs else None, still=still if outputs else None)

        if args.launches:
            for rep in range(args.warmup + args.reps):
                call(True)()
                call(False)()
            codec.sync()
            continue

        # the route taken today
        h_msgs = torch.empty(n * 64, dtype=torch.uint8).pin_memory()
        h_st = torch.empty(n, dtype=torch.int32).pin_memory()
        h_conn = torch.empty(n, dtype=torch.int32).pin_memory()
        h_match = torch.empty(n, dtype=torch.int32).pin_memory()
        h_hit = torch.empty(npend, dtype=torch.int32).pin_memory()
        h_res = np.zeros(6, np.uint64)
        h_pend = np.ascontiguousarray(pend)
        d_match2 = torch.empty(n, dtype=torch.int32, device="cuda")
        d_hit2 = torch.empty(npend, dtype=torch.int32, device="cuda")

        def today():
            t0 = time.perf_counter()
            h_msgs.copy_(d_msgs[:n * 64], non_blocking=True)
            h_st.copy_(d_st, non_blocking=True)
            h_conn.copy_(d_conn, non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host.match_host_loop(h_msgs.data_ptr(), h_st.data_ptr(), h_conn.data_ptr(), n, h_pend.ctypes.data, npend,
                                 h_match.data_ptr(), h_hit.data_ptr(), h_res.ctypes.data)
            t2 = time.perf_counter()
            d_match2.copy_(h_match, non_blocking=True)
            d_hit2.copy_(h_hit, non_blocking=True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            return 1e6 * np.array([t3 - t0, t1 - t0, t2 - t1, t3 - t2])

        t_on, t_off, t_copy, t_host = [], [], [], []
        moved = 0
        for rep in range(args.warmup + args.reps):
            a = timed(call(True), 1, 0)
            if rep == 0:
                h = today()
                got = res.cpu().numpy().view(np.uint64)
                assert got.tolist() == h_res.tolist() and int(got[:5].sum()) == n, (got, h_res)
                assert torch.equal(match.cpu(), h_match) and torch.equal(hit.cpu(), h_hit)
                k = int(got[5])
                waiting = pend[h_hit.numpy().view(np.uint32) == R.MATCH_NONE]
                assert still.cpu().numpy()[:16 * k].tobytes() == waiting.tobytes() and len(waiting) == k
                assert torch.equal(tag.cpu()[match.cpu() >= 0],
                                   torch.from_numpy(pend["tag"].view(np.int64))[match.cpu()[match.cpu() >= 0].long()])
                moved = n * (4 + 16 + 4 + 4 + 8) + npend * (8 + 4 + 16) + 16 * k
                src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
                dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
                print(f"{name}: {got[0]} matched, {got[1]} unknown, {got[2]} duplicate, {k} of {npend} entries still "
                      f"waiting (checked against the host loop)", flush=True)
            b = timed(call(False), 1, 0)
            c = timed(lambda: dst.copy_(src), 1, 0)      # (reads moved / 2, writes moved / 2)
            h = today()
            if rep >= args.warmup:
                t_on.append(a[0])
                t_off.append(b[0])
                t_copy.append(c[0])
                t_host.append(h)
        t_on, t_off, t_copy, t_host = np.array(t_on), np.array(t_off), np.array(t_copy), np.array(t_host)
        line(f"  onc_match_replies, tag_out and still on ({moved} bytes moved)", t_on,
             f"  ({np.median(t_on) / np.median(t_copy):.2f}x the device copy, "
             f"{np.median(t_host[:, 0]) / np.median(t_on):.1f}x faster than the host route)")
        line("  onc_match_replies, match and hit only", t_off)
        line(f"  (copy) device copy of {moved} bytes (half read, half written)", t_copy)
        line("  (host) D2H + one thread's loop + H2D, host clock", t_host[:, 0],
             f"  (medians: D2H {np.median(t_host[:, 1]):.0f}, loop {np.median(t_host[:, 2]):.0f}, "
             f"H2D {np.median(t_host[:, 3]):.0f})")
        ids = [R.K_DEFRAG_PLAN, R.K_DEFRAG_COPY]
        for outputs in (True, False):
            codec.enable_timing(True, kernels=ids)
            codec.reset_stats()
            call(outputs)()
            codec.sync()
            ks = codec.kernel_stats()
            codec.enable_timing(False)
            print(f"    one call's kernels, outputs {'on' if outputs else 'off'} (dispatch timestamps): clear + insert + "
                  f"probe + resolve + scan {1e3 * ks[R.K_NAMES[R.K_DEFRAG_PLAN]][0]:.1f}, compact "
                  f"{1e3 * ks[R.K_NAMES[R.K_DEFRAG_COPY]][0]:.1f}", flush=True)
        del d_msgs, d_pend, match, hit, tag, still, src, dst, h_msgs
    codec.close()
    tmp.cleanup()


if __name__ == "__main__":
    main()
