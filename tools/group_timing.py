"""Call time of grouping a send batch by connection on the device.

The batch is configs[2]'s (1M mixed Call/Reply descriptors, payloads 64..4096 B:
the bench's c2 workload) with the Calls' call words redrawn for the 54-entry
table of tools/route_timing.py. onc_route_calls runs once, outside the timed
calls: the items are its Calls, served and rejected (n = bin_first[nh + 1]),
`via` is its order and `msgs` its replies. rec_conn says which connection's
buffer a record arrived in: the wire (sized by onc_encode_lengths, never
encoded) is cut at record boundaries as tools/streams_timing.py cuts it, into
segments of about 64 KiB (two radix passes), and into 200 and 100 000 segments
(one pass, three passes).

Measured beside the call, alternating in one process:
  (a)  a device-to-device copy of the bytes the call must move with msgs_out on,
       n x (4 + 4 + 4 + 64 + 64) + 8 (nconn + 2): via, rec_conn and the
       descriptors read, order and the descriptors written, conn_first written;
  (b)  the route taken before: rec_conn, via and the descriptors copied to
       pinned host memory, one thread's counting sort and gather
       (tools/group_host_loop.cpp), order, conn_first and the descriptors copied
       back. Host clock around the whole, ending in a synchronise.

The call's times are device-event times around the whole call (all its
launches), medians and min-max of --reps warm repetitions after --warmup, in
microseconds; the kernels' split comes from the codec's own dispatch
timestamps in a separate repetition: the counts, scans, bounds and result
launches under one id, the scatters and the gather under the other, so a
pass's share is the difference between the one-, two- and three-pass rows. The
first repetition is checked: order, conn_first, result and msgs_out against the
host loop's. One run. --launches makes the calls alone, for a kernel trace of
its own (one row per dispatch); --trace FILE reads such a trace's CSV and prints
every kernel's time, pass by pass.

    python tools/group_timing.py [--records N] [--reps 7] [--warmup 3]
    python tools/group_timing.py --launches        (under a kernel trace)
    python tools/group_timing.py --trace run_kernel_trace.csv
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _onc_pkg  # noqa: E402

_onc_pkg.load()
import onc_rpc_amd.layout as L  # noqa: E402,F401
import onc_rpc_amd.runtime as R  # noqa: E402
import onc_rpc_amd.synth as S  # noqa: E402
from route_timing import line, nfs_like, redraw_calls, timed  # noqa: E402


def host_loop_library(tmp):
    so = os.path.join(tmp, "group_host_loop.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "onc-rpc_amd", "csrc"),
                    os.path.join(ROOT, "tools", "group_host_loop.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.group_host_loop.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp]
    lib.group_host_loop.restype = None
    return lib


SHAPE_PASSES = (2, 1, 3)        # the three connection counts, in the order main() takes them


def trace_medians(path, calls):
    """A kernel trace's CSV (one row per dispatch) of a --launches run of `calls`
    calls a shape, msgs_out on and off in turn -> every group_* kernel's time."""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0].split("::")[-1]
            if name.startswith("group_"):
                start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                rows.setdefault(name, []).append((start, (end - start) / 1e3))
    print(f"kernel trace {os.path.basename(path)}: every dispatch of the --launches run, {calls} calls a shape, per "
          f"shape (1: 64 KiB segments, two passes; 2: 200 connections, one pass; 3: 100 000 connections, three)",
          flush=True)
    for name in ("group_count_kernel", "group_scan_digits_kernel", "group_scan_total_kernel", "group_scatter_kernel",
                 "group_bounds_kernel", "group_result_kernel", "group_gather_kernel"):
        t = np.array([d for _, d in sorted(rows.get(name, []))])            # in dispatch order
        per_call = {"group_bounds_kernel": 1, "group_result_kernel": 1, "group_gather_kernel": 0.5}
        at = 0
        for i, passes in enumerate(SHAPE_PASSES):
            k = per_call.get(name, passes)
            count = int(calls * k)
            part = t[at:at + count]
            at += count
            if len(part) != count or not count:
                print(f"  {name}, shape {i + 1}: {len(part)} dispatches where {count} were expected", flush=True)
                continue
            if name in per_call:
                line(f"  {name}, shape {i + 1} ({count} dispatches)", part)
            else:
                for p in range(passes):
                    line(f"  {name}, shape {i + 1}, pass {p} ({calls} dispatches)", part[p::passes])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", action="store_true", help="the calls alone, for a kernel trace")
    ap.add_argument("--trace", help="a kernel trace's CSV to summarise")
    args = ap.parse_args()
    if args.trace:
        trace_medians(args.trace, 2 * (args.warmup + args.reps))
        return
    import torch

    nrec = args.records
    hb = S.mixed(nrec, seed=2)
    rows, nh = nfs_like()
    redraw_calls(hb.msgs, rows, seed=len(rows))
    codec = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    codec.reserve(nrec)
    tmp = tempfile.TemporaryDirectory()
    host = None if args.launches else host_loop_library(tmp.name)

    # the wire's record offsets, and the Calls in handler order with their reply descriptors
    db = R.DeviceBatch.from_host(hb, "cuda")
    rec_len = torch.empty(nrec, dtype=torch.int32, device="cuda")
    st = torch.empty(nrec, dtype=torch.int32, device="cuda")
    codec.encode_lengths(db, rec_len, st)
    codec.sync()
    assert int((st != 0).sum()) == 0
    h_off = np.concatenate([[0], np.cumsum(rec_len.cpu().numpy().view(np.uint32).astype(np.uint64))]).astype(np.uint64)
    total = int(h_off[-1])
    tab = R.route_table(rows)
    d_tab = R.to_device(tab, "cuda")
    route = torch.empty(nrec, dtype=torch.int32, device="cuda")
    via = torch.empty(nrec, dtype=torch.int32, device="cuda")
    bin_first = torch.empty(nh + 4, dtype=torch.int64, device="cuda")
    res4 = torch.empty(4, dtype=torch.int64, device="cuda")
    msgs = torch.empty(nrec * 64, dtype=torch.uint8, device="cuda")
    st.zero_()
    codec.route_calls(db.msgs, st, nrec, d_tab, len(tab), nh, route, via, bin_first, res4, replies=msgs)
    codec.sync()
    n = int(bin_first[nh + 1])
    del db, route
    if not args.launches:
        print(f"configs[2]: {nrec} mixed descriptors, {total} wire bytes by their lengths; {len(tab)}-entry table, {nh} "
              f"handlers: {n} Calls in handler order are the items; {args.reps} timed repetitions after {args.warmup} "
              f"warm-up; device-event time of whole calls (the host route: host clock); one run", flush=True)

    order = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    res = torch.empty(3, dtype=torch.int64, device="cuda")
    h_conn = torch.empty(nrec, dtype=torch.int32).pin_memory()
    h_via = torch.empty(n, dtype=torch.int32).pin_memory()
    h_msgs = torch.empty(n * 64, dtype=torch.uint8).pin_memory()
    h_order = torch.empty(n, dtype=torch.int32).pin_memory()
    h_out = torch.empty(n * 64, dtype=torch.uint8).pin_memory()
    h_res = torch.empty(3, dtype=torch.int64)
    d_order2 = torch.empty(n, dtype=torch.int32, device="cuda")
    d_out2 = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

    for shape, target in enumerate((65536, total // 200 + 1, total // 100_000 + 1)):
        idx = np.unique(np.searchsorted(h_off[:-1], np.arange(0, total, target, dtype=np.uint64)))
        idx = idx[idx < nrec]
        nconn = len(idx)
        rec_seg = (np.searchsorted(idx, np.arange(nrec), side="right") - 1).astype(np.uint32)
        d_conn = torch.from_numpy(rec_seg.view(np.int32).copy()).cuda()
        conn_first = torch.empty(nconn + 2, dtype=torch.int64, device="cuda")
        h_first = torch.empty(nconn + 2, dtype=torch.int64).pin_memory()
        d_first2 = torch.empty(nconn + 2, dtype=torch.int64, device="cuda")
        passes = (int(nconn).bit_length() + 7) // 8
        assert nrec != 1_000_000 or passes == SHAPE_PASSES[shape]       # (what --trace splits the dispatches by)
        moved = n * (4 + 4 + 4 + 64 + 64) + 8 * (nconn + 2)

        def call(gather):
            return lambda: codec.group_by_conn(d_conn, nrec, via, n, nconn, order, conn_first, res, msgs=msgs,
                                               msgs_out=out if gather else None)

        def before():
            t0 = time.perf_counter()
            h_conn.copy_(d_conn, non_blocking=True)
            h_via.copy_(via[:n], non_blocking=True)
            h_msgs.copy_(msgs[:n * 64], non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host.group_host_loop(h_conn.data_ptr(), nrec, h_via.data_ptr(), n, nconn, h_order.data_ptr(),
                                 h_first.data_ptr(), h_msgs.data_ptr(), h_out.data_ptr(), h_res.data_ptr())
            t2 = time.perf_counter()
            d_order2.copy_(h_order, non_blocking=True)
            d_first2.copy_(h_first, non_blocking=True)
            d_out2.copy_(h_out, non_blocking=True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            return 1e6 * np.array([t3 - t0, t1 - t0, t2 - t1, t3 - t2])

        if args.launches:
            for rep in range(args.warmup + args.reps):
                call(True)()
                call(False)()
            codec.sync()
            continue
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        copy = lambda: dst.copy_(src)  # noqa: E731  (reads moved / 2, writes moved / 2)

        t_on, t_off, t_copy, t_host = [], [], [], []
        for rep in range(args.warmup + args.reps):
            a = timed(call(True), 1, 0)
            if rep == 0:
                before()
                got = res.cpu().numpy().tolist()
                assert got == h_res.numpy().tolist() and got[0] + got[1] == n, (got, h_res)
                assert torch.equal(order.cpu(), h_order) and torch.equal(conn_first.cpu(), h_first)
                assert torch.equal(out.cpu(), h_out)
                print(f"{nconn} connections ({passes} pass{'es' if passes != 1 else ''}): {got[0]} items sent on "
                      f"{got[2]} connections, {got[1]} dropped (checked against the host loop)", flush=True)
            b = timed(call(False), 1, 0)
            c = timed(copy, 1, 0)
            h = before()
            if rep >= args.warmup:
                t_on.append(a[0])
                t_off.append(b[0])
                t_copy.append(c[0])
                t_host.append(h)
        t_on, t_off, t_copy, t_host = np.array(t_on), np.array(t_off), np.array(t_copy), np.array(t_host)
        line(f"  onc_group_by_conn, msgs_out on ({moved} bytes moved)", t_on,
             f"  ({np.median(t_on) / np.median(t_copy):.2f}x the device copy, "
             f"{np.median(t_host[:, 0]) / np.median(t_on):.1f}x faster than the host route)")
        line("  onc_group_by_conn, order and conn_first only", t_off)
        line(f"  (a) device copy of {moved} bytes (half read, half written)", t_copy)
        line("  (b) D2H + one thread's counting sort and gather + H2D, host clock", t_host[:, 0],
             f"  (medians: D2H {np.median(t_host[:, 1]):.0f}, loop {np.median(t_host[:, 2]):.0f}, "
             f"H2D {np.median(t_host[:, 3]):.0f})")
        ids = [R.K_DEFRAG_PLAN, R.K_DEFRAG_COPY]
        for gather in (True, False):
            codec.enable_timing(True, kernels=ids)
            codec.reset_stats()
            call(gather)()
            codec.sync()
            ks = codec.kernel_stats()
            codec.enable_timing(False)
            plan, cp = ks[R.K_NAMES[R.K_DEFRAG_PLAN]], ks[R.K_NAMES[R.K_DEFRAG_COPY]]
            print(f"    one call's kernels, msgs_out {'on' if gather else 'off'} (dispatch timestamps): counts + scans + "
                  f"bounds + result {1e3 * plan[0]:.1f} in {plan[1]} launches, scatters"
                  f"{' + gather' if gather else ''} {1e3 * cp[0]:.1f} in {cp[1]} launches", flush=True)
        del src, dst, d_conn
    codec.close()
    tmp.cleanup()


if __name__ == "__main__":
    main()
