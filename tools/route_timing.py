"""Call time of dispatching decoded Calls to handlers on the device.

The records are configs[2]'s (1M mixed Call/Reply records, payloads
64..4096 B, about 1.9 GB of wire: the bench's c2 workload) with the three call
words of every Call redrawn, since configs[2] draws them at random and no table
would serve any: 90% hit an entry of the table, the rest an unserved procedure,
version or program. The wire is encoded and decoded (onc_decode) once per
table, outside the timed calls; onc_route_calls runs on the decode's output.

Two tables: about 60 entries over 40 handlers (an NFS-like export: NFS v3
a procedure an entry, NFS v4, MOUNT, NLM, NSM, ACL, the portmapper) and 1024
entries over 253 handlers; each with and without the two optional outputs.

Measured beside the call, alternating in one process:
  (copy)  a device-to-device copy of the bytes the call must move with both
          outputs on, n x (64 + 4 + 64 + 64 + 4 + 4): the descriptor and status
          read, calls_out and replies written, route and order written;
  (host)  the route taken today: the descriptors and statuses copied to pinned
          host memory, one thread's C++ loop (tools/route_host_loop.cpp: the
          same lookup, a counting sort, the replies), order and the replies
          copied back. Host clock around the whole, ending in a synchronise.

The call's times are device-event times around the whole call (its four
launches), medians and min-max of --reps warm repetitions after --warmup, in
microseconds; the per-kernel split comes from the codec's own dispatch
timestamps in a separate repetition. The first repetition is checked: route,
order, bin_first and the replies against the host loop's. One run.

    python tools/route_timing.py [--records N] [--reps 7] [--warmup 3]
"""
import argparse
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


def nfs_like():
    """About 60 entries over 40 handlers."""
    rows = [(100003, 3, p, 1, p, 0) for p in range(22)]                 # NFS v3: a procedure an entry
    rows.append((100003, 4, 0, 2, 22, 0))                               # NFS v4: NULL, COMPOUND
    rows += [(100005, 1, 0, 6, 24, 1), (100005, 3, 0, 6, 24, 1)]        # MOUNT
    rows += [(100021, 4, p, 1, 25 + p % 8, 1) for p in range(24)]       # NLM v4
    rows.append((100024, 1, 0, 6, 33, 0))                               # NSM
    rows.append((100227, 3, 0, 5, 39, 1))                               # ACL
    rows += [(100000, v, 0, 6, 39, 1) for v in (2, 3, 4)]               # the portmapper
    return sorted(rows), 40


def wide():
    """1024 entries over 253 handlers."""
    return [(100 + i // 4, 1 + (i // 2) % 2, 1000 * (i % 2), 1 + i % 3, i % 253, 1) for i in range(1024)], 253


def redraw_calls(msgs, rows, seed):
    """Every Call's (program, version, procedure): 90% inside a random entry,
    4% far past its range, 3% another version, 3% another program."""
    rng = np.random.default_rng(seed)
    t = np.array(rows, np.int64)
    idx = np.nonzero(msgs["msg_type"] == L.MSG_CALL)[0]
    e = t[rng.integers(0, len(t), len(idx))]
    u = rng.random(len(idx))
    proc = e[:, 2] + rng.integers(0, 1 << 30, len(idx)) % e[:, 3]
    proc = np.where((u >= 0.90) & (u < 0.94), e[:, 2] + e[:, 3] + 5000, proc)
    msgs["f0"][idx] = np.where(u >= 0.97, e[:, 0] + 500000, e[:, 0])
    msgs["f1"][idx] = np.where((u >= 0.94) & (u < 0.97), e[:, 1] + 100, e[:, 1])
    msgs["f2"][idx] = proc


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
    so = os.path.join(tmp, "route_host_loop.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "onc-rpc_amd", "csrc"),
                    os.path.join(ROOT, "tools", "route_host_loop.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.route_host_loop.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    lib.route_host_loop.restype = None
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    n = args.records
    hb = S.mixed(n, seed=2)
    codec = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    codec.reserve(n)
    tmp = tempfile.TemporaryDirectory()
    host = host_loop_library(tmp.name)
    moved = n * (64 + 4 + 64 + 64 + 4 + 4)
    print(f"configs[2]: {n} mixed records, the Calls' call words redrawn per table; {args.reps} timed repetitions after "
          f"{args.warmup} warm-up; device-event time of whole calls (the host route: host clock); one run", flush=True)

    for name, (rows, nh) in (("NFS-like", nfs_like()), ("wide", wide())):
        redraw_calls(hb.msgs, rows, seed=len(rows))
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
        del wire

        tab = R.route_table(rows)
        ntab = len(tab)
        d_tab = R.to_device(tab, "cuda")
        route = torch.empty(n, dtype=torch.int32, device="cuda")
        order = torch.empty(n, dtype=torch.int32, device="cuda")
        bin_first = torch.empty(nh + 4, dtype=torch.int64, device="cuda")
        res = torch.empty(4, dtype=torch.int64, device="cuda")
        calls = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        reps = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

        def call(outputs):
            return lambda: codec.route_calls(bufs.msgs, bufs.status, n, d_tab, ntab, nh, route, order, bin_first, res,
                                             calls_out=calls if outputs else None, replies=reps if outputs else None)

        # the route taken today
        h_msgs = torch.empty(n * 64, dtype=torch.uint8).pin_memory()
        h_st = torch.empty(n, dtype=torch.int32).pin_memory()
        h_route = torch.empty(n, dtype=torch.int32).pin_memory()
        h_order = torch.empty(n, dtype=torch.int32).pin_memory()
        h_first = torch.empty(nh + 4, dtype=torch.int64).pin_memory()
        h_reps = torch.empty(n * 64, dtype=torch.uint8).pin_memory()
        h_tab = np.ascontiguousarray(tab)
        d_order2 = torch.empty(n, dtype=torch.int32, device="cuda")
        d_reps2 = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

        def today():
            t0 = time.perf_counter()
            h_msgs.copy_(bufs.msgs[:n * 64], non_blocking=True)
            h_st.copy_(bufs.status[:n], non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host.route_host_loop(h_msgs.data_ptr(), h_st.data_ptr(), n, h_tab.ctypes.data, ntab, nh, h_route.data_ptr(),
                                 h_order.data_ptr(), h_first.data_ptr(), h_reps.data_ptr())
            t2 = time.perf_counter()
            d_order2.copy_(h_order, non_blocking=True)
            d_reps2.copy_(h_reps, non_blocking=True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            return 1e6 * np.array([t3 - t0, t1 - t0, t2 - t1, t3 - t2])

        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        copy = lambda: dst.copy_(src)  # noqa: E731  (reads moved / 2, writes moved / 2)

        t_on, t_off, t_copy, t_host = [], [], [], []
        for rep in range(args.warmup + args.reps):
            a = timed(call(True), 1, 0)
            if rep == 0:
                h = today()
                got = res.cpu().numpy().tolist()
                assert got[3] == 0 and got[0] + got[1] + got[2] == n, got
                assert torch.equal(route.cpu(), h_route) and torch.equal(order.cpu(), h_order)
                assert torch.equal(bin_first.cpu(), h_first) and torch.equal(reps.cpu(), h_reps)
                assert torch.equal(calls.view(-1, 64), bufs.msgs[:n * 64].view(-1, 64)[order.long()])
                print(f"{name}: {ntab} entries, {nh} handlers: {got[0]} Calls served, {got[1]} rejected, {got[2]} other "
                      f"records (checked against the host loop)", flush=True)
            b = timed(call(False), 1, 0)
            c = timed(copy, 1, 0)
            h = today()
            if rep >= args.warmup:
                t_on.append(a[0])
                t_off.append(b[0])
                t_copy.append(c[0])
                t_host.append(h)
        t_on, t_off, t_copy, t_host = np.array(t_on), np.array(t_off), np.array(t_copy), np.array(t_host)
        line(f"  onc_route_calls, calls_out and replies on ({moved} bytes moved)", t_on,
             f"  ({np.median(t_on) / np.median(t_copy):.2f}x the device copy, "
             f"{np.median(t_host[:, 0]) / np.median(t_on):.1f}x faster than the host route)")
        line("  onc_route_calls, route and order only", t_off)
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
            print(f"    one call's kernels, outputs {'on' if outputs else 'off'} (dispatch timestamps): classify + scans "
                  f"{1e3 * ks[R.K_NAMES[R.K_DEFRAG_PLAN]][0]:.1f}, scatter {1e3 * ks[R.K_NAMES[R.K_DEFRAG_COPY]][0]:.1f}",
                  flush=True)
        del bufs, calls, reps, src, dst, d_reps2
    codec.close()
    tmp.cleanup()


if __name__ == "__main__":
    main()
