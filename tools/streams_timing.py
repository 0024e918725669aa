"""Call time of segmented framing and of the extents decode.

configs[2]'s wire (1M mixed Call/Reply records, payloads 64..4096 B, about
1.9 GB: the bench's c2 workload) is cut at record boundaries into segments of
about 4 KiB, 64 KiB and 1 MiB, as if it were that many connections' buffers.

Framing: onc_frame_streams over each segment list, onc_frame_stream over the
whole wire, and onc_frame_stream called once per segment for 256 of the 64 KiB
segments (per-call cost; the loop over all of them is that times the segment
count — extrapolated, not run). Decode: onc_decode_extents against
onc_decode_bounded on the same back-to-back records, alternating, and
onc_decode_extents with the 64 KiB segments listed in descending address
order, over the device wire and over a mapped host copy of it.

Times are device-event times around a whole call (all its launches), medians
and min-max of --reps warm repetitions after --warmup, in microseconds; the
per-kernel split of one onc_frame_streams call comes from the codec's own
dispatch timestamps in a separate repetition.

    python tools/streams_timing.py [--records N] [--reps 25] [--warmup 5] [--lab-lib PATH]

--lab-lib names a second build of the library made with
-DONC_EXT_FIRST_BASE=1 (csrc/Makefile HIPFLAGS, OUT): its extents decode keeps
the loaders' base at the wave's first record instead of its lowest, so a wave
that crosses into a lower segment takes the per-lane loads. The descending
decode then alternates between the two builds in this process, which shows
what the minimum-base rule buys.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _onc_pkg  # noqa: E402

_onc_pkg.load()
import onc_rpc_amd.layout as L  # noqa: E402
import onc_rpc_amd.runtime as R  # noqa: E402
import onc_rpc_amd.synth as S  # noqa: E402


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
    print(f"{name:66s} us: median {np.median(t):9.2f}  min {t.min():9.2f}  max {t.max():9.2f}{extra}", flush=True)


def i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lab-lib", default="")
    args = ap.parse_args()
    import torch

    n = args.records
    hb = S.mixed(n, seed=2)
    db = R.DeviceBatch.from_host(hb, "cuda")
    codec = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    codec.reserve(n)
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
    h_off = off.cpu().numpy().view(np.uint64).copy()
    h_len = np.diff(h_off.astype(np.int64)).astype(np.uint32)
    print(f"configs[2]: {n} mixed records, {total} wire bytes; {args.reps} timed repetitions after "
          f"{args.warmup} warm-up; device-event time of whole calls", flush=True)

    def cut(target):
        idx = np.unique(np.searchsorted(h_off[:-1], np.arange(0, total, target, dtype=np.uint64)))
        idx = idx[idx < n]
        so = h_off[idx]
        return idx, so, np.diff(np.append(so, np.uint64(total))).astype(np.uint64)

    start = torch.empty(n + 8, dtype=torch.int64, device="cuda")
    rlen = torch.empty(n + 8, dtype=torch.int32, device="cuda")
    rseg = torch.empty(n + 8, dtype=torch.int32, device="cuda")
    res3 = torch.zeros(3, dtype=torch.int64, device="cuda")
    dec = R.DecodeBuffers(n)
    out = (dec.msgs, dec.unix, dec.status, dec.aux0, dec.aux1)

    res5 = torch.zeros(5, dtype=torch.int64, device="cuda")
    foff = torch.empty(n + 8, dtype=torch.int64, device="cuda")
    t = timed(lambda: codec.frame_stream(wire, total, foff, n + 4, res5), args.reps, args.warmup)
    assert int(res5[0]) == n and torch.equal(foff[:n + 1], off)
    line("onc_frame_stream, the whole wire", t)
    whole = float(np.median(t))
    for name, target in (("4 KiB", 4096), ("64 KiB", 65536), ("1 MiB", 1 << 20)):
        idx, so, sl = cut(target)
        nseg = len(so)
        d_so, d_sl = i64(so), i64(sl)
        rows = torch.zeros(6 * nseg, dtype=torch.int64, device="cuda")
        codec.reserve(max(n, nseg))
        call = lambda: codec.frame_streams(wire, d_so, d_sl, nseg, start, rlen, rseg, n + 4, rows, res3)  # noqa: E731
        t = timed(call, args.reps, args.warmup)
        r = res3.cpu().numpy()
        assert (int(r[0]), int(r[1]), int(r[2])) == (n, n, 0)
        assert torch.equal(start[:n], off[:n]) and torch.equal(rlen[:n], rec_len)
        line(f"onc_frame_streams, {nseg} segments of about {name}", t,
             f"  ({np.median(t) / whole:.2f}x onc_frame_stream)")
        ids = [R.K_FRAME, R.K_LEN_TILES, R.K_LEN_APPLY, R.K_SCAN_TILES, R.K_FRAME_WRITE, R.K_FRAME_COUNTS]
        codec.enable_timing(True, kernels=ids)
        codec.reset_stats()
        call()
        codec.sync()
        ks = codec.kernel_stats()
        codec.enable_timing(False)
        print("    one call's kernels (dispatch timestamps): " +
              ", ".join(f"{R.K_NAMES[k]} {1e3 * ks[R.K_NAMES[k]][0]:.1f}" for k in ids if ks[R.K_NAMES[k]][1]),
              flush=True)
        if target == 65536:
            m = min(256, nseg)
            seg = [(int(so[i]), int(sl[i])) for i in range(m)]
            base = wire.data_ptr()

            class At:                                   # the segment's first byte as the call's wire
                def __init__(self, p):
                    self.p = p

                def data_ptr(self):
                    return self.p

            views = [At(base + o) for o, _ in seg]

            def loop():
                for v, (_, ln) in zip(views, seg):
                    codec.frame_stream(v, ln, foff, n + 4, res5)

            t = timed(loop, args.reps, args.warmup) / m
            line(f"onc_frame_stream looped over {m} of the 64 KiB segments, per call", t)
            print(f"    the loop over all {nseg} segments: {np.median(t) * nseg / 1e3:.1f} ms "
                  f"(extrapolated: per-call median x segment count, not run)", flush=True)

    # decode: extents against bounded offsets on the same back-to-back records, alternating
    tb, te = [], []
    for rep in range(args.warmup + args.reps):
        b = timed(lambda: codec.decode_bounded(wire, total, off, n, L.DECODE_SLICE, *out), 1, 0)
        e = timed(lambda: codec.decode_extents(wire, total, off, rec_len, n, L.DECODE_SLICE, *out), 1, 0)
        if rep >= args.warmup:
            tb.append(b[0])
            te.append(e[0])
    assert int((dec.status != 0).sum()) == 0
    tb, te = np.array(tb), np.array(te)
    line("onc_decode_bounded, records back to back", tb)
    line("onc_decode_extents, the same records", te)
    d, spread = np.median(te) - np.median(tb), tb.max() - tb.min()
    print(f"    extents - bounded (medians): {d:+.2f} us; bounded min-max spread {spread:.2f} us "
          f"({'inside' if abs(d) <= spread else 'OUTSIDE'} the spread)", flush=True)

    # the 64 KiB segments in descending address order (records ascending inside a segment)
    idx, so, sl = cut(65536)
    ends = np.append(idx[1:], n)
    order = np.concatenate([np.arange(idx[k], ends[k]) for k in range(len(idx) - 1, -1, -1)])
    d_start, d_len = i64(h_off[:-1][order]), torch.from_numpy(h_len[order].view(np.int32).copy()).cuda()
    codecs = [("minimum base", codec)]
    if args.lab_lib:
        main_lib, R._LIB = R._LIB, None                    # a second library in this process
        R.load_library(args.lab_lib)
        codecs.append(("first-record base (lab build)", R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)))
        R._LIB = main_lib
    # the same over a mapped host copy of the wire (a pinned slab: the headers cross PCIe)
    host = R.HostMapped.from_array(codec, wire.cpu().numpy())
    for where, w in (("device wire", wire), ("mapped host wire", host)):
        ts = {name: [] for name, _ in codecs}
        for rep in range(args.warmup + args.reps):
            for name, c in codecs:
                t = timed(lambda: c.decode_extents(w, total, d_start, d_len, n, L.DECODE_SLICE, *out), 1, 0)
                assert rep or int((dec.status != 0).sum()) == 0
                if rep >= args.warmup:
                    ts[name].append(t[0])
        for name, _ in codecs:
            line(f"onc_decode_extents, {len(so)} 64 KiB segments descending, {where}, {name}", np.array(ts[name]))
    host.close()
    for _, c in codecs:
        c.close()


if __name__ == "__main__":
    main()
