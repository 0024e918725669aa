"""Call time of reassembling fragmented records of many connections.

configs[2]'s wire (1M mixed Call/Reply records, payloads 64..4096 B, about
1.9 GB: the bench's c2 workload) is cut at record boundaries into segments of
about 64 KiB, as if it were that many connections' buffers, and every record
is refragmented at max_frag 1 KiB by onc_fragment itself, so that the same
bytes are also one valid fragmented stream. Both wires lie in one buffer.

Measured, against the calls that existed before (never against the new code
itself):
  (a) onc_frame_fragments + onc_defragment on the fragmented wire as one
      stream;
  (b) the same two calls looped over 256 of the segments (per pair; the loop
      over all of them is that times the segment count — extrapolated, not
      run);
  onc_frame_fragment_streams over the segment list, beside onc_frame_streams
  on the unfragmented wire at the same segment size, and
  onc_defragment_extents on its extents beside (a)'s onc_defragment
  (alternating), each with its plan / copy split;
  and the mixed flow: every tenth segment taken from the fragmented wire, the
  others from the unfragmented one — onc_frame_streams, then the rests of the
  FRAGMENTED rows through the two new calls.

Times are device-event times around a whole call (all its launches), medians
and min-max of --reps warm repetitions after --warmup, in microseconds; the
per-kernel splits come from the codec's own dispatch timestamps in a separate
repetition. One run.

    python tools/fragment_streams_timing.py [--records N] [--reps 7] [--warmup 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _onc_pkg  # noqa: E402

_onc_pkg.load()
import onc_rpc_amd.runtime as R  # noqa: E402
import onc_rpc_amd.synth as S  # noqa: E402

MAX_FRAG = 1024
FRAGMENTED = 3


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
    print(f"{name:78s} us: median {np.median(t):10.2f}  min {t.min():10.2f}  max {t.max():10.2f}{extra}", flush=True)


def i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


class At:
    """A byte address as a call's [dev] pointer."""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def split(codec, ids, call):
    codec.enable_timing(True, kernels=ids)
    codec.reset_stats()
    call()
    codec.sync()
    ks = codec.kernel_stats()
    codec.enable_timing(False)
    by = {k: 1e3 * ks[R.K_NAMES[k]][0] for k in ids if ks[R.K_NAMES[k]][1]}
    print("    one call's kernels (dispatch timestamps): " + ", ".join(f"{R.K_NAMES[k]} {v:.1f}" for k, v in by.items()),
          flush=True)
    return by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
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
    first = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode(db, first, off, st, rec_len)
    codec.sync()
    assert int((st != 0).sum()) == 0
    del db
    # the fragmented wire's size: a plan-only onc_fragment call; then both wires in one buffer
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    res3 = torch.zeros(3, dtype=torch.int64, device="cuda")
    codec.fragment(first, off, n, MAX_FRAG, 0, out_off, st, res3, out_cap=0)
    codec.sync()
    nfrag, ftotal = int(res3[0]), int(res3[1])
    fbase = (total + 16 + 255) // 256 * 256
    buf = torch.zeros(fbase + ftotal + 16, dtype=torch.uint8, device="cuda")
    wire, fwire = buf[:total + 16], At(buf.data_ptr() + fbase)
    wire.copy_(first)
    del first
    codec.fragment(wire, off, n, MAX_FRAG, fwire.p, out_off, st, res3, out_cap=ftotal)
    codec.sync()
    assert int((st != 0).sum()) == 0 and int(res3[0]) == nfrag and int(res3[1]) == ftotal
    codec.reserve(nfrag + 8)
    h_off = off.cpu().numpy().view(np.uint64).copy()
    h_out = out_off.cpu().numpy().view(np.uint64).copy()
    print(f"configs[2]: {n} mixed records, {total} wire bytes; refragmented at {MAX_FRAG} B: {nfrag} fragments, "
          f"{ftotal} bytes; {args.reps} timed repetitions after {args.warmup} warm-up; device-event time of whole "
          f"calls; one run", flush=True)

    idx = np.unique(np.searchsorted(h_off[:-1], np.arange(0, total, 65536, dtype=np.uint64)))
    idx = idx[idx < n]
    nseg = len(idx)
    so, fo = h_off[idx], h_out[idx]
    sl = np.diff(np.append(so, np.uint64(total))).astype(np.uint64)
    fl = np.diff(np.append(fo, np.uint64(ftotal))).astype(np.uint64)
    cap = nfrag + 4
    start = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    rlen = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    rows = torch.zeros(8 * nseg, dtype=torch.int64, device="cuda")
    res4 = torch.zeros(4, dtype=torch.int64, device="cuda")
    frame_ids = [R.K_FRAME, R.K_LEN_TILES, R.K_LEN_APPLY, R.K_SCAN_TILES, R.K_FRAME_WRITE, R.K_FRAME_COUNTS]
    defrag_ids = [R.K_DEFRAG_PLAN, R.K_LEN_TILES, R.K_LEN_APPLY, R.K_SCAN_TILES, R.K_DEFRAG_COPY]

    # the framer on the unfragmented wire at the same segment size
    d_so, d_sl = i64(so), i64(sl)
    call = lambda: codec.frame_streams(wire, d_so, d_sl, nseg, start, rlen, None, n + 4, rows, res3)  # noqa: E731
    t = timed(call, args.reps, args.warmup)
    assert res3.cpu().numpy().tolist() == [n, n, 0]
    line(f"onc_frame_streams, {nseg} unfragmented segments of about 64 KiB", t)
    split(codec, frame_ids, call)

    # (a) one stream
    frag_off = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    res5 = torch.zeros(5, dtype=torch.int64, device="cuda")
    call = lambda: codec.frame_fragments(fwire, ftotal, frag_off, cap, res5)  # noqa: E731
    t = timed(call, args.reps, args.warmup)
    assert int(res5[0]) == nfrag and int(res5[1]) == ftotal and int(res5[2]) == 0
    line("(a) onc_frame_fragments, the fragmented wire as one stream", t)
    out = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    rec_off = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    status = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    res6 = torch.zeros(6, dtype=torch.int64, device="cuda")
    one = lambda: codec.defragment(fwire, frag_off, nfrag, out, rec_off, status, res6, out_cap=total)  # noqa: E731

    # onc_frame_fragment_streams over the fragmented segments
    d_fo, d_fl = i64(fo), i64(fl)
    call = lambda: codec.frame_fragment_streams(fwire, d_fo, d_fl, nseg, start, rlen, None, cap, rows, res4)  # noqa: E731
    t = timed(call, args.reps, args.warmup)
    assert res4.cpu().numpy().tolist() == [nfrag, nfrag, n, 0]
    assert torch.equal(start[:nfrag], frag_off[:nfrag])
    line(f"onc_frame_fragment_streams, {nseg} fragmented segments", t)
    split(codec, frame_ids, call)
    ext = lambda: codec.defragment_extents(fwire, start, rlen, nfrag, out, rec_off, status, res6, out_cap=total)  # noqa: E731

    # the reassembly: extents against offsets on the same fragments, alternating
    ta, te = [], []
    for rep in range(args.warmup + args.reps):
        out.zero_()
        a = timed(one, 1, 0)
        assert rep or (torch.equal(out[:total], wire[:total]) and torch.equal(rec_off[:n + 1], off))
        out.zero_()
        e = timed(ext, 1, 0)
        assert rep or (torch.equal(out[:total], wire[:total]) and torch.equal(rec_off[:n + 1], off))
        if rep >= args.warmup:
            ta.append(a[0])
            te.append(e[0])
    ta, te = np.array(ta), np.array(te)
    line("(a) onc_defragment, the same fragments back to back", ta)
    ka = split(codec, defrag_ids, one)
    line("onc_defragment_extents, the same fragments as extents", te)
    ke = split(codec, defrag_ids, ext)
    for name, k in (("plan", R.K_DEFRAG_PLAN), ("copy", R.K_DEFRAG_COPY)):
        print(f"    {name}: extents {ke[k]:.1f} us, offsets {ka[k]:.1f} us", flush=True)
    d, spread = np.median(te) - np.median(ta), ta.max() - ta.min()
    print(f"    extents - offsets (call medians): {d:+.2f} us; (a)'s min-max spread {spread:.2f} us "
          f"({'inside' if abs(d) <= spread else 'OUTSIDE'} the spread)", flush=True)

    # (b) the pair looped over 256 segments
    m = min(256, nseg)
    counts = rows.cpu().numpy().reshape(-1, 8)[:m, 1].tolist()
    views = [(At(fwire.p + int(fo[i])), int(fl[i]), int(counts[i])) for i in range(m)]

    def loop():
        for v, ln, k in views:
            codec.frame_fragments(v, ln, frag_off, cap, res5)
            codec.defragment(v, frag_off, k, out, rec_off, status, res6, out_cap=total)

    t = timed(loop, args.reps, args.warmup) / m
    pair = float(np.median(t))
    line(f"(b) onc_frame_fragments + onc_defragment looped over {m} segments, per pair", t)
    print(f"    the loop over all {nseg} segments: {pair * nseg / 1e3:.1f} ms "
          f"(extrapolated: per-pair median x segment count, not run)", flush=True)

    # the mixed flow: every tenth segment from the fragmented wire
    fr = np.arange(nseg) % 10 == 0
    mo = np.where(fr, fo + np.uint64(fbase), so)
    ml = np.where(fr, fl, sl)
    d_mo, d_ml = i64(mo), i64(ml)
    rows6 = torch.zeros(6 * nseg, dtype=torch.int64, device="cuda")
    call = lambda: codec.frame_streams(buf, d_mo, d_ml, nseg, start, rlen, None, n + 4, rows6, res3)  # noqa: E731
    t1 = timed(call, args.reps, args.warmup)
    r6 = rows6.cpu().numpy().view(np.uint64).reshape(-1, 6)
    which = np.nonzero(r6[:, 3] == FRAGMENTED)[0]
    assert set(which) <= set(np.nonzero(fr)[0]) and len(which) > 0
    nrest = len(which)
    d_ro, d_rl = i64(mo[which] + r6[which, 2]), i64(ml[which] - r6[which, 2])
    fstart = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    flen = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    call = lambda: codec.frame_fragment_streams(buf, d_ro, d_rl, nrest, fstart, flen, None, cap, rows, res4)  # noqa: E731
    t2 = timed(call, args.reps, args.warmup)
    nf, nr = int(res4[0]), int(res4[2])
    assert int(res4[1]) == nf and int(res4[3]) == 0
    call = lambda: codec.defragment_extents(buf, fstart, flen, nf, out, rec_off, status, res6, out_cap=total)  # noqa: E731
    t3 = timed(call, args.reps, args.warmup)
    assert int(res6[0]) == nr and int(res6[3]) == 0 and int((status[:nr] != 0).sum()) == 0
    line(f"mixed: onc_frame_streams, {nseg} segments, {int(fr.sum())} of them fragmented", t1)
    line(f"mixed: onc_frame_fragment_streams, the {nrest} FRAGMENTED rests", t2)
    line(f"mixed: onc_defragment_extents, their {nf} fragments ({nr} records, {int(res6[2])} bytes)", t3)
    print(f"    the three calls: {np.median(t1) + np.median(t2) + np.median(t3):.1f} us; (b)'s pair looped over the "
          f"{nrest} rests: {pair * nrest / 1e3:.1f} ms (extrapolated)", flush=True)
    codec.close()


if __name__ == "__main__":
    main()
