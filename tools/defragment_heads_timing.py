"""Call time of decoding fragmented records without copying their payloads.

The wire is tools/fragment_streams_timing.py's: configs[2] (1M mixed Call/Reply
records, payloads 64..4096 B, about 1.9 GB: the bench's c2 workload) cut at
record boundaries into segments of about 64 KiB, every record refragmented at
max_frag 1 KiB by onc_fragment itself; onc_frame_fragment_streams gives the
fragments as extents, once, outside the timed calls.

Measured, alternating in one process:
  baseline  onc_defragment_extents (the whole stream rebuilt, payloads
            included) + onc_decode of it: the path that existed before, and
            the yardstick — never the new code against itself;
  new       onc_defragment_heads + onc_decode_heads at head_len 64, 160 and
            736: only the heads are gathered, the payloads stay in the wire;
  context   onc_decode_heads beside onc_decode_extents on the unfragmented
            wire's records, and a device fill of n * head_len bytes (what
            writing the heads buffer alone costs).

Times are device-event times around whole calls (all their launches), medians
and min-max of --reps warm repetitions after --warmup, in microseconds; the
per-kernel splits come from the codec's own dispatch timestamps in a separate
repetition. The first repetition of every path is checked: statuses, lengths
and descriptors of the new path against the baseline's. One run.

    python tools/defragment_heads_timing.py [--records N] [--reps 7] [--warmup 3]
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

MAX_FRAG = 1024
HEADS = (64, 160, 736)
DEC_BAD_EXTENT = 106


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
    wire = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode(db, wire, off, st, rec_len)
    codec.sync()
    assert int((st != 0).sum()) == 0
    del db
    # the fragmented wire: a plan-only onc_fragment call for its size, then the call
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    res3 = torch.zeros(3, dtype=torch.int64, device="cuda")
    codec.fragment(wire, off, n, MAX_FRAG, 0, out_off, st, res3, out_cap=0)
    codec.sync()
    nfrag, ftotal = int(res3[0]), int(res3[1])
    fbuf = torch.zeros(ftotal + 16, dtype=torch.uint8, device="cuda")
    codec.fragment(wire, off, n, MAX_FRAG, fbuf, out_off, st, res3, out_cap=ftotal)
    codec.sync()
    assert int((st != 0).sum()) == 0 and int(res3[0]) == nfrag and int(res3[1]) == ftotal
    codec.reserve(nfrag + 8)
    h_off = off.cpu().numpy().view(np.uint64).copy()
    h_out = out_off.cpu().numpy().view(np.uint64).copy()
    idx = np.unique(np.searchsorted(h_off[:-1], np.arange(0, total, 65536, dtype=np.uint64)))
    idx = idx[idx < n]
    nseg = len(idx)
    fo = h_out[idx]
    fl = np.diff(np.append(fo, np.uint64(ftotal))).astype(np.uint64)
    print(f"configs[2]: {n} mixed records, {total} wire bytes; refragmented at {MAX_FRAG} B: {nfrag} fragments, "
          f"{ftotal} bytes, {nseg} segments of about 64 KiB; {args.reps} timed repetitions after {args.warmup} warm-up; "
          f"device-event time of whole calls; one run", flush=True)

    cap = nfrag + 4
    start = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    flen = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    rows = torch.zeros(8 * nseg, dtype=torch.int64, device="cuda")
    res4 = torch.zeros(4, dtype=torch.int64, device="cuda")
    codec.frame_fragment_streams(fbuf, i64(fo), i64(fl), nseg, start, flen, None, cap, rows, res4)
    codec.sync()
    assert res4.cpu().numpy().tolist() == [nfrag, nfrag, n, 0]

    # baseline: the whole stream rebuilt, then decoded
    out = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    rec_off = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    status = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    res6 = torch.zeros(6, dtype=torch.int64, device="cuda")
    base_bufs = R.DecodeBuffers(n)
    new_bufs = R.DecodeBuffers(n)

    def dec(b):
        return b.msgs, b.unix, b.status, b.aux0, b.aux1

    ext = lambda: codec.defragment_extents(fbuf, start, flen, nfrag, out, rec_off, status, res6, out_cap=total)  # noqa: E731
    decode = lambda: codec.decode(out, rec_off, n, L.DECODE_SLICE, *dec(base_bufs))  # noqa: E731

    def baseline():
        ext()
        decode()

    # new: the heads gathered, then decoded
    hmax = max(HEADS)
    hbase, hlo = R.aligned_bytes(n * hmax, 0, "cuda")
    heads = At(hbase.data_ptr() + hlo)
    h_len = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    h_frag = torch.empty(cap + 5, dtype=torch.int64, device="cuda")
    h_pre = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    h_st = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    h_res = torch.zeros(6, dtype=torch.int64, device="cuda")

    def gather(h):
        return lambda: codec.defragment_heads(fbuf, start, flen, nfrag, h, heads, n, h_len, h_frag, h_pre, h_st, h_res)

    def decode_heads(h):
        return lambda: codec.decode_heads(heads, h, h_len, n, L.DECODE_SLICE, *dec(new_bufs))

    def new(h):
        g, d = gather(h), decode_heads(h)

        def both():
            g()
            d()
        return both

    def check(h):
        """The new path's results against the baseline's, on the device."""
        assert torch.equal(rec_off[:n + 1], off) and torch.equal(out[:total], wire[:total])
        assert h_res.cpu().numpy().tolist() == [n, nfrag, n * h, 0, 0, int(res6[5])]
        assert torch.equal(h_len[:n], rec_len) and int((h_st[:n] != 0).sum()) == 0
        short = new_bufs.status[:n] == DEC_BAD_EXTENT
        assert torch.equal(new_bufs.status[:n][~short], base_bufs.status[:n][~short])
        assert int((base_bufs.status[:n] != 0).sum()) == 0
        a = new_bufs.msgs.view(-1, 64)[:n][~short]
        b = base_bufs.msgs.view(-1, 64)[:n][~short]
        # xid .. payload_len, the auths' ids and kinds (the offsets differ by the rebase)
        for lo, hi in ((0, 24), (32, 40), (48, 56)):
            assert torch.equal(a[:, lo:hi], b[:, lo:hi])
        return int(short.sum())

    tb = {h: [] for h in HEADS}
    tn = {h: [] for h in HEADS}
    shorts = {}
    for rep in range(args.warmup + args.reps):
        for h in HEADS:
            out.zero_()
            b = timed(baseline, 1, 0)
            hbase.zero_()
            t = timed(new(h), 1, 0)
            if rep == 0:
                shorts[h] = check(h)
            if rep >= args.warmup:
                tb[h].append(b[0])
                tn[h].append(t[0])
    allb = np.concatenate([np.array(tb[h]) for h in HEADS])
    line("baseline: onc_defragment_extents + onc_decode (every repetition)", allb)
    tx = timed(ext, args.reps, args.warmup)
    td = timed(decode, args.reps, args.warmup)
    line("    onc_defragment_extents alone", tx)
    split(codec, [R.K_DEFRAG_PLAN, R.K_LEN_TILES, R.K_LEN_APPLY, R.K_SCAN_TILES, R.K_DEFRAG_COPY], ext)
    line("    onc_decode of the rebuilt stream alone", td)
    for h in HEADS:
        b, t = np.array(tb[h]), np.array(tn[h])
        line(f"new: onc_defragment_heads + onc_decode_heads, head_len {h}", t,
             f"  ({np.median(b) / np.median(t):.2f}x the baseline beside it, {np.median(b):.2f} us; "
             f"{shorts[h]} HEAD_SHORT records)")
        tg = timed(gather(h), args.reps, args.warmup)
        line(f"    onc_defragment_heads alone, head_len {h} ({n * h} heads bytes)", tg)
        split(codec, [R.K_DEFRAG_PLAN, R.K_DEFRAG_COPY], gather(h))
        th = timed(decode_heads(h), args.reps, args.warmup)
        line(f"    onc_decode_heads alone, head_len {h}", th)

    # context: the heads decode beside the extents decode of the unfragmented records, and a plain fill
    d_start = off[:n].contiguous()
    ctx_bufs = R.DecodeBuffers(n)
    dext = lambda: codec.decode_extents(wire, total, d_start, rec_len, n, L.DECODE_SLICE, *dec(ctx_bufs))  # noqa: E731
    te, th = [], []
    g160 = gather(160)
    g160()
    codec.sync()
    dh = decode_heads(160)
    for rep in range(args.warmup + args.reps):
        e = timed(dext, 1, 0)
        t = timed(dh, 1, 0)
        if rep >= args.warmup:
            te.append(e[0])
            th.append(t[0])
    line("context: onc_decode_extents, the unfragmented wire's records", np.array(te))
    line("context: onc_decode_heads, head_len 160, beside it", np.array(th))
    for h in HEADS:
        view = hbase[hlo:hlo + n * h]
        tf = timed(lambda: view.fill_(0x5A), args.reps, args.warmup)
        line(f"context: device fill of n * head_len = {n * h} bytes", tf)
    codec.close()


if __name__ == "__main__":
    main()
