"""Call time of placing head-decoded payloads in aligned slots on the device.

The wire is tools/defragment_heads_timing.py's: configs[2] (1M mixed Call/Reply
records, payloads 64..4096 B, about 1.9 GB: the bench's c2 workload) cut at
record boundaries into segments of about 64 KiB, every record refragmented at
max_frag 1 KiB by onc_fragment itself; onc_frame_fragment_streams gives the
fragments as extents, once, outside the timed calls.

Measured, alternating in one process:
  (a) baseline  onc_defragment_extents (the whole stream rebuilt, headers
                included) + onc_decode of it: the only device route to
                contiguous payloads that existed before, and the yardstick —
                its copy kernel moves the same payload bytes;
  (b) new       onc_defragment_heads + onc_decode_heads (head_len 160) +
                onc_payload_slots + onc_place_payloads at align 16 and 4096,
                and the last two calls, and the place kernel, alone;
  (c) context   a device copy of the same number of payload bytes;
  (d) identity  on the unfragmented wire: onc_decode_extents alone (what
                existed before: no placement at all), then the added cost of
                onc_payload_slots (rec_start form) + onc_place_payloads
                (identity form) at align 16 and 4096, and the same device copy.

Times are device-event times around whole calls (all their launches), medians
and min-max of --reps warm repetitions after --warmup, in microseconds; the
per-kernel splits come from the codec's own dispatch timestamps in a separate
repetition. The first repetition of every path is checked: the slots against
the decoded lengths, and a sample of the placed payloads byte for byte against
the baseline's rebuilt stream. One run.

    python tools/place_payloads_timing.py [--records N] [--reps 7] [--warmup 3]
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
HEAD = 160
ALIGNS = (16, 4096)


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

    def dec(b):
        return b.msgs, b.unix, b.status, b.aux0, b.aux1

    # (a) the whole stream rebuilt, then decoded
    out = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    rec_off = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    status = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    res6 = torch.zeros(6, dtype=torch.int64, device="cuda")
    base_bufs = R.DecodeBuffers(n)
    ext = lambda: codec.defragment_extents(fbuf, start, flen, nfrag, out, rec_off, status, res6, out_cap=total)  # noqa: E731
    decode = lambda: codec.decode(out, rec_off, n, L.DECODE_SLICE, *dec(base_bufs))  # noqa: E731

    def baseline():
        ext()
        decode()

    # (b) the heads gathered and decoded, the payloads placed
    new_bufs = R.DecodeBuffers(n)
    hbase, hlo = R.aligned_bytes(n * HEAD, 0, "cuda")
    heads = At(hbase.data_ptr() + hlo)
    h_len = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    h_frag = torch.empty(cap + 5, dtype=torch.int64, device="cuda")
    h_pre = torch.empty(cap + 4, dtype=torch.int64, device="cuda")
    h_st = torch.empty(cap + 4, dtype=torch.int32, device="cuda")
    h_res = torch.zeros(6, dtype=torch.int64, device="cuda")
    pay_pos = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    pay_len = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    slot_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    msgs_out = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    p_res = torch.zeros(3, dtype=torch.int64, device="cuda")
    dst_cap = n * 4096 + 4096                        # payloads of up to 4096 bytes in slots of 4096
    dst = torch.zeros(dst_cap, dtype=torch.uint8, device="cuda")

    gather = lambda: codec.defragment_heads(fbuf, start, flen, nfrag, HEAD, heads, n, h_len, h_frag, h_pre, h_st,  # noqa: E731
                                            h_res)
    decode_heads = lambda: codec.decode_heads(heads, HEAD, h_len, n, L.DECODE_SLICE, *dec(new_bufs))  # noqa: E731

    def slots(align):
        return lambda: codec.payload_slots(new_bufs.msgs, new_bufs.status, n, align, pay_pos, pay_len, slot_off, p_res,
                                           head_len=HEAD, msgs_out=msgs_out)

    place = lambda: codec.place_payloads(fbuf, start, flen, nfrag, h_frag, h_pre, h_len, pay_pos, pay_len, slot_off, n,  # noqa: E731
                                         dst, dst_cap=dst_cap)

    def new(align):
        s = slots(align)

        def every():
            gather()
            decode_heads()
            s()
            place()
        return every

    def check(align, where, where_off):
        """The slots against the decoded lengths, and a sample of the placed
        payloads against the bytes at `where`[`where_off`[r]]."""
        k, nbytes, need = (int(x) for x in p_res.cpu().numpy())
        lens = pay_len[:n].cpu().numpy().view(np.uint32).astype(np.int64)
        so = slot_off.cpu().numpy().view(np.uint64).astype(np.int64)
        rounded = (lens + align - 1) // align * align
        assert k == int((lens > 0).sum()) and nbytes == int(lens.sum()) and need == int(rounded.sum()) <= dst_cap
        assert np.array_equal(so, np.concatenate(([0], np.cumsum(rounded))))
        src = where_off.cpu().numpy().view(np.uint64).astype(np.int64)
        rng = np.random.default_rng(align)
        for r in np.concatenate((rng.integers(0, n, 1500), [0, n - 1])):
            a, b, ln = int(so[r]), int(src[r]), int(lens[r])
            assert torch.equal(dst[a:a + ln], where[b:b + ln]), r
        return k, nbytes, need

    tb = {a: [] for a in ALIGNS}
    tn = {a: [] for a in ALIGNS}
    sizes = {}
    for rep in range(args.warmup + args.reps):
        for align in ALIGNS:
            out.zero_()
            b = timed(baseline, 1, 0)
            t = timed(new(align), 1, 0)
            if rep == 0:
                assert int((new_bufs.status[:n] != 0).sum()) == 0 and int((base_bufs.status[:n] != 0).sum()) == 0
                base_pay = base_bufs.msgs.view(torch.int64).view(-1, 8)[:n, 3].contiguous()    # payload_off in `out`
                sizes[align] = check(align, out, base_pay)
            if rep >= args.warmup:
                tb[align].append(b[0])
                tn[align].append(t[0])
    allb = np.concatenate([np.array(tb[a]) for a in ALIGNS])
    line("(a) baseline: onc_defragment_extents + onc_decode (every repetition)", allb)
    tx = timed(ext, args.reps, args.warmup)
    line("    onc_defragment_extents alone", tx)
    by = split(codec, [R.K_DEFRAG_PLAN, R.K_LEN_TILES, R.K_LEN_APPLY, R.K_SCAN_TILES, R.K_DEFRAG_COPY], ext)
    yard = by[R.K_DEFRAG_COPY]
    nbytes = sizes[ALIGNS[0]][1]
    copy_src = out[:nbytes]
    copy_dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tc = timed(lambda: copy_dst.copy_(copy_src), args.reps, args.warmup)
    for align in ALIGNS:
        b, t = np.array(tb[align]), np.array(tn[align])
        k, nb, need = sizes[align]
        line(f"(b) new: heads + decode_heads + payload_slots + place_payloads, align {align}", t,
             f"  ({np.median(b) / np.median(t):.2f}x the baseline beside it, {np.median(b):.2f} us; {k} payloads, "
             f"{nb} bytes in {need})")
        s = slots(align)
        s()
        codec.sync()
        ts = timed(s, args.reps, args.warmup)
        line(f"    onc_payload_slots alone, align {align}", ts)
        tp = timed(place, args.reps, args.warmup)
        line(f"    onc_place_payloads alone, align {align}", tp,
             f"  ({np.median(tp) / yard:.2f}x defrag_copy_kernel, {np.median(tp) / np.median(tc):.2f}x the device copy)")
        split(codec, [R.K_DEFRAG_PLAN, R.K_DEFRAG_COPY], lambda: (s(), place()))
    line(f"(c) context: device copy of the payload bytes ({nbytes})", tc)

    # (d) the unfragmented wire: decoded in place, then the added cost of placing
    d_start = off[:n].contiguous()
    ctx_bufs = R.DecodeBuffers(n)
    dext = lambda: codec.decode_extents(wire, total, d_start, rec_len, n, L.DECODE_SLICE, *dec(ctx_bufs))  # noqa: E731
    dext()
    codec.sync()
    te = timed(dext, args.reps, args.warmup)
    line("(d) identity: onc_decode_extents of the unfragmented wire (before: no placement)", te)

    def slots_id(align):
        return lambda: codec.payload_slots(ctx_bufs.msgs, ctx_bufs.status, n, align, pay_pos, pay_len, slot_off, p_res,
                                           rec_start=d_start, msgs_out=msgs_out)

    place_id = lambda: codec.place_payloads(wire, d_start, rec_len, n, None, None, rec_len, pay_pos, pay_len, slot_off,  # noqa: E731
                                            n, dst, dst_cap=dst_cap)
    for align in ALIGNS:
        s = slots_id(align)

        def added():
            s()
            place_id()
        ta, tp = [], []
        for rep in range(args.warmup + args.reps):
            a = timed(added, 1, 0)
            if rep == 0:
                ctx_pay = ctx_bufs.msgs.view(torch.int64).view(-1, 8)[:n, 3].contiguous()
                assert check(align, wire, ctx_pay) == sizes[align]
            p = timed(place_id, 1, 0)
            if rep >= args.warmup:
                ta.append(a[0])
                tp.append(p[0])
        line(f"    added: onc_payload_slots + onc_place_payloads (identity form), align {align}", np.array(ta))
        line(f"    onc_place_payloads alone, identity form, align {align}", np.array(tp),
             f"  ({np.median(tp) / np.median(tc):.2f}x the device copy)")
    codec.close()


if __name__ == "__main__":
    main()
