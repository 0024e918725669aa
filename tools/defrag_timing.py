"""Kernel time of fragment framing and reassembly on configs[2]'s wire.

configs[2]'s batch (1M mixed Call/Reply records, payloads 64..4096 B: the
bench's c2 workload) is encoded, then cut into fragments the way a sender
flushing a fixed buffer does: every `size` body bytes of a record start a new
fragment. Sizes: 8192 (every configs[2] record is shorter: the stream keeps
one fragment per record, only the entry points change) and 1024 (most records
become 2..5 fragments). Per size, in one process, from the dispatch
timestamps (Codec.enable_timing / kernel_stats), medians and min-max over
--reps repetitions:

  * onc_frame_fragments on the fragmented stream against onc_frame_stream on
    the unfragmented wire (sum of the framer's launches), and how many chunks
    the one-wave walk re-chased — from a host model of frame.hip's fragment
    mode (the guess per chunk, the chains, the walk), since the device keeps
    no such count; the walk kernel's own time is printed next to it;
  * onc_defragment's copy kernel: time, bytes moved (read + written), and
    the rate against a device-to-device hipMemcpyAsync (torch copy_) of as
    many bytes as the copy writes, timed by events in the same run;
  * its plan (the plan kernels and the length scan).

The outputs are checked first: frag_off against the cut's own offsets, the
reassembled bytes and rec_off against the unfragmented wire.

    python tools/defrag_timing.py [--records N] [--reps 7] [--warmup 2] [--sizes 8192,1024]
"""
import argparse
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _onc_pkg  # noqa: E402

_onc_pkg.load()
import onc_rpc_amd.runtime as R  # noqa: E402
import onc_rpc_amd.synth as S  # noqa: E402

CHUNK = 65536
FRAME_IDS = ("frame_guess_kernel", "frame_chunks_kernel", "frame_walk_kernel", "frame_counts_kernel",
             "frame_write_kernel")
PLAN_IDS = ("defrag_plan_kernels", "len_tiles_kernel", "scan_tiles_kernel", "len_apply_kernel")


def cut(wire, off, size):
    """The stream with every record cut each `size` body bytes ->
    (bytes, frag_off int64[nfrag + 1], records of more than one fragment)."""
    mv = memoryview(wire)
    off = off.tolist()
    parts, fo, pos, multi = [], [0], 0, 0
    pack = struct.Struct(">I").pack
    for i in range(len(off) - 1):
        a, b = off[i] + 4, off[i + 1]
        if b - a <= size:
            parts.append(mv[off[i]:b])
            pos += b - off[i]
            fo.append(pos)
            continue
        multi += 1
        for s in range(a, b, size):
            e = min(s + size, b)
            parts.append(pack((e - s) | (0x80000000 if e == b else 0)))
            parts.append(mv[s:e])
            pos += 4 + e - s
            fo.append(pos)
    return b"".join(parts), np.array(fo, np.int64), multi


def be32_at(a, p):
    p = p.astype(np.int64)
    return ((a[p].astype(np.uint32) << 24) | (a[p + 1].astype(np.uint32) << 16) | (a[p + 2].astype(np.uint32) << 8)
            | a[p + 3].astype(np.uint32))


def model_guesses(a, chunk):
    """frame.hip frame_guess<kFrag>: per chunk the first position passing the
    byte filter (zero bytes at +8..+10), the first-fragment header test and
    the test of the mark behind the fragment; -1 = none; chunk 0 guesses 0."""
    ln = len(a)
    nch = (ln + chunk - 1) // chunk
    g = np.full(nch, -1, np.int64)
    pad = np.concatenate([a, np.zeros(64, np.uint8)])
    slab = 64 << 20
    for s in range(0, max(ln - 15, 0), slab):
        e = min(s + slab, ln - 15)
        z = pad[s:e + 16] == 0
        p = s + np.nonzero(z[8:e - s + 8] & z[9:e - s + 9] & z[10:e - s + 10])[0]
        h, mt, rv = be32_at(pad, p), be32_at(pad, p + 8), be32_at(pad, p + 12)
        want = (h & 0x7FFFFFFF).astype(np.int64) + 4
        ok = (want >= 24) & (want <= ln - p)
        call = (mt == 0) & (rv == 2) & (want >= 44) & (be32_at(pad, p + 32) <= 200)
        rep0 = (mt == 1) & (rv == 0) & (want >= 28) & (be32_at(pad, p + 20) <= 200)
        rep1 = (mt == 1) & (rv == 1) & (be32_at(pad, p + 16) <= 1)
        ok &= call | rep0 | rep1
        p, want = p[ok], want[ok]
        q = p + want
        at_end = q == ln
        qq = np.where(ln - q >= 4, q, 0)
        fits = (ln - q >= 4) & ((be32_at(pad, qq) & 0x7FFFFFFF).astype(np.int64) + 4 <= ln - q)
        p = p[at_end | fits]
        t = p // chunk
        first = np.concatenate(([True], t[1:] != t[:-1])) if len(t) else np.zeros(0, bool)
        new = first & (g[t] < 0) if len(t) else first
        g[t[new]] = p[new]
    if nch:
        g[0] = 0
    return g


def model_walk(fo, g, chunk):
    """frame_chunks<kFrag> + frame_walk<kFrag> over the true chain `fo`
    (fragment starts, then the stream's end): (chunks whose check failed
    among those on the chain, chunks the walk re-chased)."""
    ln = int(fo[-1])
    nch = len(g)
    guessed = np.nonzero(g >= 0)[0]
    on_chain = np.zeros(nch, bool)
    on_chain[guessed] = np.isin(g[guessed], fo[:-1])

    def first_at_or_after(lim):
        return int(fo[np.searchsorted(fo, lim, "left")]) if lim < ln else ln

    fail, xs = {}, {}
    for t in guessed.tolist():
        if not on_chain[t]:
            continue
        x = first_at_or_after(min((t + 1) * chunk, ln))
        prev, bad = t, False
        while x < ln:
            j = x // chunk
            if (g[prev + 1:j] >= 0).any():
                bad = True
                break
            gj = int(g[j])
            if gj == x:
                break
            if 0 <= gj < x:
                bad = True
                break
            x = first_at_or_after(gj if gj >= 0 else min((j + 1) * chunk, ln))
            if gj >= 0 and x < ln and x != gj:
                bad = True
                break
            prev = j
        fail[t], xs[t] = bad, x
    fails = sorted(t for t, b in fail.items() if b)
    rechased = 0
    if fails:
        t, E = fails[0], int(g[fails[0]])
        while True:
            if int(g[t]) == E and not fail.get(t, True):
                nxt = [f for f in fails if f > t]
                if not nxt:
                    break
                t, E = nxt[0], int(g[nxt[0]])
                continue
            if int(g[t]) != E:
                rechased += 1
                x = first_at_or_after(min((t + 1) * chunk, ln))
            else:
                x = xs[t]
            if x >= ln:
                break
            t, E = x // chunk, x
    return len(fails), rechased


def stats(us):
    a = np.array(us)
    return f"median {np.median(a):8.2f}  min {a.min():8.2f}  max {a.max():8.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="8192,1024")
    args = ap.parse_args()
    import torch

    n = args.records
    db = R.DeviceBatch.from_host(S.mixed(n, seed=2), "cuda")
    codec = R.Codec(0)
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
    h_wire = wire[:total].cpu().numpy()
    h_off = off.cpu().numpy()
    print(f"configs[2]: {n} mixed records, {total} wire bytes; {args.reps} timed repetitions after {args.warmup} "
          f"warm-up; {CHUNK}-byte framing chunks", flush=True)

    def timed(call, ids):
        """us per repetition: the sum of the launches under `ids`, and each id's own."""
        tot, per = [], {k: [] for k in ids}
        for rep in range(args.warmup + args.reps):
            codec.reset_stats()
            call()
            codec.sync()
            ks = codec.kernel_stats()
            if rep >= args.warmup:
                tot.append(1e3 * sum(ks[k][0] for k in ids))
                for k in ids:
                    per[k].append(1e3 * ks[k][0])
        return tot, per

    codec.enable_timing(True)
    roff = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    rres = torch.zeros(5, dtype=torch.int64, device="cuda")
    t_rec, _ = timed(lambda: codec.frame_stream(wire, total, roff, n + 1, rres), FRAME_IDS)
    assert rres.cpu().numpy().tolist()[:3] == [n, total, 0] and torch.equal(roff[:n + 1], off)
    print(f"onc_frame_stream, unfragmented wire      us: {stats(t_rec)}", flush=True)

    for size in (int(x) for x in args.sizes.split(",")):
        fbytes, fo, multi = cut(h_wire, h_off, size)
        nfrag, flen = len(fo) - 1, len(fbytes)
        h_frag = np.frombuffer(fbytes, np.uint8)
        print(f"-- fragments of up to {size} body bytes: {nfrag} fragments, {multi} records of more than one, "
              f"{flen} stream bytes", flush=True)
        fw = torch.from_numpy(np.concatenate([h_frag, np.zeros(16, np.uint8)])).cuda()
        d_fo = torch.zeros(nfrag + 2, dtype=torch.int64, device="cuda")
        fres = torch.zeros(5, dtype=torch.int64, device="cuda")
        t_fr, per = timed(lambda: codec.frame_fragments(fw, flen, d_fo, nfrag + 1, fres), FRAME_IDS)
        assert fres.cpu().numpy().tolist()[:3] == [nfrag, flen, 0]
        assert np.array_equal(d_fo.cpu().numpy()[:nfrag + 1], fo), "frag_off differs from the cut's offsets"
        g = model_guesses(h_frag, CHUNK)
        nfail, rechased = model_walk(fo, g, CHUNK)
        print(f"onc_frame_fragments                      us: {stats(t_fr)}   "
              f"= {np.median(t_fr) / np.median(t_rec):.2f} x onc_frame_stream", flush=True)
        print(f"  of which frame_walk                    us: {stats(per['frame_walk_kernel'])}", flush=True)
        print(f"  model: {len(g)} chunks, {int((g >= 0).sum())} guessed, {nfail} failed checks on the chain, "
              f"{rechased} chunks re-chased by the walk"
              + (" (no chunk fell to the serial walk)" if rechased == 0 else ""), flush=True)

        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        o_off = torch.zeros(nfrag + 1, dtype=torch.int64, device="cuda")
        o_st = torch.zeros(nfrag, dtype=torch.int32, device="cuda")
        o_res = torch.zeros(6, dtype=torch.int64, device="cuda")
        ids = ("defrag_copy_kernel",) + PLAN_IDS
        _, per = timed(lambda: codec.defragment(fw, d_fo, nfrag, out, o_off, o_st, o_res, out_cap=total), ids)
        assert o_res.cpu().numpy().tolist() == [n, flen, total, 0, 0, multi]
        assert torch.equal(out[:total], wire[:total]) and torch.equal(o_off[:n + 1], off)
        assert int((o_st[:n] != 0).sum()) == 0 and int((out[total:] != 0xA5).sum()) == 0
        t_copy = per["defrag_copy_kernel"]
        t_plan = [sum(per[k][i] for k in PLAN_IDS) for i in range(args.reps)]
        moved = (flen - 4 * nfrag) + total          # bodies read + records written
        dst = torch.empty(total, dtype=torch.uint8, device="cuda")
        t_cp = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(wire[:total])
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                t_cp.append(1e3 * e0.elapsed_time(e1))
        r_copy = moved / np.median(t_copy) / 1e3
        r_cp = 2 * total / np.median(t_cp) / 1e3
        print(f"onc_defragment copy kernel               us: {stats(t_copy)}   {moved} bytes moved, {r_copy:.0f} GB/s",
              flush=True)
        print(f"device-to-device copy of {total} bytes us: {stats(t_cp)}   {2 * total} bytes moved, {r_cp:.0f} GB/s",
              flush=True)
        print(f"  copy kernel rate / memcpy rate: {r_copy / r_cp:.2f} "
              f"(min-max {moved / max(t_copy) / (2 * total / min(t_cp)):.2f} .. "
              f"{moved / min(t_copy) / (2 * total / max(t_cp)):.2f})", flush=True)
        print(f"onc_defragment plan + length scan        us: {stats(t_plan)}", flush=True)
        del fw, out, dst
    codec.close()


if __name__ == "__main__":
    main()
