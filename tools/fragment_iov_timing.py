"""Kernel time of fragmenting the vectored encode (onc_fragment_iov) against
the packed path, on configs[2].

configs[2]'s batch (1M mixed Call/Reply records, payloads 64..4096 B: the
bench's c2 workload) is sent fragmented in two ways, on the same batch, in one
process, the two paths alternated per repetition:

  * vectored: onc_encode_iov (headers only), then onc_fragment_iov (marks and
    a list of pieces; its three plan launches and its fill separately);
  * packed:   onc_encode (every byte), then onc_fragment (every byte again) —
    the only way to the same stream without onc_fragment_iov.

max_frag: 8192 (no configs[2] record is split: the entry points alone) and
1024 (most records become 2..5 fragments). Times are the dispatch timestamps
(Codec.enable_timing / kernel_stats), medians and min-max over --reps
repetitions after --warmup. The store-bound floor of the fill is a device
fill (torch fill_) of as many bytes as the fill kernel writes, timed by events
in the same run. The bytes each path writes are computed from the record
lengths.

The outputs are checked first: result, out_off and piece_off against the
closed form, and the pieces of the first 20 000 records gathered on the host
against onc_fragment's output bytes.

    python tools/fragment_iov_timing.py [--records N] [--reps 7] [--warmup 2] [--sizes 8192,1024]
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

CHECKED = 20_000


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
    hb = S.mixed(n, seed=2)
    arena = hb.payload_arena
    db = R.DeviceBatch.from_host(hb, "cuda")
    codec = R.Codec(0)
    rec_len = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    codec.encode_lengths(db, rec_len, st)
    codec.sync()
    lens = rec_len.cpu().numpy().view(np.uint32).astype(np.int64)
    total = int(lens.sum())
    wire = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    hdr = torch.zeros(1024 * n, dtype=torch.uint8, device="cuda")
    d_iov = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    i_st = torch.empty(n, dtype=torch.int32, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")

    def encode():
        codec.encode(db, wire, off, st, rec_len)

    def encode_iov():
        codec.encode_iov(db, hdr, d_iov, i_st, tot)

    encode()
    encode_iov()
    codec.sync()
    assert int((st != 0).sum()) == 0 and int((i_st != 0).sum()) == 0
    iov = d_iov.cpu().numpy().view(L.IOV_DTYPE)
    hl, pl = iov["hdr_len"].astype(np.int64), iov["payload_len"].astype(np.int64)
    assert np.array_equal(hl + pl, lens) and int(tot.cpu()[1]) == total
    hdr_bytes = int(hl.sum())
    print(f"configs[2]: {n} mixed records, {total} wire bytes of which {hdr_bytes} header bytes; {args.reps} timed "
          f"repetitions after {args.warmup} warm-up, the two paths alternated", flush=True)

    def device_us(call):
        """Device time of every launch of one call, by kernel id."""
        codec.reset_stats()
        call()
        codec.sync()
        return {k: 1e3 * v[0] for k, v in codec.kernel_stats().items()}

    codec.enable_timing(True)
    for size in (int(x) for x in args.sizes.split(",")):
        Hb, B = hl - 4, lens - 4
        k = np.maximum(1, -(-B // size))
        x = ((Hb % size != 0) & (pl > 0)).astype(np.int64)
        e = np.where(B == 0, 1, 2 * k + x)
        out_len = B + 4 * k
        nfrag, need, multi, npieces = int(k.sum()), int(out_len.sum()), int((k > 1).sum()), int(e.sum())
        codec.reserve(n)
        print(f"-- max_frag {size}: {nfrag} fragments, {multi} records of more than one, {need} stream bytes, "
              f"{npieces} pieces", flush=True)
        out = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        o_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        o_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        o_res = torch.zeros(3, dtype=torch.int64, device="cuda")
        marks = torch.full((4 * nfrag + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        pieces = torch.full((16 * npieces + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        v_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        p_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        v_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        v_res = torch.zeros(4, dtype=torch.int64, device="cuda")

        def fragment():
            codec.fragment(wire, off, n, size, out, o_off, o_st, o_res, out_cap=need)

        def fragment_iov():
            codec.fragment_iov(d_iov, n, size, marks, pieces, v_off, p_off, v_st, v_res, marks_cap=4 * nfrag,
                               max_pieces=npieces)

        # the check
        fragment()
        fragment_iov()
        codec.sync()
        assert o_res.cpu().numpy().tolist() == [nfrag, need, multi]
        assert v_res.cpu().numpy().tolist() == [nfrag, need, multi, npieces]
        assert np.array_equal(v_off.cpu().numpy(), np.concatenate(([0], np.cumsum(out_len))))
        assert np.array_equal(p_off.cpu().numpy(), np.concatenate(([0], np.cumsum(e))))
        assert torch.equal(v_off, o_off) and int((v_st != 0).sum()) == 0 and int((o_st != 0).sum()) == 0
        assert int((marks[4 * nfrag:] != 0xA5).sum()) == 0 and int((pieces[16 * npieces:] != 0xA5).sum()) == 0
        m = min(n, CHECKED)
        pe, fe, be = int(e[:m].sum()), int(k[:m].sum()), int(out_len[:m].sum())
        he = int((iov["hdr_off"][:m].astype(np.int64) + hl[:m]).max())
        got = R.gather_pieces(pieces[:16 * pe].cpu().numpy().view(L.FRAG_PIECE_DTYPE), marks[:4 * fe].cpu().numpy(),
                              hdr[:he].cpu().numpy(), arena)
        assert got == out[:be].cpu().numpy().tobytes(), "gathered pieces differ from onc_fragment's bytes"
        print(f"checked: result, out_off, piece_off against the closed form; the {pe} pieces of the first {m} records "
              f"gather to onc_fragment's first {be} bytes", flush=True)

        t = {name: [] for name in ("enc_iov", "plan_iov", "fill_iov", "enc", "plan", "copy")}
        for rep in range(args.warmup + args.reps):
            a, b = device_us(encode_iov), device_us(fragment_iov)
            c, d = device_us(encode), device_us(fragment)
            if rep >= args.warmup:
                t["enc_iov"].append(sum(a.values()))
                t["plan_iov"].append(b["defrag_plan_kernels"])
                t["fill_iov"].append(b["defrag_copy_kernel"])
                t["enc"].append(sum(c.values()))
                t["plan"].append(d["defrag_plan_kernels"])
                t["copy"].append(d["defrag_copy_kernel"])
        fill_bytes = 16 * npieces + 4 * nfrag
        dst = torch.empty(fill_bytes, dtype=torch.uint8, device="cuda")
        t_fill = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.fill_(0x5A)
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                t_fill.append(1e3 * e0.elapsed_time(e1))
        tables = 2 * 8 * (n + 1) + 4 * n
        print(f"bytes written  vectored: onc_encode_iov {hdr_bytes + 36 * n} (headers, entries, statuses) + "
              f"onc_fragment_iov {fill_bytes + tables + 16 * (n + 1)} ({16 * npieces} pieces, {4 * nfrag} marks, "
              f"tables and scratch)", flush=True)
        print(f"bytes written  packed:   onc_encode {total + 8 * (n + 1) + 8 * n} + onc_fragment "
              f"{need + 8 * (n + 1) + 4 * n + 8 * (n + 1)}", flush=True)
        print(f"onc_fragment_iov plan (3 launches)       us: {stats(t['plan_iov'])}", flush=True)
        print(f"onc_fragment_iov fill kernel             us: {stats(t['fill_iov'])}   {fill_bytes} bytes written, "
              f"{fill_bytes / np.median(t['fill_iov']) / 1e3:.0f} GB/s", flush=True)
        print(f"device fill of {fill_bytes} bytes      us: {stats(t_fill)}   "
              f"{fill_bytes / np.median(t_fill) / 1e3:.0f} GB/s; fill kernel / floor: "
              f"{np.median(t['fill_iov']) / np.median(t_fill):.2f}", flush=True)
        print(f"onc_fragment plan (3 launches)           us: {stats(t['plan'])}", flush=True)
        print(f"onc_fragment copy kernel                 us: {stats(t['copy'])}", flush=True)
        v_frag = np.array(t["plan_iov"]) + np.array(t["fill_iov"])
        p_frag = np.array(t["plan"]) + np.array(t["copy"])
        print(f"fragmenting    vectored plan + fill      us: {stats(v_frag)}", flush=True)
        print(f"fragmenting    packed plan + copy        us: {stats(p_frag)}   packed / vectored: "
              f"{np.median(p_frag) / np.median(v_frag):.1f}", flush=True)
        v_all = v_frag + np.array(t["enc_iov"])
        p_all = p_frag + np.array(t["enc"])
        print(f"onc_encode_iov (all launches)            us: {stats(t['enc_iov'])}", flush=True)
        print(f"onc_encode (all launches)                us: {stats(t['enc'])}", flush=True)
        print(f"whole path     onc_encode_iov + onc_fragment_iov us: {stats(v_all)}", flush=True)
        print(f"whole path     onc_encode + onc_fragment         us: {stats(p_all)}   packed / vectored: "
              f"{np.median(p_all) / np.median(v_all):.1f}", flush=True)
        del out, marks, pieces, dst
    codec.close()


if __name__ == "__main__":
    main()
