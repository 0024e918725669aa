"""Kernel time of writing a fragmented send stream as bytes by gathering the
vectored encode's pieces (onc_piece_offsets + onc_gather_pieces) against the
packed path, on configs[2].

configs[2]'s batch (1M mixed Call/Reply records, payloads 64..4096 B: the
bench's c2 workload) is turned into the same fragmented byte stream in two
ways, on the same batch, in one process, the paths alternated per repetition:

  (a) packed:   onc_encode (every byte), then onc_fragment (every byte again);
  (b) gathered: onc_encode_iov (headers only), onc_fragment_iov (marks and a
      list of pieces), onc_piece_offsets (the pieces' stream positions), then
      onc_gather_pieces over the whole stream (every byte once);
  (c) the gather kernel alone against a device copy (torch copy_) of as many
      bytes, timed by events in the same run, and against onc_fragment's copy
      kernel at the same max_frag.

max_frag: 1024 (most records become 2..5 fragments) and 8192 (no configs[2]
record is split), alternating. Kernel times are the dispatch timestamps
(Codec.enable_timing / kernel_stats), medians and min-max over --reps
repetitions after --warmup. A window of the stream (--window bytes from the
middle) is timed too: the shape a sender with a bounded ring uses.

The outputs are checked first: the gathered stream equals onc_fragment's
output byte for byte, on the device.

    python tools/gather_timing.py [--records N] [--reps 7] [--warmup 2] [--sizes 1024,8192] [--window 1048576]
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


def stats(us):
    a = np.array(us)
    return f"median {np.median(a):8.2f}  min {a.min():8.2f}  max {a.max():8.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024,8192")
    ap.add_argument("--window", type=int, default=1 << 20)
    args = ap.parse_args()
    import torch

    n = args.records
    hb = S.mixed(n, seed=2)
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
    hdr_bytes = int(tot.cpu()[0])
    assert np.array_equal(hl + pl, lens) and int(tot.cpu()[1]) == total
    print(f"configs[2]: {n} mixed records, {total} wire bytes of which {hdr_bytes} header bytes; {args.reps} timed "
          f"repetitions after {args.warmup} warm-up, the paths and the sizes alternated", flush=True)

    def device_us(call):
        """Device time of every launch of one call, by kernel id."""
        codec.reset_stats()
        call()
        codec.sync()
        return {k: 1e3 * v[0] for k, v in codec.kernel_stats().items()}

    codec.enable_timing(True)
    codec.reserve(n)
    sizes = [int(x) for x in args.sizes.split(",")]
    work = {}
    for size in sizes:
        Hb, B = hl - 4, lens - 4
        k = np.maximum(1, -(-B // size))
        x = ((Hb % size != 0) & (pl > 0)).astype(np.int64)
        e = np.where(B == 0, 1, 2 * k + x)
        nfrag, need, npieces = int(k.sum()), int((B + 4 * k).sum()), int(e.sum())
        w = {"size": size, "nfrag": nfrag, "need": need, "npieces": npieces}
        w["out"] = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        w["gout"] = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        w["o_off"] = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        w["o_st"] = torch.zeros(n, dtype=torch.int32, device="cuda")
        w["o_res"] = torch.zeros(3, dtype=torch.int64, device="cuda")
        w["marks"] = torch.zeros(4 * nfrag, dtype=torch.uint8, device="cuda")
        w["pieces"] = torch.zeros(16 * npieces, dtype=torch.uint8, device="cuda")
        w["v_off"] = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        w["p_off"] = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        w["v_st"] = torch.zeros(n, dtype=torch.int32, device="cuda")
        w["v_res"] = torch.zeros(4, dtype=torch.int64, device="cuda")
        w["pos"] = torch.zeros(npieces + 1, dtype=torch.int64, device="cuda")
        w["g_res"] = torch.zeros(3, dtype=torch.int64, device="cuda")
        w["src"] = R.gather_src(w["marks"], (hdr, hdr_bytes), db.payload_arena)
        w["t"] = {name: [] for name in ("enc", "fplan", "fcopy", "enc_iov", "vplan", "vfill", "goff", "gcopy", "gwin",
                                        "memcpy")}
        work[size] = w

    def fragment(w):
        codec.fragment(wire, off, n, w["size"], w["out"], w["o_off"], w["o_st"], w["o_res"], out_cap=w["need"])

    def fragment_iov(w):
        codec.fragment_iov(d_iov, n, w["size"], w["marks"], w["pieces"], w["v_off"], w["p_off"], w["v_st"], w["v_res"],
                           marks_cap=4 * w["nfrag"], max_pieces=w["npieces"])

    def offsets(w):
        codec.piece_offsets(w["pieces"], w["npieces"], w["src"], w["pos"], w["g_res"])

    def gather(w):
        codec.gather_pieces(w["pieces"], w["pos"], w["npieces"], w["src"], 0, w["need"], w["gout"])

    def gather_window(w):
        codec.gather_pieces(w["pieces"], w["pos"], w["npieces"], w["src"], w["need"] // 2 + 5, args.window, w["gout"])

    for w in work.values():                          # the check
        fragment(w)
        fragment_iov(w)
        offsets(w)
        gather(w)
        codec.sync()
        assert w["o_res"].cpu().numpy().tolist()[:2] == [w["nfrag"], w["need"]]
        assert w["g_res"].cpu().numpy().tolist() == [w["need"], 0, w["npieces"]]
        assert torch.equal(w["gout"], w["out"]), "the gathered stream differs from onc_fragment's bytes"
        print(f"-- max_frag {w['size']}: {w['nfrag']} fragments, {w['need']} stream bytes, {w['npieces']} pieces; "
              f"checked: the gathered stream equals onc_fragment's output byte for byte", flush=True)

    for rep in range(args.warmup + args.reps):
        for w in work.values():
            a, b = device_us(encode), device_us(lambda: fragment(w))
            c, d = device_us(encode_iov), device_us(lambda: fragment_iov(w))
            f, g = device_us(lambda: offsets(w)), device_us(lambda: gather(w))
            h = device_us(lambda: gather_window(w))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            w["gout"][:w["need"]].copy_(w["out"][:w["need"]])
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                t = w["t"]
                t["enc"].append(sum(a.values()))
                t["fplan"].append(b["defrag_plan_kernels"])
                t["fcopy"].append(b["defrag_copy_kernel"])
                t["enc_iov"].append(sum(c.values()))
                t["vplan"].append(d["defrag_plan_kernels"])
                t["vfill"].append(d["defrag_copy_kernel"])
                t["goff"].append(f["defrag_plan_kernels"])
                t["gcopy"].append(g["defrag_copy_kernel"])
                t["gwin"].append(h["defrag_copy_kernel"])
                t["memcpy"].append(1e3 * e0.elapsed_time(e1))

    for w in work.values():
        t = {k: np.array(v) for k, v in w["t"].items()}
        need = w["need"]
        print(f"== max_frag {w['size']} ({need} stream bytes, {w['npieces']} pieces)", flush=True)
        pa = t["enc"] + t["fplan"] + t["fcopy"]
        pb = t["enc_iov"] + t["vplan"] + t["vfill"] + t["goff"] + t["gcopy"]
        print(f"(a) onc_encode (all launches)              us: {stats(t['enc'])}", flush=True)
        print(f"(a) onc_fragment plan + copy               us: {stats(t['fplan'] + t['fcopy'])}", flush=True)
        print(f"(a) packed chain                           us: {stats(pa)}", flush=True)
        print(f"(b) onc_encode_iov (all launches)          us: {stats(t['enc_iov'])}", flush=True)
        print(f"(b) onc_fragment_iov plan + fill           us: {stats(t['vplan'] + t['vfill'])}", flush=True)
        print(f"(b) onc_piece_offsets (3 launches)         us: {stats(t['goff'])}", flush=True)
        print(f"(b) onc_gather_pieces, the whole stream    us: {stats(t['gcopy'])}   "
              f"{need / np.median(t['gcopy']) / 1e3:.0f} GB/s written", flush=True)
        print(f"(b) gathered chain                         us: {stats(pb)}   packed / gathered: "
              f"{np.median(pa) / np.median(pb):.2f}", flush=True)
        print(f"(c) gather_copy                            us: {stats(t['gcopy'])}", flush=True)
        print(f"(c) device copy of {need} bytes     us: {stats(t['memcpy'])}   gather_copy / copy: "
              f"{np.median(t['gcopy']) / np.median(t['memcpy']):.2f}", flush=True)
        print(f"(c) frag_copy (onc_fragment's copy kernel) us: {stats(t['fcopy'])}   gather_copy / frag_copy: "
              f"{np.median(t['gcopy']) / np.median(t['fcopy']):.2f}", flush=True)
        print(f"    gather of a {args.window}-byte window from the middle us: {stats(t['gwin'])}", flush=True)
    codec.close()


if __name__ == "__main__":
    main()
