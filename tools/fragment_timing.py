"""Kernel time of send-side fragmentation (onc_fragment) on configs[2]'s wire.

configs[2]'s batch (1M mixed Call/Reply records, payloads 64..4096 B: the
bench's c2 workload) is encoded on the device, then cut by onc_fragment the
way a sender flushing a fixed buffer does. max_frag: 8192 (every configs[2]
record is shorter: no record is split, so this measures the entry points
alone) and 1024 (most records become 2..5 fragments). Per max_frag, in one
process, from the dispatch timestamps (Codec.enable_timing / kernel_stats),
medians and min-max over --reps repetitions:

  * onc_fragment's plan (three launches) and its copy kernel: time, bytes
    moved (bodies read + fragments written) and the rate;
  * a device-to-device hipMemcpyAsync (torch copy_) of as many bytes as the
    copy writes, timed by events in the same run;
  * onc_defragment's copy kernel on the stream just produced (the inverse
    copy, which finds every fragment by search), with its rate.

The outputs are checked first: out_off and result against the closed form
computed from the record lengths, and onc_frame_fragments + onc_defragment of
the output against the unfragmented wire, byte for byte.

    python tools/fragment_timing.py [--records N] [--reps 7] [--warmup 2] [--sizes 8192,1024]
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
    rec_len = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    codec.encode_lengths(db, rec_len, st)
    codec.sync()
    lens = rec_len.cpu().numpy().view(np.uint32).astype(np.int64)
    total = int(lens.sum())
    wire = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    codec.encode(db, wire, off, st, rec_len)
    codec.sync()
    assert int((st != 0).sum()) == 0
    del db
    print(f"configs[2]: {n} mixed records, {total} wire bytes; {args.reps} timed repetitions after {args.warmup} "
          f"warm-up", flush=True)

    def timed(call, ids):
        """us per repetition and id: the launches under each id of `ids`."""
        per = {k: [] for k in ids}
        for rep in range(args.warmup + args.reps):
            codec.reset_stats()
            call()
            codec.sync()
            ks = codec.kernel_stats()
            if rep >= args.warmup:
                for k in ids:
                    per[k].append(1e3 * ks[k][0])
        return per

    codec.enable_timing(True)
    ids = ("defrag_plan_kernels", "defrag_copy_kernel")
    for size in (int(x) for x in args.sizes.split(",")):
        k = np.maximum(1, -(-(lens - 4) // size))
        out_len = lens - 4 + 4 * k
        nfrag, need, multi = int(k.sum()), int(out_len.sum()), int((k > 1).sum())
        codec.reserve(max(n, nfrag))
        print(f"-- max_frag {size}: {nfrag} fragments, {multi} records of more than one, {need} output bytes",
              flush=True)
        out = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        o_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        o_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        o_res = torch.zeros(3, dtype=torch.int64, device="cuda")
        per = timed(lambda: codec.fragment(wire, off, n, size, out, o_off, o_st, o_res, out_cap=need), ids)
        assert o_res.cpu().numpy().tolist() == [nfrag, need, multi]
        assert np.array_equal(o_off.cpu().numpy(), np.concatenate(([0], np.cumsum(out_len))))
        assert int((o_st != 0).sum()) == 0 and int((out[need:] != 0xA5).sum()) == 0
        t_plan, t_copy = per["defrag_plan_kernels"], per["defrag_copy_kernel"]

        # back through the receive side: the check, and the inverse copy's time
        d_fo = torch.zeros(nfrag + 2, dtype=torch.int64, device="cuda")
        fres = torch.zeros(5, dtype=torch.int64, device="cuda")
        codec.frame_fragments(out, need, d_fo, nfrag + 1, fres)
        codec.sync()
        assert fres.cpu().numpy().tolist()[:3] == [nfrag, need, 0]
        back = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        b_off = torch.zeros(nfrag + 1, dtype=torch.int64, device="cuda")
        b_st = torch.zeros(nfrag, dtype=torch.int32, device="cuda")
        b_res = torch.zeros(6, dtype=torch.int64, device="cuda")
        per = timed(lambda: codec.defragment(out, d_fo, nfrag, back, b_off, b_st, b_res, out_cap=total),
                    ("defrag_copy_kernel",))
        assert b_res.cpu().numpy().tolist() == [n, need, total, 0, 0, multi]
        assert torch.equal(back[:total], wire[:total]) and torch.equal(b_off[:n + 1], off)
        t_inv = per["defrag_copy_kernel"]
        del back, b_off, b_st, d_fo

        dst = torch.empty(need, dtype=torch.uint8, device="cuda")
        t_cp = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(out[:need])
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                t_cp.append(1e3 * e0.elapsed_time(e1))
        moved = (total - 4 * n) + need                # bodies read + fragments written
        moved_inv = (need - 4 * nfrag) + total        # bodies read + records written
        r_copy = moved / np.median(t_copy) / 1e3
        r_inv = moved_inv / np.median(t_inv) / 1e3
        r_cp = 2 * need / np.median(t_cp) / 1e3
        print(f"onc_fragment plan (3 launches)           us: {stats(t_plan)}", flush=True)
        print(f"onc_fragment copy kernel                 us: {stats(t_copy)}   {moved} bytes moved, {r_copy:.0f} GB/s",
              flush=True)
        print(f"device-to-device copy of {need} bytes us: {stats(t_cp)}   {2 * need} bytes moved, {r_cp:.0f} GB/s",
              flush=True)
        print(f"  copy kernel rate / memcpy rate: {r_copy / r_cp:.2f} "
              f"(min-max {moved / max(t_copy) / (2 * need / min(t_cp)):.2f} .. "
              f"{moved / min(t_copy) / (2 * need / max(t_cp)):.2f})", flush=True)
        print(f"onc_defragment copy kernel on that stream us: {stats(t_inv)}   {moved_inv} bytes moved, "
              f"{r_inv:.0f} GB/s = {r_inv / r_cp:.2f} of memcpy", flush=True)
        del out, dst
    codec.close()


if __name__ == "__main__":
    main()
