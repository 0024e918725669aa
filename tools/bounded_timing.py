"""Kernel time of the bounded lengths decode against the unbounded one.

configs[2]'s batch (1M mixed Call/Reply records, payloads 64..4096 B: the
bench's c2 workload) decoded by onc_decode_lengths and by
onc_decode_lengths_bounded with the exact wire length, alternating in one
process; the decode kernel's own time (ONC_K_DEC_PARSE, from the dispatch
timestamps: Codec.enable_timing / kernel_stats). Two cache states as in
bench.py: warm (the same wire every repetition) and cold (identical wire
copies in rotation, so a header line is re-read only after more than the
Infinity Cache of other reads). Prints medians and min-max in microseconds.

    python tools/bounded_timing.py [--records N] [--reps 30] [--warmup 5] [--copies 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copies", type=int, default=5)
    args = ap.parse_args()
    import torch

    n = args.records
    hb = S.mixed(n, seed=2)
    db = R.DeviceBatch.from_host(hb, "cuda")
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
    dec = R.DecodeBuffers(n)
    out = (dec.msgs, dec.unix, dec.status, dec.aux0, dec.aux1)
    codec.enable_timing(True, kernels=[R.K_DEC_PARSE])

    def once(w, bounded):
        codec.reset_stats()
        if bounded:
            codec.decode_lengths_bounded(w, total, rec_len, n, 0, L.DECODE_SLICE, *out)
        else:
            codec.decode_lengths(w, rec_len, n, 0, L.DECODE_SLICE, *out)
        codec.sync()
        ms, cnt = codec.kernel_stats()["decode_kernel"]
        assert cnt == 1
        return 1e3 * ms

    print(f"configs[2]: {n} mixed records, {total} wire bytes, slice mode, {args.reps} timed repetitions per form "
          f"after {args.warmup} warm-up, the two forms alternating", flush=True)
    for state in ("warm", "cold"):
        wires = [wire] if state == "warm" else [wire] + [wire.clone() for _ in range(args.copies - 1)]
        t = {False: [], True: []}
        k = 0
        for rep in range(args.warmup + args.reps):
            for bounded in (False, True):
                us = once(wires[k % len(wires)], bounded)
                k += 1
                if rep >= args.warmup:
                    t[bounded].append(us)
            if rep == 0:
                # same results from both forms on good input
                s = dec.status.clone()
                once(wires[0], False)
                assert torch.equal(s, dec.status) and int((s != 0).sum()) == 0
        for bounded in (False, True):
            a = np.array(t[bounded])
            print(f"{state:4s} {'bounded  ' if bounded else 'unbounded'} decode_kernel us: median {np.median(a):7.2f}  "
                  f"min {a.min():7.2f}  max {a.max():7.2f}", flush=True)
        d = np.median(t[True]) - np.median(t[False])
        spread = max(t[False]) - min(t[False])
        print(f"{state:4s} bounded - unbounded (medians): {d:+.2f} us; unbounded min-max spread {spread:.2f} us "
              f"({'inside' if abs(d) <= spread else 'OUTSIDE'} the spread)", flush=True)
        del wires
    codec.close()


if __name__ == "__main__":
    main()
