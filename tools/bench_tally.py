#!/usr/bin/env python3
"""Times the single-launch ciphertext tally against the chain of additions.

Shape: N = 16384, q = 132120577, polys = 2, one group, device-resident data,
count ballots (default 64, 1024, 4096).  Legs:

  sum    fhe_ct_sum_batch over the contiguous [count][2][N] buffer
  ptrs   fhe_ct_sum_ptrs over a table of the same ballots in shuffled order
  chain  count - 1 fhe_poly_add_batch calls, each over one ciphertext, the
         running sum ping-ponging between two buffers: what a host loop of
         add() (the engine's former batchAdd) launches, without its
         allocations.  Uses only entry points older builds have, so the same
         script times the baseline on another build:

           FHE_GPU_LIB=/path/to/older/libfhe_gpu.so python tools/bench_tally.py --legs chain

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up; each leg is timed in `windows` windows and reports
their minimum and median.  The read bandwidth of a sum is count * 2N * 8
bytes over its time.  One JSON line per (count, leg), then a summary line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "node-fhe-accelerate_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, Q, POLYS = 16384, 132120577, 2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--counts", default="64,1024,4096")
    ap.add_argument("--legs", default="sum,ptrs,chain")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=40.0, help="device time aimed at per window")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_tally.py needs a GPU")
    L = fhe_gpu.lib()
    legs = args.legs.split(",")
    if ("sum" in legs or "ptrs" in legs) and not hasattr(L, "fhe_ct_sum_batch"):
        sys.exit("this build has no fhe_ct_sum_batch: run it with --legs chain")
    ring = fhe_gpu.PolynomialRing(N, Q, device=0)
    ring._bind_stream(fhe_gpu.FHE_DEVICE)
    h = ring._h
    stream = L.fhe_ctx_stream(h)
    words = POLYS * N
    dev = torch.device("cuda:0")

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    def timed(fn, reps):
        for _ in range(args.warmup):
            fn()
        check(L.fhe_ctx_synchronize(h))
        spans = []
        for _ in range(args.windows):
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            spans.append(e0.elapsed_ms(e1) / reps)
        return min(spans), statistics.median(spans)

    results = {}
    for count in [int(c) for c in args.counts.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(count)
        cts = torch.randint(0, Q, (count, POLYS, N), dtype=torch.int64, device=dev, generator=gen)
        out = {leg: torch.empty((POLYS, N), dtype=torch.int64, device=dev) for leg in ("sum", "ptrs", "chain", "tmp")}
        base = cts.data_ptr()
        order = torch.randperm(count, generator=torch.Generator().manual_seed(1)).tolist()
        table = (C.c_void_p * count)(*[base + 8 * words * i for i in order])
        nbytes = count * words * 8

        def run_sum():
            check(L.fhe_ct_sum_batch(h, base, POLYS, count, 1, 0, out["sum"].data_ptr(), fhe_gpu.FHE_DEVICE))

        def run_ptrs():
            check(L.fhe_ct_sum_ptrs(h, table, POLYS, count, 0, out["ptrs"].data_ptr()))

        def run_chain():
            # the last addition lands in out["chain"]
            bufs = [out["tmp"].data_ptr(), out["chain"].data_ptr()]
            acc = base
            for i in range(1, count):
                dst = bufs[(count - 1 - i) % 2 == 0]
                check(L.fhe_poly_add_batch(h, acc, base + 8 * words * i, dst, POLYS, fhe_gpu.FHE_DEVICE))
                acc = dst

        runs = {"sum": run_sum, "ptrs": run_ptrs, "chain": run_chain}
        for leg in legs:
            # one call's time sizes the window
            runs[leg]()
            check(L.fhe_ctx_synchronize(h))
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            runs[leg]()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            reps = max(2, min(2000, int(args.target_ms / max(e0.elapsed_ms(e1), 1e-3))))
            lo, med = timed(runs[leg], reps)
            rec = {"count": count, "leg": leg, "reps": reps, "windows": args.windows, "ms_min": round(lo, 5),
                   "ms_median": round(med, 5), "read_GBps_median": round(nbytes / med / 1e6, 1),
                   "build_id": fhe_gpu.build_id()}
            results[(count, leg)] = rec
            print(json.dumps(rec), flush=True)
        torch.cuda.synchronize()
        done = [leg for leg in legs if leg in out]
        for leg in done[1:]:
            assert torch.equal(out[leg], out[done[0]]), f"{leg} and {done[0]} differ at count {count}"
        del cts

    summary = {"shape": {"n": N, "q": Q, "polys": POLYS, "groups": 1}, "device": torch.cuda.get_device_name(0)}
    for count in sorted({c for c, _ in results}):
        row = {leg: results[(count, leg)]["ms_median"] for leg in legs if (count, leg) in results}
        if "chain" in row:
            for leg in ("sum", "ptrs"):
                if leg in row:
                    row[f"chain_over_{leg}"] = round(row["chain"] / row[leg], 2)
        summary[str(count)] = row
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
