#!/usr/bin/env python3
"""Times the fused ciphertext inner product against the composed sequences.

Shape: N = 16384, q = 132120577, one group, device-resident data, count pairs
(default 64, 4096).  Legs:

  dot        fhe_ct_dot_batch over the contiguous [count][2][N] operands
  intent     fhe_ct_multiply_batch into [count][3][N], then fhe_ct_sum_batch
             (polys = 3): the composed degree-2 sum
  dot_relin  dot, then fhe_relinearize_batch of the one degree-2 sum
  full       multiply -> relinearize ([count][2][N]) -> sum (polys = 2): the
             relinearise-per-ballot fold of tally_weighted_votes

intent and full use only entry points older builds have, so the same script
times the baseline on another build:

  FHE_GPU_LIB=/path/to/older/libfhe_gpu.so python tools/bench_dot.py --legs intent,full

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up; each leg is timed in `windows` windows and reports
their minimum and median.  FHE_DOT_SPLIT in the environment forces the slices
of the fused call.  One JSON line per (count, leg), then a summary line with
the peak temporary memory of each path.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "node-fhe-accelerate_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

Q, BASE_LOG, LEVEL = 132120577, 7, 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--q", type=int, default=Q)
    ap.add_argument("--counts", default="64,4096")
    ap.add_argument("--legs", default="dot,intent,dot_relin,full")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=40.0, help="device time aimed at per window")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_dot.py needs a GPU")
    L = fhe_gpu.lib()
    legs = args.legs.split(",")
    if ("dot" in legs or "dot_relin" in legs) and not hasattr(L, "fhe_ct_dot_batch"):
        sys.exit("this build has no fhe_ct_dot_batch: run it with --legs intent,full")
    n, q = args.n, args.q
    ring = fhe_gpu.PolynomialRing(n, q, device=0)
    ring._bind_stream(fhe_gpu.FHE_DEVICE)
    h = ring._h
    stream = L.fhe_ctx_stream(h)
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE
    rlk = torch.randint(0, q, (LEVEL, 2, n), dtype=torch.int64, device=dev,
                        generator=torch.Generator(device=dev).manual_seed(5))
    ek = fhe_gpu.EvaluationKey(ring, rlk, BASE_LOG)
    key = ek.rlk_ntt.data_ptr()

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
        a = torch.randint(0, q, (count, 2, n), dtype=torch.int64, device=dev, generator=gen)
        b = torch.randint(0, q, (count, 2, n), dtype=torch.int64, device=dev, generator=gen)
        need3 = "intent" in legs or "full" in legs
        ct3 = torch.empty((count if need3 else 1, 3, n), dtype=torch.int64, device=dev)
        ct2 = torch.empty((count if "full" in legs else 1, 2, n), dtype=torch.int64, device=dev)
        d2 = {leg: torch.empty((3, n), dtype=torch.int64, device=dev) for leg in ("dot", "intent")}
        d1 = {leg: torch.empty((2, n), dtype=torch.int64, device=dev) for leg in ("dot_relin", "full")}
        pa, pb, p3, p2 = a.data_ptr(), b.data_ptr(), ct3.data_ptr(), ct2.data_ptr()

        def run_dot(out=d2["dot"]):
            check(L.fhe_ct_dot_batch(h, pa, pb, count, 1, 0, 0, out.data_ptr(), DEV))

        def run_intent():
            check(L.fhe_ct_multiply_batch(h, pa, pb, p3, count, 0, DEV))
            check(L.fhe_ct_sum_batch(h, p3, 3, count, 1, 0, d2["intent"].data_ptr(), DEV))

        def run_dot_relin():
            run_dot()
            check(L.fhe_relinearize_batch(h, BASE_LOG, LEVEL, d2["dot"].data_ptr(), key, d1["dot_relin"].data_ptr(), 1, DEV))

        def run_full():
            check(L.fhe_ct_multiply_batch(h, pa, pb, p3, count, 0, DEV))
            check(L.fhe_relinearize_batch(h, BASE_LOG, LEVEL, p3, key, p2, count, DEV))
            check(L.fhe_ct_sum_batch(h, p2, 2, count, 1, 0, d1["full"].data_ptr(), DEV))

        runs = {"dot": run_dot, "intent": run_intent, "dot_relin": run_dot_relin, "full": run_full}
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
                   "ms_median": round(med, 5), "us_per_pair_median": round(1e3 * med / count, 4),
                   "build_id": fhe_gpu.build_id()}
            results[(count, leg)] = rec
            print(json.dumps(rec), flush=True)
        torch.cuda.synchronize()
        if "dot" in legs and "intent" in legs:
            assert torch.equal(d2["dot"], d2["intent"]), f"dot and intent differ at count {count}"
        del a, b, ct3, ct2

    summary = {"shape": {"n": n, "q": q, "groups": 1, "base_log": BASE_LOG, "level": LEVEL},
               "device": torch.cuda.get_device_name(0), "dot_split": os.environ.get("FHE_DOT_SPLIT", "")}
    for count in sorted({c for c, _ in results}):
        row = {leg: results[(count, leg)]["ms_median"] for leg in legs if (count, leg) in results}
        if "dot" in row and "intent" in row:
            row["intent_over_dot"] = round(row["intent"] / row["dot"], 2)
        if "dot_relin" in row and "full" in row:
            row["full_over_dot_relin"] = round(row["full"] / row["dot_relin"], 2)
        # temporaries the caller (intent, full) or the library (dot) holds beside inputs and output
        row["temp_MiB"] = {"intent": round(count * 3 * n * 8 / 2**20, 1), "full": round(count * 5 * n * 8 / 2**20, 1)}
        summary[str(count)] = row
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
