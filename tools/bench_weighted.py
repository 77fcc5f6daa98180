#!/usr/bin/env python3
"""Times the public-weight tallies against the chains of older entry points.

Shape: the tally workload's (N = 16384, one group, device-resident data), at
q = 132120577 (32-bit lanes) and q = 4611686018326724609 (64-bit lanes), count
ballots (default 64, 1024, 4096).  Pairs of legs, each fused call against the
chain whose words it reproduces:

  scaled           fhe_ct_sum_scaled_batch over [count][2][N] and [count]
  scaled_chain     fhe_poly_mul_scalar_batch per ballot into [count][2][N],
                   then fhe_ct_sum_batch (polys = 2): count + 1 launches
  sum              fhe_ct_sum_batch over the same ballots (another result: the
                   unweighted tally): the same bytes without the products, so
                   scaled over sum is what the arithmetic costs
  plain            fhe_ct_dot_plain_batch over [count][2][N] and [count][N]
  plain_chain      ONE fhe_polymul_batch of the 2 count components with the
                   plaintext replicated per component (built outside the timed
                   window: the chain is not charged for it) into [count][2][N],
                   then fhe_ct_sum_batch
  plain_ntt        fhe_ct_dot_plain_batch with is_ntt
  plain_ntt_chain  fhe_ntt_fwd_batch of the replicated plaintexts,
                   fhe_pointwise_batch, then fhe_ct_sum_batch

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up.  The legs of a pair are timed in alternating windows
of the same process; each reports the minimum and the median of its windows.
bytes/s is the mandatory traffic (one read of every ballot; for the plain dot
also of every plaintext) over the median time -- an end-to-end figure of the
call, not a kernel's share of peak.  FHE_TALLY_SPLIT / FHE_DOT_SPLIT in the
environment force the slices of the fused calls.  One JSON line per (q, count,
leg), then a summary line.
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

P27, P62 = 132120577, 4611686018326724609
PAIRS = [("scaled", "scaled_chain", "sum"), ("plain", "plain_chain"), ("plain_ntt", "plain_ntt_chain")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--moduli", default=f"{P27},{P62}")
    ap.add_argument("--counts", default="64,1024,4096")
    ap.add_argument("--pairs", default="scaled,plain,plain_ntt")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=40.0, help="device time aimed at per window")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_weighted.py needs a GPU")
    L = fhe_gpu.lib()
    n = args.n
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE
    pairs = [p for p in PAIRS if p[0] in args.pairs.split(",")]

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    results = {}
    for q in [int(x) for x in args.moduli.split(",")]:
        ring = fhe_gpu.PolynomialRing(n, q, device=0)
        ring._bind_stream(DEV)
        h = ring._h
        stream = L.fhe_ctx_stream(h)

        def span(fn, reps):
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            return e0.elapsed_ms(e1) / reps

        for count in [int(c) for c in args.counts.split(",")]:
            gen = torch.Generator(device=dev).manual_seed(count)
            cts = torch.randint(0, q, (count, 2, n), dtype=torch.int64, device=dev, generator=gen)
            pts = torch.randint(0, q, (count, n), dtype=torch.int64, device=dev, generator=gen)
            scal = torch.randint(0, q, (count,), dtype=torch.int64, device=dev, generator=gen)
            hscal = [int(x) for x in scal.cpu().tolist()]
            ptb = pts.unsqueeze(1).expand(count, 2, n).contiguous()  # the chain's replicated plaintexts
            tmp = torch.empty((count, 2, n), dtype=torch.int64, device=dev)
            tmp2 = torch.empty((count, 2, n), dtype=torch.int64, device=dev)
            outs = {leg: torch.empty((2, n), dtype=torch.int64, device=dev) for pr in PAIRS for leg in pr}
            pc, pp, ps, pb, pt, pt2 = (x.data_ptr() for x in (cts, pts, scal, ptb, tmp, tmp2))
            ct_bytes = 2 * n * 8

            def run_scaled():
                check(L.fhe_ct_sum_scaled_batch(h, pc, ps, 2, count, 1, 0, outs["scaled"].data_ptr(), DEV))

            def run_scaled_chain():
                for i in range(count):
                    check(L.fhe_poly_mul_scalar_batch(h, pc + i * ct_bytes, hscal[i], pt + i * ct_bytes, 2, DEV))
                check(L.fhe_ct_sum_batch(h, pt, 2, count, 1, 0, outs["scaled_chain"].data_ptr(), DEV))

            def run_sum():
                check(L.fhe_ct_sum_batch(h, pc, 2, count, 1, 0, outs["sum"].data_ptr(), DEV))

            def run_plain():
                check(L.fhe_ct_dot_plain_batch(h, pc, pp, count, 1, 0, 0, outs["plain"].data_ptr(), DEV))

            def run_plain_chain():
                check(L.fhe_polymul_batch(h, pc, pb, pt, 2 * count, DEV))
                check(L.fhe_ct_sum_batch(h, pt, 2, count, 1, 0, outs["plain_chain"].data_ptr(), DEV))

            def run_plain_ntt():
                check(L.fhe_ct_dot_plain_batch(h, pc, pp, count, 1, 1, 0, outs["plain_ntt"].data_ptr(), DEV))

            def run_plain_ntt_chain():
                check(L.fhe_ntt_fwd_batch(h, pb, pt2, 2 * count, DEV))
                check(L.fhe_pointwise_batch(h, pc, pt2, pt, 2 * count, DEV))
                check(L.fhe_ct_sum_batch(h, pt, 2, count, 1, 0, outs["plain_ntt_chain"].data_ptr(), DEV))

            runs = {"scaled": run_scaled, "scaled_chain": run_scaled_chain, "sum": run_sum, "plain": run_plain,
                    "plain_chain": run_plain_chain, "plain_ntt": run_plain_ntt, "plain_ntt_chain": run_plain_ntt_chain}
            for pair in pairs:
                reps, spans = {}, {leg: [] for leg in pair}
                for leg in pair:
                    for _ in range(args.warmup):
                        runs[leg]()
                    check(L.fhe_ctx_synchronize(h))
                    reps[leg] = max(2, min(2000, int(args.target_ms / max(span(runs[leg], 1), 1e-3))))
                for _ in range(args.windows):  # alternate the legs
                    for leg in pair:
                        spans[leg].append(span(runs[leg], reps[leg]))
                torch.cuda.synchronize()
                assert torch.equal(outs[pair[0]], outs[pair[1]]), f"{pair} differ at q {q} count {count}"
                mandatory = count * (2 if pair[0] == "scaled" else 3) * n * 8
                for leg in pair:
                    med = statistics.median(spans[leg])
                    rec = {"q": q, "count": count, "leg": leg, "reps": reps[leg], "windows": args.windows,
                           "ms_min": round(min(spans[leg]), 5), "ms_median": round(med, 5),
                           "ballots_per_s": round(count / (med * 1e-3)),
                           "mandatory_GB_per_s": round(mandatory / (med * 1e-3) / 1e9, 1),
                           "build_id": fhe_gpu.build_id()}
                    results[(q, count, leg)] = rec
                    print(json.dumps(rec), flush=True)
            del cts, pts, ptb, tmp, tmp2

    summary = {"shape": {"n": n, "groups": 1}, "device": torch.cuda.get_device_name(0),
               "tally_split": os.environ.get("FHE_TALLY_SPLIT", ""), "dot_split": os.environ.get("FHE_DOT_SPLIT", ""),
               "build_id": fhe_gpu.build_id()}
    for (q, count) in sorted({(q, c) for q, c, _ in results}):
        row = {}
        for fused, chain, *rest in pairs:
            if (q, count, fused) in results:
                f, c = results[(q, count, fused)]["ms_median"], results[(q, count, chain)]["ms_median"]
                row[fused] = f
                row[chain] = c
                row[f"{chain}_over_{fused}"] = round(c / f, 2)
                for leg in rest:
                    row[leg] = results[(q, count, leg)]["ms_median"]
                    row[f"{fused}_over_{leg}"] = round(f / row[leg], 2)
        summary[f"{q}:{count}"] = row
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
