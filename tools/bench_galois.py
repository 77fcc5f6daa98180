#!/usr/bin/env python3
"""Times fhe_ct_galois_batch and fhe_ct_trace_batch against the chains of older
entry points whose words they reproduce.

Shapes: N = 16384 with q = 132120577 (32-bit lanes; base 2^9, 3 levels) and with
the 62-bit prime (base 2^21, 3 levels), N = 4096 with the 62-bit prime (base
2^16, 4 levels); batch 8192, 64 and 1; g = 3, n + 1 and 2n - 1; device-resident
data, random words below q, add_input = 0.  Legs, all in one process:

  fused   fhe_ct_galois_batch
  chain   fhe_poly_galois_batch over both components (one call, 2 * batch rows),
          two strided device copies of the rows into ct3 = (sigma(c0), 0,
          sigma(c1)) -- the entry point writes contiguous rows only --, and
          fhe_relinearize_batch
  relin   fhe_relinearize_batch alone on that ct3: the same transforms and key
          products, so it is the floor of the fused call
  sigma   fhe_poly_galois_batch alone (2 * batch rows read and written once:
          `sigma_gbs` is 2 * batch * n * 16 bytes over its time)

and once per shape and batch the trace:

  trace        fhe_ct_trace_batch, all log2(n) steps
  trace_chain  fhe_poly_mul_scalar_batch and log2(n) calls of
               fhe_ct_galois_batch (add_input = 1) through two buffers

Times are hipEvent spans on the context's stream over `reps` back-to-back calls,
after warm-up, the legs in alternating windows; a repeat is `windows` windows per
leg and yields one median per leg; the figure is the median of the repeats'
medians and `chain_spread_ms` is max - min of the chain's.  One JSON line per
row, then one summary line with the build id and the rows where the fused call
was slower than its chain.
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
# name -> (n, q, base_log, level)
SHAPES = {"16384x27": (16384, P27, 9, 3), "16384x62": (16384, P62, 21, 3), "4096x62": (4096, P62, 16, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batches", default="8192,64,1")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_galois.py needs a GPU")
    L = fhe_gpu.lib()
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    rows = []
    for name in args.shapes.split(","):
        n, q, bl, lv = SHAPES[name]
        steps = n.bit_length() - 1
        ring = fhe_gpu.PolynomialRing(n, q, mode="negacyclic", device=0)
        ring._bind_stream(DEV)
        h = ring._h
        stream = L.fhe_ctx_stream(h)
        gen = torch.Generator(device=dev).manual_seed(n)
        new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
        rand = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)
        keys = new(steps, lv, 2, n)
        check(L.fhe_relin_key_prepare(h, steps * lv, rand(steps, lv, 2, n).data_ptr(), keys.data_ptr(), DEV))
        inv = pow(pow(2, steps, q), -1, q)

        def span(fn, reps):
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            return e0.elapsed_ms(e1) / reps

        def measure(legs):
            """{leg: median ms}, the chain's spread, and the reps per leg."""
            reps = {}
            for k, fn in legs.items():
                for _ in range(args.warmup):
                    fn()
                check(L.fhe_ctx_synchronize(h))
                reps[k] = max(1, min(500, int(args.target_ms / max(span(fn, 1), 1e-3))))
            meds = {k: [] for k in legs}
            for _ in range(args.repeats):
                spans = {k: [] for k in legs}
                for _ in range(args.windows):  # alternate the legs
                    for k, fn in legs.items():
                        spans[k].append(span(fn, reps[k]))
                for k in meds:
                    meds[k].append(statistics.median(spans[k]))
            return {k: statistics.median(v) for k, v in meds.items()}, {k: max(v) - min(v) for k, v in meds.items()}, reps

        for batch in [int(b) for b in args.batches.split(",")]:
            ct, fo, co, ro = rand(batch, 2, n), new(batch, 2, n), new(batch, 2, n), new(batch, 2, n)
            sig = new(batch, 2, n)
            ct3 = torch.zeros(batch, 3, n, dtype=torch.int64, device=dev)
            base = {"n": n, "q": q, "base_log": bl, "level": lv, "batch": batch}
            for g in (3, n + 1, 2 * n - 1):
                def fused():
                    check(L.fhe_ct_galois_batch(h, bl, lv, g, keys.data_ptr(), ct.data_ptr(), 0, fo.data_ptr(), batch, DEV))

                def chain():
                    check(L.fhe_poly_galois_batch(h, g, ct.data_ptr(), sig.data_ptr(), 2 * batch, DEV))
                    ct3[:, 0].copy_(sig[:, 0])
                    ct3[:, 2].copy_(sig[:, 1])
                    check(L.fhe_relinearize_batch(h, bl, lv, ct3.data_ptr(), keys.data_ptr(), co.data_ptr(), batch, DEV))

                def relin():
                    check(L.fhe_relinearize_batch(h, bl, lv, ct3.data_ptr(), keys.data_ptr(), ro.data_ptr(), batch, DEV))

                def sigma():
                    check(L.fhe_poly_galois_batch(h, g, ct.data_ptr(), sig.data_ptr(), 2 * batch, DEV))

                ms, spread, reps = measure({"fused": fused, "chain": chain, "relin": relin, "sigma": sigma})
                torch.cuda.synchronize()
                assert torch.equal(fo, co), f"the key switch differs from its chain at {name} batch {batch} g {g}"
                row = dict(base, leg="galois", g=g, fused_ms=round(ms["fused"], 5), chain_ms=round(ms["chain"], 5),
                           relin_ms=round(ms["relin"], 5), sigma_ms=round(ms["sigma"], 5),
                           sigma_gbs=round(2 * batch * n * 16 / ms["sigma"] / 1e6, 1),
                           chain_over_fused=round(ms["chain"] / ms["fused"], 3),
                           fused_over_relin=round(ms["fused"] / ms["relin"], 3), chain_spread_ms=round(spread["chain"], 5),
                           fused_not_slower=bool(ms["fused"] <= ms["chain"] + spread["chain"]), reps=list(reps.values()),
                           windows=args.windows, repeats=args.repeats, build_id=fhe_gpu.build_id())
                rows.append(row)
                print(json.dumps(row), flush=True)
            if not args.no_trace:
                pong = [new(batch, 2, n), new(batch, 2, n)]

                def trace():
                    check(L.fhe_ct_trace_batch(h, bl, lv, steps, keys.data_ptr(), ct.data_ptr(), fo.data_ptr(), batch, DEV))

                def trace_chain():
                    check(L.fhe_poly_mul_scalar_batch(h, ct.data_ptr(), inv, pong[0].data_ptr(), 2 * batch, DEV))
                    for i in range(steps):
                        dst = co if i + 1 == steps else pong[(i + 1) & 1]
                        check(L.fhe_ct_galois_batch(h, bl, lv, (n >> i) + 1, keys[i].data_ptr(), pong[i & 1].data_ptr(), 1,
                                                    dst.data_ptr(), batch, DEV))

                ms, spread, reps = measure({"fused": trace, "chain": trace_chain})
                torch.cuda.synchronize()
                assert torch.equal(fo, co), f"the trace differs from its chain at {name} batch {batch}"
                row = dict(base, leg="trace", steps=steps, fused_ms=round(ms["fused"], 5), chain_ms=round(ms["chain"], 5),
                           chain_over_fused=round(ms["chain"] / ms["fused"], 3), chain_spread_ms=round(spread["chain"], 5),
                           fused_not_slower=bool(ms["fused"] <= ms["chain"] + spread["chain"]), reps=list(reps.values()),
                           windows=args.windows, repeats=args.repeats, build_id=fhe_gpu.build_id())
                rows.append(row)
                print(json.dumps(row), flush=True)
                del pong
            del ct, fo, co, ro, sig, ct3
            torch.cuda.empty_cache()
        del keys
        torch.cuda.empty_cache()
    losers = [(r["leg"], r["n"], r["q"], r["batch"], r.get("g")) for r in rows if not r["fused_not_slower"]]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "slower_than_chain": losers}), flush=True)


if __name__ == "__main__":
    main()
