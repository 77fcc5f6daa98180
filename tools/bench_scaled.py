#!/usr/bin/env python3
"""Times the scale-invariant BFV product (fhe_ct_multiply_scaled_batch,
fhe_ct_dot_scaled_batch) and its parts.

Shapes: N = 16384 and 4096, each with q = 132120577 (32-bit lanes) and the
62-bit prime; batch 8192, 64 and 1; t = 4; device-resident data, random words
below q.  Legs per shape and batch, all in one process:

  scaled    fhe_ct_multiply_scaled_batch
  floor     fhe_ct_multiply_batch on the main context: the reference's unscaled
            tensor, one of the three channels
  tensors   the tensor calls alone: fhe_ct_multiply_batch on the main context
            and on contexts with the auxiliary primes the call uses (`naux`:
            one while t n q stays below the first, else two)
  lift      the centred lift alone (fhe_ct_center_lift_batch over the batch: 8
            bytes read and 16 written per word, `lift_gbs`)
  round     the scale-and-round step alone (fhe_poly_scale_round_batch over
            2 * batch rows: 24 bytes read and 8 written per word, `round_gbs`)

and once per shape the inner product of 4096 pairs in one group:

  dot_scaled  fhe_ct_dot_scaled_batch
  dot_floor   fhe_ct_dot_batch on the main context

A scaled multiply runs two lifts, 1 + naux tensors and one rounding step, so
`scaled_over_floor` is at least 1 + naux.  Times are hipEvent spans on the context's
stream over `reps` back-to-back calls, after warm-up, the legs in alternating
windows; the figure is the median over `repeats` of the per-repeat medians.
One JSON line per row, then a markdown table; a row is printed in **bold** when
one of the two streaming kernels stays below three quarters of the mixed
read/write ceiling of 6.1 TB/s (tools/lab/c3bw.hip).
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
SHAPES = {"16384x27": (16384, P27), "16384x62": (16384, P62), "4096x27": (4096, P27), "4096x62": (4096, P62)}
CEILING_GBS = 6100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batches", default="8192,64,1")
    ap.add_argument("--pairs", type=int, default=4096, help="pairs of the inner product (0: skip it)")
    ap.add_argument("--t", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_scaled.py needs a GPU")
    L = fhe_gpu.lib()
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    rows = []
    for name in args.shapes.split(","):
        n, q = SHAPES[name]
        ring = fhe_gpu.PolynomialRing(n, q, mode="negacyclic", device=0)
        sm = fhe_gpu.ScaledMultiplier(ring, args.t)
        naux = 1 if sm.t * n * q < sm.aux[0] else 2
        aux = [fhe_gpu.PolynomialRing(n, p, mode="negacyclic", device=0) for p in sm.aux[:naux]]
        for r in [ring] + aux:
            r._bind_stream(DEV)
        h, sh = ring._h, sm._h
        stream = L.fhe_ctx_stream(h)
        gen = torch.Generator(device=dev).manual_seed(n)
        new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
        rand = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)

        def span(fn, reps):
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            return e0.elapsed_ms(e1) / reps

        def measure(legs):
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
            return {k: statistics.median(v) for k, v in meds.items()}

        for batch in [int(b) for b in args.batches.split(",")]:
            x, y = rand(batch, 2, n), rand(batch, 2, n)
            out, t1, t2 = new(batch, 3, n), new(batch, 3, n), new(batch, 3, n)
            l1, l2, ro = new(batch, 2, n), new(batch, 2, n), new(batch, 2, n)
            legs = {
                "scaled": lambda: check(L.fhe_ct_multiply_scaled_batch(sh, x.data_ptr(), y.data_ptr(), out.data_ptr(), batch, DEV)),
                "floor": lambda: check(L.fhe_ct_multiply_batch(h, x.data_ptr(), y.data_ptr(), out.data_ptr(), batch, 0, DEV)),
                "tensors": lambda: [check(L.fhe_ct_multiply_batch(r._h, x.data_ptr(), y.data_ptr(), o.data_ptr(), batch, 0, DEV))
                                    for r, o in zip([ring] + aux, (out, t1, t2))],
                "lift": lambda: check(L.fhe_ct_center_lift_batch(sh, x.data_ptr(), None, 0, l1.data_ptr(), l2.data_ptr(), batch, DEV)),
                # the 2 * batch rows of x and of the lift's outputs as the three residues
                "round": lambda: check(L.fhe_poly_scale_round_batch(sh, x.data_ptr(), l1.data_ptr(), l2.data_ptr(), ro.data_ptr(),
                                                                    2 * batch, DEV)),
            }
            ms = measure(legs)
            words = 2 * batch * n
            row = dict(n=n, q=q, t=sm.t, naux=naux, batch=batch, leg="multiply", scaled_ms=round(ms["scaled"], 5),
                       floor_ms=round(ms["floor"], 5), tensors_ms=round(ms["tensors"], 5), lift_ms=round(ms["lift"], 5),
                       round_ms=round(ms["round"], 5), lift_gbs=round(words * 24 / ms["lift"] / 1e6, 1),
                       round_gbs=round(words * 32 / ms["round"] / 1e6, 1),
                       scaled_over_floor=round(ms["scaled"] / ms["floor"], 3),
                       scaled_over_tensors=round(ms["scaled"] / ms["tensors"], 3), build_id=fhe_gpu.build_id())
            row["short_of_ceiling"] = bool(min(row["lift_gbs"], row["round_gbs"]) < 0.75 * CEILING_GBS)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, y, out, t1, t2, l1, l2, ro, legs
            torch.cuda.empty_cache()
        if args.pairs:
            count = args.pairs
            a, b, out = rand(1, count, 2, n), rand(1, count, 2, n), new(1, 3, n)
            ms = measure({
                "dot_scaled": lambda: check(L.fhe_ct_dot_scaled_batch(sh, a.data_ptr(), b.data_ptr(), count, 1, out.data_ptr(), DEV)),
                "dot_floor": lambda: check(L.fhe_ct_dot_batch(h, a.data_ptr(), b.data_ptr(), count, 1, 0, 0, out.data_ptr(), DEV)),
            })
            row = dict(n=n, q=q, t=sm.t, naux=1 if sm.t * count * n * q < sm.aux[0] else 2, batch=count, leg="dot", scaled_ms=round(ms["dot_scaled"], 5),
                       floor_ms=round(ms["dot_floor"], 5), scaled_over_floor=round(ms["dot_scaled"] / ms["dot_floor"], 3),
                       short_of_ceiling=False, build_id=fhe_gpu.build_id())
            rows.append(row)
            print(json.dumps(row), flush=True)
            del a, b, out
            torch.cuda.empty_cache()
        sm.close()
        del aux
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "short_of_ceiling": [(r["n"], r["q"], r["batch"]) for r in rows if r["short_of_ceiling"]]}), flush=True)
    print("\n| N | q | leg | batch | scaled ms | floor ms | x floor | tensors ms | lift ms (GB/s) | round ms (GB/s) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cells = [r["n"], "27-bit" if r["q"] == P27 else "62-bit", r["leg"], r["batch"], r["scaled_ms"], r["floor_ms"],
                 r["scaled_over_floor"], r.get("tensors_ms", ""),
                 "%s (%s)" % (r["lift_ms"], r["lift_gbs"]) if "lift_ms" in r else "",
                 "%s (%s)" % (r["round_ms"], r["round_gbs"]) if "round_ms" in r else ""]
        mark = "**" if r["short_of_ceiling"] else ""
        print("| " + " | ".join(mark + str(c) + mark if str(c) else "" for c in cells) + " |")


if __name__ == "__main__":
    main()
