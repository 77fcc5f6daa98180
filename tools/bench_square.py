#!/usr/bin/env python3
"""Times ciphertext squaring / the squared difference against the chains of
older entry points whose words they reproduce.

Shapes: N = 16384 and 4096, q = 132120577 (32-bit lanes) and
q = 4611686018326724609 (64-bit lanes), batch 8192 and 64, device-resident
data.  Pairs of legs (fused call, chain):

  sqdiff        fhe_ct_square_batch with one shared ref
  sqdiff_chain  fhe_poly_sub_batch (the ref replicated per ciphertext outside
                the timed window: the chain is not charged for it) into
                [batch][2][N], then fhe_ct_multiply_batch(d, d)
  square        fhe_ct_square_batch without a ref
  square_chain  fhe_ct_multiply_batch(ct, ct)
  relin         fhe_ct_square_relin_batch with one shared ref
  relin_chain   sqdiff_chain, then fhe_relinearize_batch (base_log 4, 7 levels)
  sqdiff_ntt / square_ntt (+ _chain): the first two pairs with is_ntt = 1

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up.  The legs of a pair are timed in alternating windows of
the same process; a repeat is `windows` (>= 20) windows per leg and yields one
median per leg.  Three repeats: the figure of a leg is the median of its three
medians, and `chain_spread_ms` is max - min of the chain's three -- the noise
against which "not slower than the chain" is read.  One JSON line per (n, q,
batch, pair), then a summary line.
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
PAIRS = ["sqdiff", "square", "relin", "sqdiff_ntt", "square_ntt"]
BASE_LOG, LEVEL = 4, 7


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--degrees", default="16384,4096")
    ap.add_argument("--moduli", default=f"{P27},{P62}")
    ap.add_argument("--batches", default="8192,64")
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_square.py needs a GPU")
    L = fhe_gpu.lib()
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE
    pairs = [p for p in PAIRS if p in args.pairs.split(",")]

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    rows = []
    for n in [int(x) for x in args.degrees.split(",")]:
        for q in [int(x) for x in args.moduli.split(",")]:
            ring = fhe_gpu.PolynomialRing(n, q, device=0)
            ring._bind_stream(DEV)
            h = ring._h
            stream = L.fhe_ctx_stream(h)
            gen = torch.Generator(device=dev).manual_seed(n)
            rlk = torch.randint(0, q, (LEVEL, 2, n), dtype=torch.int64, device=dev, generator=gen)
            ek = fhe_gpu.EvaluationKey(ring, rlk, BASE_LOG)
            pk = ek.rlk_ntt.data_ptr()

            def span(fn, reps):
                e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
                e0.record(stream)
                for _ in range(reps):
                    fn()
                e1.record(stream)
                check(L.fhe_ctx_synchronize(h))
                return e0.elapsed_ms(e1) / reps

            for batch in [int(b) for b in args.batches.split(",")]:
                cts = torch.randint(0, q, (batch, 2, n), dtype=torch.int64, device=dev, generator=gen)
                ref = torch.randint(0, q, (2, n), dtype=torch.int64, device=dev, generator=gen)
                rep = ref.unsqueeze(0).expand(batch, 2, n).contiguous()  # the chain's replicated ref
                diff = torch.empty((batch, 2, n), dtype=torch.int64, device=dev)
                o3 = {k: torch.empty((batch, 3, n), dtype=torch.int64, device=dev) for k in ("f", "c")}
                o2 = {k: torch.empty((batch, 2, n), dtype=torch.int64, device=dev) for k in ("f", "c")}
                pc, pr, prep, pd = cts.data_ptr(), ref.data_ptr(), rep.data_ptr(), diff.data_ptr()
                f3, c3, f2, c2 = o3["f"].data_ptr(), o3["c"].data_ptr(), o2["f"].data_ptr(), o2["c"].data_ptr()

                def sub_mul(is_ntt):
                    check(L.fhe_poly_sub_batch(h, pc, prep, pd, 2 * batch, DEV))
                    check(L.fhe_ct_multiply_batch(h, pd, pd, c3, batch, is_ntt, DEV))

                def relin_chain():
                    sub_mul(0)
                    check(L.fhe_relinearize_batch(h, BASE_LOG, LEVEL, c3, pk, c2, batch, DEV))

                legs = {
                    "sqdiff": (lambda: check(L.fhe_ct_square_batch(h, pc, pr, 1, f3, batch, 0, DEV)), lambda: sub_mul(0), o3),
                    "square": (lambda: check(L.fhe_ct_square_batch(h, pc, None, 0, f3, batch, 0, DEV)),
                               lambda: check(L.fhe_ct_multiply_batch(h, pc, pc, c3, batch, 0, DEV)), o3),
                    "relin": (lambda: check(L.fhe_ct_square_relin_batch(h, BASE_LOG, LEVEL, pc, pr, 1, pk, f2, batch, DEV)),
                              relin_chain, o2),
                    "sqdiff_ntt": (lambda: check(L.fhe_ct_square_batch(h, pc, pr, 1, f3, batch, 1, DEV)),
                                   lambda: sub_mul(1), o3),
                    "square_ntt": (lambda: check(L.fhe_ct_square_batch(h, pc, None, 0, f3, batch, 1, DEV)),
                                   lambda: check(L.fhe_ct_multiply_batch(h, pc, pc, c3, batch, 1, DEV)), o3),
                }
                for name in pairs:
                    fused, chain, outs = legs[name]
                    reps = {}
                    for key, fn in (("f", fused), ("c", chain)):
                        for _ in range(args.warmup):
                            fn()
                        check(L.fhe_ctx_synchronize(h))
                        reps[key] = max(1, min(500, int(args.target_ms / max(span(fn, 1), 1e-3))))
                    torch.cuda.synchronize()
                    assert torch.equal(outs["f"], outs["c"]), f"{name} differs from its chain at n {n} q {q} batch {batch}"
                    meds = {"f": [], "c": []}
                    for _ in range(args.repeats):
                        spans = {"f": [], "c": []}
                        for _ in range(args.windows):  # alternate the legs
                            spans["f"].append(span(fused, reps["f"]))
                            spans["c"].append(span(chain, reps["c"]))
                        for key in meds:
                            meds[key].append(statistics.median(spans[key]))
                    f, c = statistics.median(meds["f"]), statistics.median(meds["c"])
                    spread = max(meds["c"]) - min(meds["c"])
                    row = {"n": n, "q": q, "batch": batch, "pair": name, "fused_ms": round(f, 5), "chain_ms": round(c, 5),
                           "chain_over_fused": round(c / f, 3), "chain_spread_ms": round(spread, 5),
                           "fused_not_slower": bool(f <= c + spread), "reps": [reps["f"], reps["c"]],
                           "windows": args.windows, "repeats": args.repeats, "build_id": fhe_gpu.build_id()}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del cts, rep, diff, o3, o2
                torch.cuda.empty_cache()
    losers = [(r["n"], r["q"], r["batch"], r["pair"]) for r in rows if not r["fused_not_slower"]]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "slower_than_chain": losers}), flush=True)


if __name__ == "__main__":
    main()
