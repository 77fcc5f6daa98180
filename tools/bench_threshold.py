#!/usr/bin/env python3
"""Times batched threshold decryption against the chains of older entry points
whose words it reproduces.

Shapes: N = 16384 and 4096, q = 132120577 (32-bit lanes) and
q = 4611686018326724609 (64-bit lanes), batch 4096 and 64, device-resident
data, one local share.  Pairs of legs (fused call, chain):

  partial         fhe_partial_decrypt_batch with one prepared share
  partial_chain   a gather of c1 from [batch][2][N] into [batch][N] (a strided
                  device copy), then fhe_polymul_batch(c1, share) with the share
                  replicated per ciphertext outside the timed window (the chain
                  is not charged for it); `chain_nogather_ms` is the same chain
                  with c1 gathered outside the window too
  combine3/7      fhe_combine_partials_batch over 3 / 7 partials, values +
                  max_noise out
  combine_chain   per partial fhe_poly_mul_scalar_batch (+ fhe_poly_add_batch
                  from the second on), then fhe_poly_sub_batch(c0, .) with c0
                  gathered outside the window.  The chain STOPS AT THE PHASE: it
                  has no device decode to call, so it does less work than the
                  fused leg, which also decodes every word and reduces the
                  noise -- the comparison favours the chain.

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up.  The legs of a pair are timed in alternating windows of
the same process; a repeat is `windows` (>= 20) windows per leg and yields one
median per leg.  Three repeats: the figure of a leg is the median of its three
medians, and `chain_spread_ms` is max - min of the chain's three -- the noise
against which "not slower than the chain" is read.  One JSON line per (n, q,
batch, pair), then a summary line.
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

P27, P62 = 132120577, 4611686018326724609
PAIRS = ["partial", "combine3", "combine7"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--degrees", default="16384,4096")
    ap.add_argument("--moduli", default=f"{P27},{P62}")
    ap.add_argument("--batches", default="4096,64")
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_threshold.py needs a GPU")
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
            share = fhe_gpu.KeyShare(ring, 1, torch.randint(0, q, (n,), dtype=torch.int64, device=dev, generator=gen))
            sp = share.prep.data_ptr()

            def span(fn, reps):
                e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
                e0.record(stream)
                for _ in range(reps):
                    fn()
                e1.record(stream)
                check(L.fhe_ctx_synchronize(h))
                return e0.elapsed_ms(e1) / reps

            for batch in [int(b) for b in args.batches.split(",")]:
                new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
                cts = torch.randint(0, q, (batch, 2, n), dtype=torch.int64, device=dev, generator=gen)
                pc = cts.data_ptr()
                for name in pairs:
                    if name == "partial":
                        rep = share.poly.unsqueeze(0).expand(batch, n).contiguous()  # the chain's replicated share
                        c1, c1pre = new(batch, n), cts[:, 1, :].contiguous()
                        outs = {"f": new(batch, n), "c": new(batch, n)}
                        pf, pch, p1, p1pre, prep = (outs["f"].data_ptr(), outs["c"].data_ptr(), c1.data_ptr(),
                                                    c1pre.data_ptr(), rep.data_ptr())

                        def chain():
                            c1.copy_(cts[:, 1, :])  # on the context's stream (torch's current one)
                            check(L.fhe_polymul_batch(h, p1, prep, pch, batch, DEV))

                        legs = {"f": lambda: check(L.fhe_partial_decrypt_batch(h, sp, 1, pc, pf, batch, DEV)), "c": chain,
                                "g": lambda: check(L.fhe_polymul_batch(h, p1pre, prep, pch, batch, DEV))}
                        keep = (rep, c1, c1pre)
                    else:
                        count = int(name[len("combine"):])
                        par = torch.randint(0, q, (count, batch, n), dtype=torch.int64, device=dev, generator=gen)
                        lams = [int(x) for x in torch.randint(1, q, (count,), generator=torch.Generator().manual_seed(count))]
                        lam = (C.c_uint64 * count)(*lams)
                        c0 = cts[:, 0, :].contiguous()
                        acc, term = new(batch, n), new(batch, n)
                        vals, mx, ph = new(batch, n), new(batch), new(batch, n)
                        outs = {"f": ph, "c": acc}
                        pp, p0, pa, pt = par.data_ptr(), c0.data_ptr(), acc.data_ptr(), term.data_ptr()
                        pv, pm, pph = vals.data_ptr(), mx.data_ptr(), ph.data_ptr()

                        def chain():
                            for i in range(count):
                                check(L.fhe_poly_mul_scalar_batch(h, pp + i * batch * n * 8, lams[i], pt if i else pa, batch, DEV))
                                if i:
                                    check(L.fhe_poly_add_batch(h, pa, pt, pa, batch, DEV))
                            check(L.fhe_poly_sub_batch(h, p0, pa, pa, batch, DEV))

                        # once with the phase, for the equality check below; the timed leg writes values + max_noise
                        check(L.fhe_combine_partials_batch(h, 0, pc, pp, lam, count, None, pph, None, batch, DEV))
                        legs = {"f": lambda: check(L.fhe_combine_partials_batch(h, 0, pc, pp, lam, count, pv, None, pm, batch, DEV)),
                                "c": chain}
                        keep = (par, c0, term, vals, mx)
                    reps = {}
                    for key, fn in legs.items():
                        for _ in range(args.warmup):
                            fn()
                        check(L.fhe_ctx_synchronize(h))
                        reps[key] = max(1, min(500, int(args.target_ms / max(span(fn, 1), 1e-3))))
                    torch.cuda.synchronize()
                    assert torch.equal(outs["f"], outs["c"]), f"{name} differs from its chain at n {n} q {q} batch {batch}"
                    meds = {k: [] for k in legs}
                    for _ in range(args.repeats):
                        spans = {k: [] for k in legs}
                        for _ in range(args.windows):  # alternate the legs
                            for key, fn in legs.items():
                                spans[key].append(span(fn, reps[key]))
                        for key in meds:
                            meds[key].append(statistics.median(spans[key]))
                    f, c = statistics.median(meds["f"]), statistics.median(meds["c"])
                    spread = max(meds["c"]) - min(meds["c"])
                    row = {"n": n, "q": q, "batch": batch, "pair": name, "fused_ms": round(f, 5), "chain_ms": round(c, 5),
                           "chain_over_fused": round(c / f, 3), "chain_spread_ms": round(spread, 5),
                           "fused_not_slower": bool(f <= c + spread)}
                    if "g" in legs:
                        g = statistics.median(meds["g"])
                        gs = max(meds["g"]) - min(meds["g"])
                        row.update({"chain_nogather_ms": round(g, 5), "chain_nogather_spread_ms": round(gs, 5),
                                    "fused_not_slower_nogather": bool(f <= g + gs)})
                    else:
                        row["note"] = "chain stops at the phase (no decode, no noise): the comparison favours the chain"
                    row.update({"reps": [reps[k] for k in legs], "windows": args.windows, "repeats": args.repeats,
                                "build_id": fhe_gpu.build_id()})
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del outs, keep, legs
                    torch.cuda.empty_cache()
                del cts
                torch.cuda.empty_cache()
    losers = [(r["n"], r["q"], r["batch"], r["pair"]) for r in rows
              if not (r["fused_not_slower"] and r.get("fused_not_slower_nogather", True))]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "slower_than_chain": losers}), flush=True)


if __name__ == "__main__":
    main()
