#!/usr/bin/env python3
"""Times fhe_slot_extract_batch against the chain of older entry points whose
words it reproduces, and a whole encrypted comparison around it.

Shapes: (N, q) = (2048, Q_50_1) and (4096, Q_60_1); batch 1, 64 and 4096; 1 and
16 slots; with a reference ciphertext per ciphertext and without one;
device-resident data.  Legs:

  fused   fhe_slot_extract_batch (no body offsets: the chain has no entry point
          that adds one)
  chain   fhe_poly_sub_batch(ct, ref) (against zeros without a reference: the
          chain needs the reduced words), then per slot fhe_glwe_rotate_batch by
          -slot and fhe_sample_extract_batch.  The (mask, body) swap of the RLWE
          pair is made outside the timed window: the chain is not charged for it.

Traffic model, in words per ciphertext of degree N with S slots: the fused call
reads ct (2 N) and the reference (2 N) and writes S rows (S N); the chain moves
6 N for the subtraction and 6 N per slot (rotate 2 N in, 2 N out; extract N in,
N out, the body aside).  `fused_gbs` / `chain_gbs` are those bytes over the
measured time.

`ge_ms` is one Comparisons.greater_equal (extraction, key switch, sign
bootstrap, sum) over the same ciphertexts and slots with random keys of the
preset's dimensions, for the shapes of at most --pipeline-max bootstraps;
`extract_share` = fused_ms / ge_ms.

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up, the two legs in alternating windows of one process; a
repeat is `windows` windows per leg and yields one median per leg; the figure is
the median of the repeats' medians and `chain_spread_ms` is max - min of the
chain's.  One JSON line per row, then a summary line.
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

Q_50_1, Q_60_1 = 1125899906826241, 1152921504606584833
# (n, q, t, lwe dimension, base_log, level): tfhe-128-balanced and tfhe-256-secure
SHAPES = {2048: (2048, Q_50_1, 8, 830, 15, 2), 4096: (4096, Q_60_1, 16, 1024, 10, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--degrees", default="2048,4096")
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--slots", default="1,16")
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    ap.add_argument("--pipeline-max", type=int, default=1024, help="most bootstraps of a timed greater_equal (0: none)")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_compare.py needs a GPU")
    L = fhe_gpu.lib()
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    rows = []
    for n, q, t, dim, bl, lv in [SHAPES[int(x)] for x in args.degrees.split(",")]:
        ring = fhe_gpu.PolynomialRing(n, q, device=0)
        ring._bind_stream(DEV)
        h = ring._h
        stream = L.fhe_ctx_stream(h)
        gen = torch.Generator(device=dev).manual_seed(n)
        new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
        rand = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)
        cmp_ = None
        if args.pipeline_max:
            be = fhe_gpu.BootstrapEngine(ring, bl, lv, 1)
            cmp_ = fhe_gpu.Comparisons(ring, t, be.prepare_ggsw(rand(dim, 2 * lv, 2, n)), rand(n * lv, dim), rand(n * lv),
                                       bl, lv, bl, lv)

        def span(fn, reps):
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            return e0.elapsed_ms(e1) / reps

        for batch in [int(b) for b in args.batches.split(",")]:
            cts, refs = rand(batch, 2, n), rand(batch, 2, n)
            zeros = torch.zeros_like(cts)
            cts_sw, refs_sw = cts.flip(-2).contiguous(), refs.flip(-2).contiguous()
            for S in [int(s) for s in args.slots.split(",")]:
                slots = [(s * (n // S) + 5) % n for s in range(S)]
                sl = (C.c_uint32 * S)(*slots)
                rots = [torch.full((batch,), -s, dtype=torch.int32, device=dev) for s in slots]
                fa, fb = new(batch, S, n), new(batch, S)
                ca, cb = new(S, batch, n), new(S, batch)
                d, rot = new(batch, 2, n), new(batch, 2, n)
                for with_ref in (True, False):
                    pr = refs.data_ptr() if with_ref else None
                    psub = (refs_sw if with_ref else zeros).data_ptr()

                    def fused():
                        check(L.fhe_slot_extract_batch(h, cts.data_ptr(), pr, batch if with_ref else 0, 0, sl, None, S,
                                                       fa.data_ptr(), fb.data_ptr(), batch, DEV))

                    def chain():
                        check(L.fhe_poly_sub_batch(h, cts_sw.data_ptr(), psub, d.data_ptr(), 2 * batch, DEV))
                        for s in range(S):
                            check(L.fhe_glwe_rotate_batch(h, 1, rots[s].data_ptr(), d.data_ptr(), rot.data_ptr(), batch, DEV))
                            check(L.fhe_sample_extract_batch(h, 1, rot.data_ptr(), ca[s].data_ptr(), cb[s].data_ptr(), batch,
                                                             DEV))

                    legs = {"f": fused, "c": chain}
                    reps = {}
                    for key, fn in legs.items():
                        for _ in range(args.warmup):
                            fn()
                        check(L.fhe_ctx_synchronize(h))
                        reps[key] = max(1, min(500, int(args.target_ms / max(span(fn, 1), 1e-3))))
                    torch.cuda.synchronize()
                    assert torch.equal(fa, ca.transpose(0, 1)) and torch.equal(fb, cb.transpose(0, 1)), \
                        f"slot extraction differs from its chain at n {n} batch {batch} slots {S} ref {with_ref}"
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
                    fused_bytes = 8 * n * batch * ((4 if with_ref else 2) + S)
                    chain_bytes = 8 * n * batch * (6 + 6 * S)
                    row = {"n": n, "q": q, "batch": batch, "slots": S, "ref": with_ref, "fused_ms": round(f, 5),
                           "chain_ms": round(c, 5), "chain_over_fused": round(c / f, 3), "chain_spread_ms": round(spread, 5),
                           "fused_not_slower": bool(f <= c + spread), "fused_gbs": round(fused_bytes / f / 1e6, 1),
                           "chain_gbs": round(chain_bytes / c / 1e6, 1)}
                    if cmp_ is not None and with_ref and batch * S <= args.pipeline_max:
                        ge = lambda: cmp_.greater_equal(cts, refs, slots)
                        ge()
                        g = statistics.median([span(ge, 1) for _ in range(3)])
                        row.update({"ge_ms": round(g, 4), "extract_share": round(f / g, 5)})
                    row.update({"reps": [reps[k] for k in legs], "windows": args.windows, "repeats": args.repeats,
                                "build_id": fhe_gpu.build_id()})
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del fa, fb, ca, cb, d, rot
                torch.cuda.empty_cache()
            del cts, refs, zeros, cts_sw, refs_sw
            torch.cuda.empty_cache()
    losers = [(r["n"], r["batch"], r["slots"], r["ref"]) for r in rows if not r["fused_not_slower"]]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "slower_than_chain": losers}), flush=True)


if __name__ == "__main__":
    main()
