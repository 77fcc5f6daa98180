#!/usr/bin/env python3
"""Times fhe_lwe_pack_batch against the chain of older entry points whose words
it reproduces.

Shapes: tfhe-128-balanced (N 2048, Q_50_1, LWE dimension 830, key-switch base
2^15, 2 levels) and tfhe-256-secure (N 4096, Q_60_1, 1024, 2^10, 3); 1 and 16
slots; batch 1, 64 and 4096 output ciphertexts; device-resident data, random key
and LWE words below q.  Legs:

  fused   fhe_lwe_pack_batch
  chain   fhe_key_switch_batch of the batch * slots LWE ciphertexts to 2N words
          (the pack key viewed as [in_dim * level][2N], zero body key), the bodies
          added mod q on coefficient 0 of the first half (one strided device
          add), fhe_glwe_rotate_batch by +slot, fhe_ct_sum_batch over the slots.

Both legs make batch * slots * in_dim * level * 2N wrapped 64-bit
multiply-adds and read the key once per tile of ciphertexts; the chain also
writes and re-reads [batch * slots][2N] rows twice.  `gmacs` is that count over
the fused time.

Times are hipEvent spans on the context's stream over `reps` back-to-back calls,
after warm-up, the two legs in alternating windows of one process; a repeat is
`windows` windows per leg and yields one median per leg; the figure is the median
of the repeats' medians and `chain_spread_ms` is max - min of the chain's.  Rows
whose single call passes --long-ms run 3 windows of one repeat.  One JSON line
per row, then a summary line that lists the rows where the fused call was slower.
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
# (n, q, lwe dimension, base_log, level): tfhe-128-balanced and tfhe-256-secure
SHAPES = {2048: (2048, Q_50_1, 830, 15, 2), 4096: (4096, Q_60_1, 1024, 10, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--degrees", default="2048,4096")
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--slots", default="1,16")
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    ap.add_argument("--long-ms", type=float, default=100.0, help="a call longer than this runs 3 windows of one repeat")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_pack.py needs a GPU")
    L = fhe_gpu.lib()
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    rows = []
    for n, q, dim, bl, lv in [SHAPES[int(x)] for x in args.degrees.split(",")]:
        ring = fhe_gpu.PolynomialRing(n, q, device=0)
        ring._bind_stream(DEV)
        h = ring._h
        stream = L.fhe_ctx_stream(h)
        gen = torch.Generator(device=dev).manual_seed(n)
        new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
        rand = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)
        entries = dim * lv
        key = rand(entries, 2, n)
        zero_kb = torch.zeros(entries, dtype=torch.int64, device=dev)

        def span(fn, reps):
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            return e0.elapsed_ms(e1) / reps

        for batch in [int(b) for b in args.batches.split(",")]:
            for S in [int(s) for s in args.slots.split(",")]:
                slots = [(s * (n // S) + 5) % n for s in range(S)]
                sl = (C.c_uint32 * S)(*slots)
                rots = torch.tensor(slots * batch, dtype=torch.int32, device=dev)
                la, lb = rand(batch, S, dim), rand(batch, S)
                zero_b = torch.zeros(batch * S, dtype=torch.int64, device=dev)
                fo, co = new(batch, 2, n), new(batch, 2, n)
                ksa, ksb, rot = new(batch * S, 2 * n), new(batch * S), new(batch * S, 2, n)
                body = ksa[:, 0]
                flat_b = lb.reshape(-1)

                def fused():
                    check(L.fhe_lwe_pack_batch(h, bl, lv, dim, key.data_ptr(), la.data_ptr(), lb.data_ptr(), sl, S, 0,
                                               fo.data_ptr(), batch, DEV))

                def chain():
                    check(L.fhe_key_switch_batch(q, bl, lv, dim, 2 * n, key.data_ptr(), zero_kb.data_ptr(), la.data_ptr(),
                                                 zero_b.data_ptr(), ksa.data_ptr(), ksb.data_ptr(), batch * S, DEV, 0,
                                                 stream))
                    body.add_(flat_b).remainder_(q)  # both below q < 2^62
                    # the monomial rotates both halves alike: their order does not matter here
                    check(L.fhe_glwe_rotate_batch(h, 1, rots.data_ptr(), ksa.data_ptr(), rot.data_ptr(), batch * S, DEV))
                    check(L.fhe_ct_sum_batch(h, rot.data_ptr(), 2, S, batch, 0, co.data_ptr(), DEV))

                legs = {"f": fused, "c": chain}
                reps, single = {}, {}
                for k, fn in legs.items():
                    for _ in range(args.warmup):
                        fn()
                    check(L.fhe_ctx_synchronize(h))
                    single[k] = span(fn, 1)
                    reps[k] = max(1, min(500, int(args.target_ms / max(single[k], 1e-3))))
                torch.cuda.synchronize()
                assert torch.equal(fo, co), f"packing differs from its chain at n {n} batch {batch} slots {S}"
                long_row = max(single.values()) > args.long_ms
                windows, repeats = (3, 1) if long_row else (args.windows, args.repeats)
                meds = {k: [] for k in legs}
                for _ in range(repeats):
                    spans = {k: [] for k in legs}
                    for _ in range(windows):  # alternate the legs
                        for k, fn in legs.items():
                            spans[k].append(span(fn, reps[k]))
                    for k in meds:
                        meds[k].append(statistics.median(spans[k]))
                f, c = statistics.median(meds["f"]), statistics.median(meds["c"])
                spread = max(meds["c"]) - min(meds["c"])
                macs = batch * S * entries * 2 * n
                row = {"n": n, "q": q, "lwe_dim": dim, "base_log": bl, "level": lv, "batch": batch, "slots": S,
                       "fused_ms": round(f, 5), "chain_ms": round(c, 5), "chain_over_fused": round(c / f, 3),
                       "chain_spread_ms": round(spread, 5), "fused_not_slower": bool(f <= c + spread),
                       "gmacs": round(macs / f / 1e6, 1), "reps": [reps[k] for k in legs], "windows": windows,
                       "repeats": repeats, "build_id": fhe_gpu.build_id()}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del la, lb, zero_b, fo, co, ksa, ksb, rot, body, flat_b, rots
                torch.cuda.empty_cache()
        del key, zero_kb
        torch.cuda.empty_cache()
    losers = [(r["n"], r["batch"], r["slots"]) for r in rows if not r["fused_not_slower"]]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "slower_than_chain": losers}), flush=True)


if __name__ == "__main__":
    main()
