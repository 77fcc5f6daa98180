#!/usr/bin/env python3
"""Times the hoisted rotations (fhe_ct_hoist_batch + fhe_ct_hoisted_galois_batch)
and the hoisted linear transform (fhe_ct_hoist_batch +
fhe_ct_hoisted_linear_batch) against what they replace.

Shapes n = 8192 and 16384 with the 27-bit prime (base 2^9, 3 levels) and the
62-bit prime (base 2^21, 3 levels), batch 1, 64 and 8192, R rotations / D
diagonals in {8, 64}, device-resident random words; and the hoist alone.
Legs, all in one process:

  default   hoist + the hoisted call as the library routes them (fused where
            the grid fills the device, else composed)
  fused     the same two calls with FHE_HOIST_FUSED=1 (fused kernels)
  composed  the same two calls with FHE_HOIST_FUSED=0 (digit kernel, batched
            transforms, streaming gathered MAC)
  parent    the route before these entry points.  Rotations: R separate
            fhe_ct_galois_batch calls.  Linear transform: per diagonal one
            fhe_ct_galois_batch into a temporary and one fhe_ct_dot_plain_batch
            (count 1, one group per ciphertext, accumulate after the first)
            against that diagonal's plaintext, replicated once per ciphertext
            outside the timed region.

The hoist is inside the timed region of the hoisted legs.  Before anything is
timed, the composed and the default words are asserted equal to the fused
ones, and the rotation whose element is 1 equal to fhe_ct_galois_batch (other
elements differ by definition: the digits differ).  A row holds two output
buffers (the parent leg reuses one); a row whose buffers would exceed
--max-gib is skipped and listed with its size.

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up, the legs in alternating windows; a repeat is `windows`
windows per leg and yields one median per leg; the figure is the median of the
repeats' medians, the spread max - min of them.  One JSON line per row, then a
summary line with the build id and the rows where the default path was slower
than the parent route.
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
SHAPES = {"8192x27": (8192, P27, 9, 3), "8192x62": (8192, P62, 21, 3), "16384x27": (16384, P27, 9, 3),
          "16384x62": (16384, P62, 21, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batches", default="1,64,8192")
    ap.add_argument("--counts", default="8,64")
    ap.add_argument("--ops", default="hoist,rotate,linear")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    ap.add_argument("--max-gib", type=float, default=150.0, help="skip rows whose buffers exceed this")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_hoist.py needs a GPU")
    L = fhe_gpu.lib()
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE
    U32 = fhe_gpu.C.c_uint32

    def check(rc):
        if rc:
            raise fhe_gpu.FHEError(rc, L.fhe_last_error().decode())

    def bench(h, legs):
        """{leg: median ms}, {leg: spread of the repeats' medians}, reps."""
        stream = L.fhe_ctx_stream(h)

        def span(fn, reps):
            e0, e1 = fhe_gpu.HipEvent(), fhe_gpu.HipEvent()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            check(L.fhe_ctx_synchronize(h))
            return e0.elapsed_ms(e1) / reps

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

    def forced(value, fn):
        """fn with FHE_HOIST_FUSED set to `value` (read per call by the library)."""
        def run():
            os.environ["FHE_HOIST_FUSED"] = value
            try:
                fn()
            finally:
                del os.environ["FHE_HOIST_FUSED"]
        return run

    new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    rows, skipped = [], []
    for name in [s for s in args.shapes.split(",") if s]:
        n, q, bl, lv = SHAPES[name]
        ring = fhe_gpu.PolynomialRing(n, q, mode="negacyclic", device=0)
        ring._bind_stream(DEV)
        h = ring._h
        gen = torch.Generator(device=dev).manual_seed(n + lv)
        rand = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)
        for count in [int(c) for c in args.counts.split(",")]:
            # row rotations by 0 .. count - 1: the first element is 1 (checked against fhe_ct_galois_batch)
            gs = [fhe_gpu.rotation_element(n, st) for st in range(count)]
            cg, ci = (U32 * count)(*gs), (U32 * count)(*range(count))
            keys = new(count, lv, 2, n)
            check(L.fhe_relin_key_prepare(h, count * lv, rand(count, lv, 2, n).data_ptr(), keys.data_ptr(), DEV))
            pts = rand(count, n)
            pts_ntt = new(count, n)
            check(L.fhe_ntt_fwd_batch(h, pts.data_ptr(), pts_ntt.data_ptr(), count, DEV))
            for batch in [int(b) for b in args.batches.split(",")]:
                for op in [o for o in args.ops.split(",") if o]:
                    lin, only = op == "linear", op == "hoist"
                    if only and count != int(args.counts.split(",")[0]):
                        continue  # the hoist does not depend on the count
                    # ct, hoisted, two outputs (the parent leg reuses the second), linear: tmp and the replicated rows
                    per = (2 + (1 + lv) + ((1 + lv) if only else 4 if lin else 4 * count) + ((2 + count) if lin else 0))
                    if batch * n * per * 8 > args.max_gib * 2 ** 30:
                        skipped.append((op, name, batch, count, round(batch * n * per * 8 / 2 ** 30, 1)))
                        continue
                    ct, hoisted = rand(batch, 2, n), new(batch, 1 + lv, n)
                    oshape = (batch, 1 + lv, n) if only else (batch, 2, n) if lin else (batch, count, 2, n)
                    fo, co = (hoisted if only else new(*oshape)), new(*oshape)
                    if lin:
                        tmp = new(batch, 2, n)
                        rep = pts[:, None, :].expand(count, batch, n).contiguous()  # [D][batch][n], untimed
                    po = co if lin else co.view(count, batch, 2, n) if not only else None

                    def hoisted_call(out):
                        check(L.fhe_ct_hoist_batch(h, bl, lv, ct.data_ptr(), (out if only else hoisted).data_ptr(), batch, DEV))
                        if lin:
                            check(L.fhe_ct_hoisted_linear_batch(h, lv, count, cg, ci, keys.data_ptr(), pts_ntt.data_ptr(),
                                                                hoisted.data_ptr(), 0, out.data_ptr(), batch, DEV))
                        elif not only:
                            check(L.fhe_ct_hoisted_galois_batch(h, lv, count, cg, ci, keys.data_ptr(), hoisted.data_ptr(),
                                                                out.data_ptr(), batch, DEV))

                    def parent():
                        for r in range(count):
                            dst = tmp if lin else po[r]
                            check(L.fhe_ct_galois_batch(h, bl, lv, gs[r], keys[r].data_ptr(), ct.data_ptr(), 0,
                                                        dst.data_ptr(), batch, DEV))
                            if lin:
                                check(L.fhe_ct_dot_plain_batch(h, tmp.data_ptr(), rep[r].data_ptr(), 1, batch, 0,
                                                               1 if r else 0, po.data_ptr(), DEV))

                    # equal words, leg by leg, before anything is timed: the forced fused path is the reference row
                    where = f"{op} at {name} batch {batch} x {count}"
                    forced("1", lambda: hoisted_call(fo))()
                    for leg, run in (("composed", forced("0", lambda: hoisted_call(co))), ("default", lambda: hoisted_call(co))):
                        co.zero_()
                        run()
                        torch.cuda.synchronize()
                        assert torch.equal(fo, co), f"{leg} and fused words differ: {where}"
                    if not lin and not only:
                        parent()
                        torch.cuda.synchronize()
                        assert torch.equal(fo[:, 0], po[0]), f"g = 1 differs from fhe_ct_galois_batch: {where}"
                    legs = {"default": lambda: hoisted_call(co), "fused": forced("1", lambda: hoisted_call(co)),
                            "composed": forced("0", lambda: hoisted_call(co))}
                    if not only:
                        legs["parent"] = parent
                    ms, spread, reps = bench(h, legs)
                    base = "composed" if only else "parent"
                    row = dict(leg=op, n=n, q=q, base_log=bl, level=lv, batch=batch, count=0 if only else count,
                               default_ms=round(ms["default"], 5), fused_ms=round(ms["fused"], 5),
                               composed_ms=round(ms["composed"], 5), parent_ms=round(ms["parent"], 5) if not only else None,
                               parent_over_default=round(ms["parent"] / ms["default"], 3) if not only else None,
                               best_forced_over_default=round(min(ms["fused"], ms["composed"]) / ms["default"], 3),
                               spread_ms={k: round(v, 5) for k, v in spread.items()},
                               default_not_slower=bool(ms["default"] <= ms[base] + spread[base]),
                               reps=list(reps.values()), windows=args.windows, repeats=args.repeats,
                               build_id=fhe_gpu.build_id())
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del ct, hoisted, fo, co, po
                    if lin:
                        del tmp, rep
                    torch.cuda.empty_cache()
            del keys, pts, pts_ntt
            torch.cuda.empty_cache()
    losers = [(r["leg"], r["n"], r["q"], r["batch"], r["count"]) for r in rows if not r["default_not_slower"]]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "slower": losers, "skipped_for_memory": skipped}), flush=True)


if __name__ == "__main__":
    main()
