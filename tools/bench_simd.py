#!/usr/bin/env python3
"""Times the SIMD codec (fhe_simd_encode_batch / fhe_simd_decode_batch) and the
Galois chain (fhe_ct_galois_chain_batch) against what they replace.

Codec.  Shapes (n, t) = (8192, 65537), (16384, 65537) and (16384, the 62-bit
prime), batch 8192, 64 and 1, device-resident random words below t.  Legs, all
in one process:

  fused     the fused kernel (permutation in the transform's load / store)
  composed  the same call with FHE_SIMD_FUSED=0: k_simd_permute + the batched
            transform through a temporary (+ nothing else: lift = 0)
  ntt       the plain fhe_ntt_inv_batch (encode) / fhe_ntt_fwd_batch (decode) of
            the (n, t) ring: the same 16 bytes per slot, no permutation -- the
            floor of the fused kernel

Chain.  Shapes n = 8192 and 16384 with the 62-bit prime (base 2^21, 3 levels),
batch 64 and 1: sum_slots (log2 n steps, add_input = 1) and rotate_rows by an
odd step with three bits set (3 steps, add_input = 0), each as one
fhe_ct_galois_chain_batch call and as the same steps issued as separate
fhe_ct_galois_batch calls through two buffers.

Times are hipEvent spans on the context's stream over `reps` back-to-back
calls, after warm-up, the legs in alternating windows; a repeat is `windows`
windows per leg and yields one median per leg; the figure is the median of the
repeats' medians, the spread max - min of them.  One JSON line per row, then a
summary line with the build id and the rows where the fused codec was slower
than the composed path or the chain slower than the separate calls.
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

P27, P62, P62B = 132120577, 4611686018326724609, 4611686018425815041
# name -> (n, t, q)
CODEC = {"8192x65537": (8192, 65537, P27), "16384x65537": (16384, 65537, P27), "16384x62": (16384, P62, P62B)}
# name -> (n, q, base_log, level)
CHAIN = {"8192x62": (8192, P62, 21, 3), "16384x62": (16384, P62, 21, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--codec", default=",".join(CODEC))
    ap.add_argument("--chain", default=",".join(CHAIN))
    ap.add_argument("--batches", default="8192,64,1")
    ap.add_argument("--chain-batches", default="64,1")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-ms", type=float, default=8.0, help="device time aimed at per window")
    args = ap.parse_args()

    import torch

    import fhe_gpu

    if not torch.cuda.is_available():
        sys.exit("bench_simd.py needs a GPU")
    L = fhe_gpu.lib()
    dev = torch.device("cuda:0")
    DEV = fhe_gpu.FHE_DEVICE

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

    new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    rows = []
    for name in [s for s in args.codec.split(",") if s]:
        n, t, q = CODEC[name]
        ring = fhe_gpu.PolynomialRing(n, q, mode="negacyclic", device=0)
        tring = fhe_gpu.NTTProcessor(n, t, mode="negacyclic", device=0)
        ring._bind_stream(DEV)
        # the three legs share the main ring's stream
        check(L.fhe_ctx_set_stream(tring._h, L.fhe_ctx_stream(ring._h)))
        enc = fhe_gpu.SimdEncoder(ring, t)
        gen = torch.Generator(device=dev).manual_seed(n)
        for batch in [int(b) for b in args.batches.split(",")]:
            x = torch.randint(0, t, (batch, n), dtype=torch.int64, device=dev, generator=gen)
            fo, co, no = new(batch, n), new(batch, n), new(batch, n)
            for op in ("encode", "decode"):
                def call(out):
                    if op == "encode":
                        check(L.fhe_simd_encode_batch(enc._h, x.data_ptr(), 0, out.data_ptr(), batch, DEV))
                    else:
                        check(L.fhe_simd_decode_batch(enc._h, x.data_ptr(), out.data_ptr(), batch, DEV))

                def fused():
                    call(fo)

                def composed():
                    os.environ["FHE_SIMD_FUSED"] = "0"
                    try:
                        call(co)
                    finally:
                        del os.environ["FHE_SIMD_FUSED"]

                def ntt():
                    fn = L.fhe_ntt_inv_batch if op == "encode" else L.fhe_ntt_fwd_batch
                    check(fn(tring._h, x.data_ptr(), no.data_ptr(), batch, DEV))

                ms, spread, reps = bench(ring._h, {"fused": fused, "composed": composed, "ntt": ntt})
                torch.cuda.synchronize()
                assert torch.equal(fo, co), f"{op}: fused and composed words differ at {name} batch {batch}"
                row = dict(leg=op, n=n, t=t, batch=batch, fused_ms=round(ms["fused"], 5),
                           composed_ms=round(ms["composed"], 5), ntt_ms=round(ms["ntt"], 5),
                           fused_gbs=round(batch * n * 16 / ms["fused"] / 1e6, 1),
                           composed_over_fused=round(ms["composed"] / ms["fused"], 3),
                           fused_over_ntt=round(ms["fused"] / ms["ntt"], 3),
                           composed_spread_ms=round(spread["composed"], 5),
                           fused_not_slower=bool(ms["fused"] <= ms["composed"] + spread["composed"]),
                           reps=list(reps.values()), windows=args.windows, repeats=args.repeats,
                           build_id=fhe_gpu.build_id())
                rows.append(row)
                print(json.dumps(row), flush=True)
            del x, fo, co, no
            torch.cuda.empty_cache()
        enc.close()

    for name in [s for s in args.chain.split(",") if s]:
        n, q, bl, lv = CHAIN[name]
        ring = fhe_gpu.PolynomialRing(n, q, mode="negacyclic", device=0)
        ring._bind_stream(DEV)
        h = ring._h
        gen = torch.Generator(device=dev).manual_seed(n + 1)
        rand = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)
        sum_gs = fhe_gpu.slot_sum_elements(n)
        nk = len(sum_gs)
        keys = new(nk, lv, 2, n)
        check(L.fhe_relin_key_prepare(h, nk * lv, rand(nk, lv, 2, n).data_ptr(), keys.data_ptr(), DEV))
        rot_bits = [0, 2, 5]  # rotate_rows by 1 + 4 + 32 = 37
        cases = {"sum_slots": (sum_gs, list(range(nk)), 1), "rotate_rows": ([sum_gs[i] for i in rot_bits], rot_bits, 0)}
        for batch in [int(b) for b in args.chain_batches.split(",")]:
            ct, fo, co = rand(batch, 2, n), new(batch, 2, n), new(batch, 2, n)
            pong = [new(batch, 2, n), new(batch, 2, n)]
            for leg, (gs, idx, add) in cases.items():
                ns = len(gs)
                cg, ci = (fhe_gpu.C.c_uint32 * ns)(*gs), (fhe_gpu.C.c_uint32 * ns)(*idx)

                def chain():
                    check(L.fhe_ct_galois_chain_batch(h, bl, lv, ns, cg, ci, keys.data_ptr(), ct.data_ptr(), add,
                                                      fo.data_ptr(), batch, DEV))

                def calls():
                    src = ct
                    for i in range(ns):
                        dst = co if i + 1 == ns else pong[i & 1]
                        check(L.fhe_ct_galois_batch(h, bl, lv, gs[i], keys[idx[i]].data_ptr(), src.data_ptr(), add,
                                                    dst.data_ptr(), batch, DEV))
                        src = dst

                ms, spread, reps = bench(h, {"chain": chain, "calls": calls})
                torch.cuda.synchronize()
                assert torch.equal(fo, co), f"{leg}: the chain differs from the separate calls at {name} batch {batch}"
                row = dict(leg=leg, n=n, q=q, base_log=bl, level=lv, batch=batch, steps=ns,
                           chain_ms=round(ms["chain"], 5), calls_ms=round(ms["calls"], 5),
                           calls_over_chain=round(ms["calls"] / ms["chain"], 3), calls_spread_ms=round(spread["calls"], 5),
                           fused_not_slower=bool(ms["chain"] <= ms["calls"] + spread["calls"]),
                           reps=list(reps.values()), windows=args.windows, repeats=args.repeats,
                           build_id=fhe_gpu.build_id())
                rows.append(row)
                print(json.dumps(row), flush=True)
            del ct, fo, co, pong
            torch.cuda.empty_cache()
        del keys
        torch.cuda.empty_cache()
    losers = [(r["leg"], r["n"], r.get("t", r.get("q")), r["batch"]) for r in rows if not r["fused_not_slower"]]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build_id": fhe_gpu.build_id(), "rows": len(rows),
                      "slower": losers}), flush=True)


if __name__ == "__main__":
    main()
