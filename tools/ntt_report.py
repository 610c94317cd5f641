#!/usr/bin/env python3
"""What msmz_scalars_ntt costs.  BLS12-377 and Pallas, generated resident sets, ONE process.

    python tools/ntt_report.py [--out FILE] [--reps R] [--logn 16 20 24] [--batch COUNT LOGN] [--curves LABEL ...]

For every curve and shape (one transform of 2^16, 2^20 and 2^24 entries, and 64 transforms of 2^12 in one call) it
times, as the median wall milliseconds of `reps` whole calls after one warm-up (the warm-up also builds and caches the
twiddle tables; a result handle is freed outside the timed region):
    forward / inverse / coset / coset_inverse      the four directions of msmz_scalars_ntt
Beside each leg:
    copy        a plain device-to-device copy that moves the same number of bytes (every pass reads and writes every
                entry once: 64 bytes per element and pass), through torch (imported before the library is loaded: a
                process drives the GPU through one copy of the HIP runtime);
    predicted   the time the project's own measured product rate predicts: profiles/scalar_scan_report.jsonl has the
                general recurrence at 8 Montgomery products per element for 2^24 entries of the same curve; the
                transform's products per element follow from its plan (one per radix-4 step, two
                per pass boundary, two for a forward coset, one or two for the inverse scaling).
Reported: the plan's stages, products and bytes per element, GB/s, the fraction of the copy's rate, and measured over
predicted.  One JSON line per leg, to stdout and appended to --out (default profiles/ntt_report.jsonl).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INVERSE, COSET = 1, 2


def product_rate(label):
    """milliseconds per (Montgomery product x 2^24 elements), from the general recurrence of scalar_scan_report.jsonl"""
    path = os.path.join(ROOT, "profiles", "scalar_scan_report.jsonl")
    for line in open(path):
        row = json.loads(line)
        if (row["curve"], row["log2n"], row["leg"]) == (label, 24, "general"):
            return row["ms"] / row["products_per_element"]
    raise SystemExit(f"{path} has no general recurrence at 2^24 for {label}")


def products_per_element(stages, flags):
    """the Montgomery products one entry meets on its way through the plan"""
    p = sum(s // 2 for s in stages) + 2 * (len(stages) - 1)
    if flags & INVERSE:
        return p + (2 if flags & COSET else 1)
    return p + (2 if flags & COSET else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_report.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--batch", type=int, nargs=2, default=[64, 12], metavar=("COUNT", "LOGN"))
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    args = ap.parse_args()
    import torch   # before libmsmz.so
    import msm_zprize_amd as m
    from msm_zprize_amd._native import MsmzNtt, check, lib
    m.startThreads()
    rows = []

    def timed(call, reps):
        call()
        return statistics.median(call() for _ in range(reps))

    def copy_ms(nbytes):
        a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def call():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.copy_(a)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        return timed(call, args.reps)

    for params in m.curves.ALL_CURVES:
        if params["label"] not in args.curves:
            continue
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        q = params["order"]
        par, ctx = curve.Parallel, curve._ctx
        rate = product_rate(params["label"])
        shift = (q * 5 // 7).to_bytes(32, "little")
        for count, logn in [(1, k) for k in args.logn] + [tuple(args.batch)]:
            n = 1 << logn
            x = par.randomScalars(count * n, 41)
            n_passes, stages = C.c_uint32(0), (C.c_uint32 * 8)()
            check(lib().msmz_test_ntt_plan(params["curve_id"], logn, C.byref(n_passes), stages), "msmz_test_ntt_plan")
            stages = list(stages)[:n_passes.value]

            def transform(flags):
                t = MsmzNtt(x.handle, 0, logn, flags, 0, count, None, shift if flags & COSET else None)
                h = C.c_uint64(0)
                t0 = time.perf_counter()
                check(lib().msmz_scalars_ntt(ctx, C.byref(t), 0, C.byref(h)), "msmz_scalars_ntt")
                ms = (time.perf_counter() - t0) * 1e3
                check(lib().msmz_free(ctx, h.value), "msmz_free")
                return ms

            nbytes = 64 * len(stages)
            cms = copy_ms(nbytes * count * n // 2)   # reads and writes nbytes * n / 2 each: the same traffic
            for name, flags in (("forward", 0), ("inverse", INVERSE), ("coset", COSET), ("coset_inverse", INVERSE | COSET)):
                ms = timed(lambda: transform(flags), args.reps)
                products = products_per_element(stages, flags)
                predicted = products * rate * count * n / (1 << 24)
                row = {"curve": params["label"], "log2n": logn, "count": count, "leg": name, "ms": round(ms, 4),
                       "stages": stages, "bytes_per_element": nbytes, "products_per_element": products,
                       "gb_per_s": round(nbytes * count * n / (ms * 1e-3) / 1e9, 2), "reps": args.reps,
                       "copy_ms": round(cms, 4), "fraction_of_copy_rate": round(cms / ms, 4),
                       "predicted_ms": round(predicted, 4), "measured_over_predicted": round(ms / predicted, 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            x.free()
        curve.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
