#!/usr/bin/env python3
"""What msmz_scalars_recurrence / _inverse cost.  BLS12-377 and Pallas, generated resident sets, ONE process.

    python tools/scalar_scan_report.py [--out FILE] [--reps R] [--logn 16 20 24] [--host-max-logn L] [--curves LABEL ...]

For every curve and size it times, as the median wall milliseconds of `reps` calls after one warm-up (a result handle is
freed outside the timed region):
    sums / geometric / horner / products / general     the five modes of msmz_scalars_recurrence (no multiplier + addend,
                                                       broadcast multiplier without and with an addend, resident
                                                       multiplier without and with an addend)
    inverse                                            msmz_scalars_inverse
Beside each leg:
    host route  what a caller has without these calls: msmz_download_scalars, the same arithmetic with Python integers,
                msmz_upload_scalars -- ONE run (it takes seconds to minutes), sizes up to 2^host-max-logn;
    copy        a plain device-to-device copy that moves the same number of bytes, the memory-bound yardstick, through
                torch (imported before the library is loaded: a process drives the GPU through one copy of the HIP
                runtime).
Reported: bytes moved per element (32 per record read or written, both launches that read the operands counted),
Montgomery products per element, GB/s, and the fraction of the copy's rate.  One JSON line per
leg, to stdout and appended to --out (default profiles/scalar_scan_report.jsonl).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_scan_report.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--host-max-logn", type=int, default=24)
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    args = ap.parse_args()
    import torch   # before libmsmz.so
    import msm_zprize_amd as m
    from msm_zprize_amd._native import MsmzScalarRec, check, lib
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
        z = q * 5 // 7
        zb = z.to_bytes(32, "little")
        for logn in args.logn:
            n = 1 << logn
            x, y = (par.randomScalars(n, seed) for seed in (31, 32))

            def recurrence(ah, ab, bh):
                rec = MsmzScalarRec(ah, 0, ab, bh, 0, None, 0)
                h = C.c_uint64(0)
                last = C.create_string_buffer(32)
                t0 = time.perf_counter()
                check(lib().msmz_scalars_recurrence(ctx, C.byref(rec), n, 0, C.byref(h), last), "msmz_scalars_recurrence")
                ms = (time.perf_counter() - t0) * 1e3
                check(lib().msmz_free(ctx, h.value), "msmz_free")
                return ms

            def inverse():
                h = C.c_uint64(0)
                t0 = time.perf_counter()
                check(lib().msmz_scalars_inverse(ctx, x.handle, 0, n, 0, C.byref(h), None), "msmz_scalars_inverse")
                ms = (time.perf_counter() - t0) * 1e3
                check(lib().msmz_free(ctx, h.value), "msmz_free")
                return ms

            def host(a_arr, a_const, b_arr, invert):
                """download, Python integers, upload: one run"""
                t0 = time.perf_counter()
                av = curve.Scalar.toBigints(a_arr) if a_arr is not None else None
                bv = curve.Scalar.toBigints(b_arr) if b_arr is not None else None
                if invert:
                    res = [pow(v, -1, q) if v else 0 for v in av]
                else:
                    res, acc = [], 0 if bv is not None else 1
                    for i in range(n):
                        acc = ((av[i] if av is not None else a_const) * acc + (bv[i] if bv is not None else 0)) % q
                        res.append(acc)
                par.scalarsFromBigints(res).free()
                return (time.perf_counter() - t0) * 1e3

            # (name, device call, bytes per element, products per element, host route arguments).  Bytes: the tile launch
            # reads the operands, the apply launch reads them again and writes the result (its second look at an entry,
            # just before the store, is taken as a cache hit); the inverse reads, looks again and writes.  Products: the
            # per-element bodies of DESIGN.md section 19, without the per-thread shuffle scans.
            legs = [
                ("sums", lambda: recurrence(0, None, y.handle), 96, 0, (None, 1, y, False)),
                ("geometric", lambda: recurrence(0, zb, 0), 32, 3, (None, z, None, False)),
                ("horner", lambda: recurrence(0, zb, y.handle), 96, 5, (None, z, y, False)),
                ("products", lambda: recurrence(x.handle, None, 0), 96, 6, (x, 1, None, False)),
                ("general", lambda: recurrence(x.handle, None, y.handle), 160, 8, (x, 1, y, False)),
                ("inverse", inverse, 64, 5.5, (x, 1, None, True)),
            ]
            for name, call, nbytes, products, host_args in legs:
                ms = timed(call, args.reps)
                cms = copy_ms(nbytes * n // 2)   # reads and writes nbytes * n / 2 each: the same traffic
                row = {"curve": params["label"], "log2n": logn, "leg": name, "ms": round(ms, 4),
                       "bytes_per_element": nbytes, "products_per_element": products,
                       "gb_per_s": round(nbytes * n / (ms * 1e-3) / 1e9, 2), "reps": args.reps,
                       "copy_ms": round(cms, 4), "fraction_of_copy_rate": round(cms / ms, 4)}
                if logn <= args.host_max_logn:
                    row["host_route_ms"] = round(host(*host_args), 2)
                    row["host_route_over_device"] = round(row["host_route_ms"] / ms, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
            x.free()
            y.free()
        curve.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
