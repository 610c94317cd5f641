#!/usr/bin/env python3
"""What msmz_scalars_combine / _dot / _powers cost.  BLS12-377 and Pallas, generated resident sets, ONE process.

    python tools/scalar_ops_report.py [--out FILE] [--reps R] [--logn 16 20 24] [--host-max-logn L] [--curves LABEL ...]

For every curve and size it times, as the median wall milliseconds of `reps` calls after one warm-up (a result handle is
freed outside the timed region):
    combine a x / c . x / a x + b y / c . x + d . y     one and two terms, broadcast and resident coefficients
    dot <x, y> / sum x                                  msmz_scalars_dot
    powers                                              msmz_scalars_powers
Beside each leg:
    host route  what a caller has without these calls: msmz_download_scalars, the same arithmetic with Python integers,
                msmz_upload_scalars -- ONE run (it takes seconds to minutes), sizes up to 2^host-max-logn;
    copy        (beside combine) a plain device-to-device copy that moves the same number of bytes, the memory-bound
                yardstick, through torch (imported before the library is loaded: a process drives the GPU through one
                copy of the HIP runtime).
Reported: bytes moved per element (32 per record read or written), Montgomery products per element (1 per broadcast
coefficient, 2 per resident one or per canonical product, 1 per element of a dot product, at most 32 / SPOW_RUN + 1 for
powers), GB/s, and for combine the fraction of the copy's rate.  One JSON line per leg, to stdout and appended to --out
(default profiles/scalar_ops_report.jsonl).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_ops_report.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--host-max-logn", type=int, default=24)
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    args = ap.parse_args()
    import torch   # before libmsmz.so
    import msm_zprize_amd as m
    from msm_zprize_amd._native import MsmzScalarTerm, check, lib
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
        a, b = q * 5 // 7, q * 3 // 11
        ab, bb = a.to_bytes(32, "little"), b.to_bytes(32, "little")
        for logn in args.logn:
            n = 1 << logn
            x, y, c, d = (par.randomScalars(n, seed) for seed in (21, 22, 23, 24))

            def combine(tx, ty):
                h = C.c_uint64(0)
                t0 = time.perf_counter()
                check(lib().msmz_scalars_combine(ctx, C.byref(tx), None if ty is None else C.byref(ty), n, 0, C.byref(h)),
                      "msmz_scalars_combine")
                ms = (time.perf_counter() - t0) * 1e3
                check(lib().msmz_free(ctx, h.value), "msmz_free")
                return ms

            def dot(yh):
                out = C.create_string_buffer(32)
                t0 = time.perf_counter()
                check(lib().msmz_scalars_dot(ctx, x.handle, 0, yh, 0, n, out), "msmz_scalars_dot")
                return (time.perf_counter() - t0) * 1e3

            def powers():
                h = C.c_uint64(0)
                t0 = time.perf_counter()
                check(lib().msmz_scalars_powers(ctx, bb, ab, n, C.byref(h)), "msmz_scalars_powers")
                ms = (time.perf_counter() - t0) * 1e3
                check(lib().msmz_free(ctx, h.value), "msmz_free")
                return ms

            def host(fn, arrays, upload):
                """download, Python integers, upload: one run"""
                t0 = time.perf_counter()
                vals = [curve.Scalar.toBigints(arr) for arr in arrays]
                res = fn(*vals)
                if upload:
                    par.scalarsFromBigints(res).free()
                return (time.perf_counter() - t0) * 1e3

            T = MsmzScalarTerm
            # (name, device call, bytes per element, products per element, host arithmetic, its arrays, it uploads)
            legs = [
                ("combine a x", lambda: combine(T(x.handle, 0, 0, 0, ab), None), 64, 1,
                 lambda xs: [a * v % q for v in xs], (x,), True),
                ("combine c . x", lambda: combine(T(x.handle, 0, c.handle, 0, None), None), 96, 2,
                 lambda xs, cs: [w * v % q for w, v in zip(cs, xs)], (x, c), True),
                ("combine a x + b y", lambda: combine(T(x.handle, 0, 0, 0, ab), T(y.handle, 0, 0, 0, bb)), 96, 2,
                 lambda xs, ys: [(a * u + b * v) % q for u, v in zip(xs, ys)], (x, y), True),
                ("combine c . x + d . y", lambda: combine(T(x.handle, 0, c.handle, 0, None), T(y.handle, 0, d.handle, 0, None)), 160, 4,
                 lambda xs, ys, cs, ds: [(w * u + z * v) % q for w, u, z, v in zip(cs, xs, ds, ys)], (x, y, c, d), True),
                ("dot <x, y>", lambda: dot(y.handle), 64, 1, lambda xs, ys: sum(u * v for u, v in zip(xs, ys)) % q, (x, y), False),
                ("sum x", lambda: dot(0), 32, 0, lambda xs: sum(xs) % q, (x,), False),
                ("powers", powers, 32, 5, None, (), True),
            ]
            for name, call, nbytes, products, host_fn, arrays, upload in legs:
                ms = timed(call, args.reps)
                row = {"curve": params["label"], "log2n": logn, "leg": name, "ms": round(ms, 4),
                       "bytes_per_element": nbytes, "products_per_element": products,
                       "gb_per_s": round(nbytes * n / (ms * 1e-3) / 1e9, 2), "reps": args.reps}
                if name.startswith("combine"):
                    cms = copy_ms(nbytes * n // 2)   # reads and writes nbytes * n / 2 each: the same traffic
                    row["copy_ms"] = round(cms, 4)
                    row["fraction_of_copy_rate"] = round(cms / ms, 4)
                if logn <= args.host_max_logn:
                    if host_fn is None:   # powers: nothing to download
                        def pw():
                            t0 = time.perf_counter()
                            vals, acc = [], b
                            for _ in range(n):
                                vals.append(acc)
                                acc = acc * a % q
                            par.scalarsFromBigints(vals).free()
                            return (time.perf_counter() - t0) * 1e3
                        row["host_route_ms"] = round(pw(), 2)
                    else:
                        row["host_route_ms"] = round(host(host_fn, arrays, upload), 2)
                    row["host_route_over_device"] = round(row["host_route_ms"] / ms, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
            for arr in (x, y, c, d):
                arr.free()
        curve.close()
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
