#!/usr/bin/env python3
"""What msmz_points_fixed_base costs, against the only other route to the same set.  ONE process.

    python tools/fixed_base_report.py [--out FILE] [--reps R] [--logn 12 16 20] [--curves LABEL ...] [--sweep-logn 20]

For every curve (default BLS12-377 and Pallas) and size it times whole calls with a host clock -- every call returns
after the GPU has finished -- as the median wall milliseconds of `reps` calls after one warm-up, the legs of one setting
alternating inside each repetition, the result handle freed outside the timed region:
    fixed cached      msmz_points_fixed_base on a base whose table is in the cache
    fixed cold        the same on a base not seen before: a resident record is downloaded, its bases 2^(ck) B are made on
                      the host, the table is built on the device, then the points
    points_mul        msmz_points_mul_opts over n resident copies of B with the same scalars and the same bound:
                      unchanged code, the baseline
for full-width scalars (randomScalars) and for scalars below 2^64 with scalar_bits = 64.  Beside each leg: the spread of
the repetitions ((max - min) / median), the field products per point of the cost MODEL (fixed_point_products of
csrc/fixed_base.h, points_mul_products(_bounded) of csrc/mul_kernels.h) and, on the fixed legs, the ratio measured
(points_mul ms / fixed ms) next to the ratio the product model predicts.
--sweep-logn: at that size the planner's width and one width either side of it, forced through
msmz_test_set_fixed_base_window, tables cached, full-width scalars.
One JSON line per leg, to stdout and appended to --out (default profiles/fixed_base_report.jsonl).
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mul_products(params, bits):
    """points_mul_products_bounded without an addend (csrc/mul_kernels.h)"""
    if params["kind"] == "twisted-edwards":
        return bits * 9 + (bits // 2) * 7 + 18
    return bits * 9 + (bits // 2) * 10 + 19


def fixed_products(params, K):
    """fixed_point_products (csrc/fixed_base.h)"""
    te = params["kind"] == "twisted-edwards"
    return K * (9 if te else 10) + 14 + (4 if te else 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_base_report.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logn", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    ap.add_argument("--sweep-logn", type=int, default=20)
    args = ap.parse_args()
    import msm_zprize_amd as m
    from msm_zprize_amd._native import MsmzFixedBase, MsmzMul, MsmzMulOpts, check, lib
    m.startThreads()
    L = lib()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for params in m.curves.ALL_CURVES:
        if params["label"] not in args.curves:
            continue
        cid = m.curves.ALL_CURVES.index(params)
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        fb = curve.fe_bytes
        order_bits = params["order"].bit_length()
        # bases: record 0 is B of the cached legs and of the copies; every cold call takes a record not used before
        n_bases = 2 + 2 * len(args.logn) * (args.reps + 1)
        bases = curve.Parallel.randomPointsFast(n_bases, 21)
        xy = C.create_string_buffer(2 * fb)
        check(L.msmz_download_points(curve._ctx, bases.handle, 0, 1, xy, None), "msmz_download_points")
        fresh = iter(range(1, n_bases))

        def plan(n, bits):
            c, K, e = C.c_int32(), C.c_int32(), C.c_uint64()
            check(L.msmz_test_fixed_base_plan(cid, n, bits, C.byref(c), C.byref(K), C.byref(e)), "msmz_test_fixed_base_plan")
            return c.value, K.value, e.value

        def timed(call):
            h = C.c_uint64()
            t0 = time.perf_counter()
            call(h)
            ms = (time.perf_counter() - t0) * 1e3
            check(L.msmz_free(curve._ctx, h.value), "msmz_free")
            return ms

        for logn in args.logn:
            n = 1 << logn
            copies = curve.Parallel.pointsFromBytes(xy.raw * n, n)
            full = curve.Parallel.randomScalars(n, 13)
            short = curve.Parallel.scalarsFromBytes(random.Random(14).randbytes(8 * n), n, width=8)
            for setting, sc, bits in (("full", full, 0), ("64-bit", short, 64)):
                eff = order_bits if bits == 0 else bits
                c, K, entries = plan(n, bits)

                def fixed(index):
                    f = MsmzFixedBase(bases.handle, index, None, sc.handle, 0, bits, 0)
                    return lambda h: check(L.msmz_points_fixed_base(curve._ctx, C.byref(f), n, C.byref(h)), "msmz_points_fixed_base")

                def baseline(h):
                    desc = MsmzMul(copies.handle, 0, sc.handle, 0, None, 0, 0)
                    o = MsmzMulOpts(0, bits)
                    check(L.msmz_points_mul_opts(curve._ctx, C.byref(desc), n, C.byref(o), C.byref(h)), "msmz_points_mul_opts")

                timed(fixed(0)), timed(baseline), timed(fixed(next(fresh)))   # warm-up: code objects, buffers, table 0
                ms = {"fixed cached": [], "fixed cold": [], "points_mul": []}
                for _ in range(args.reps):
                    ms["fixed cached"].append(timed(fixed(0)))
                    ms["points_mul"].append(timed(baseline))
                    ms["fixed cold"].append(timed(fixed(next(fresh))))
                med = {k: statistics.median(v) for k, v in ms.items()}
                model = {"fixed cached": fixed_products(params, K), "fixed cold": fixed_products(params, K),
                         "points_mul": mul_products(params, eff)}
                for leg in ("fixed cached", "fixed cold", "points_mul"):
                    row = {"curve": params["label"], "log2n": logn, "scalars": setting, "leg": leg, "ms": round(med[leg], 4),
                           "spread": round((max(ms[leg]) - min(ms[leg])) / med[leg], 4),
                           "mpoints_per_s": round(n / med[leg] / 1e3, 3), "model_products_per_point": model[leg],
                           "reps": args.reps}
                    if leg != "points_mul":
                        row.update({"c": c, "K": K, "table_mib": round(entries * 2 * fb / 2 ** 20, 3),
                                    "measured_ratio": round(med["points_mul"] / med[leg], 2),
                                    "model_ratio": round(model["points_mul"] / model[leg], 2)})
                    emit(row)
            if logn == args.sweep_logn:
                c0, _, _ = plan(n, 0)
                f = MsmzFixedBase(bases.handle, 0, None, full.handle, 0, 0, 0)
                call = lambda h: check(L.msmz_points_fixed_base(curve._ctx, C.byref(f), n, C.byref(h)), "msmz_points_fixed_base")
                widths = [w for w in (c0 - 1, c0, c0 + 1) if 4 <= w <= 16]
                ms = {w: [] for w in widths}
                for w in widths:
                    check(L.msmz_test_set_fixed_base_window(curve._ctx, w), "msmz_test_set_fixed_base_window")
                    timed(call)
                for _ in range(args.reps):
                    for w in widths:
                        check(L.msmz_test_set_fixed_base_window(curve._ctx, w), "msmz_test_set_fixed_base_window")
                        ms[w].append(timed(call))
                check(L.msmz_test_set_fixed_base_window(curve._ctx, 0), "msmz_test_set_fixed_base_window")
                for w in widths:
                    med = statistics.median(ms[w])
                    K = (order_bits + w) // w
                    emit({"curve": params["label"], "log2n": logn, "scalars": "full", "leg": "width sweep", "c": w, "K": K,
                          "planner": w == c0, "ms": round(med, 4), "spread": round((max(ms[w]) - min(ms[w])) / med, 4),
                          "table_mib": round((K << (w - 1)) * 2 * fb / 2 ** 20, 3),
                          "model_products_per_point": fixed_products(params, K), "reps": args.reps})
            for a in (copies, full, short):
                a.free()
        bases.free()
        curve.close()
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
