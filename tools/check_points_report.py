#!/usr/bin/env python3
"""What msmz_check_points costs.  All four curves, generated (all-good) resident sets, ONE process.

    python tools/check_points_report.py [--out FILE] [--reps R] [--logn 16 20 22] [--curves LABEL ...]

For every curve and size it times what = CURVE and what = CURVE | SUBGROUP (no verdict bytes fetched): median wall
milliseconds of `reps` calls after one warm-up.  Beside each leg: the field products of its arithmetic (squarings counted
as products) and the fraction of the field-multiply peak that rate is.  The product count is the chain's own: BITS
doublings and one mixed addition per set bit of q (9 and 10 products on the Weierstrass curves, 9 and 7 on the twisted
Edwards curve), 3 or 4 products for the curve equation.  The peak is the measured fe_mul rate of
profiles/r01_ubench_fp_modmul.txt (14 x 28-bit limbs: 72 G/s BLS12-377, 67 G/s BLS12-381; 9 x 29-bit limbs: 165 G/s).
One JSON line per leg, to stdout and to --out (default profiles/check_points_report.jsonl).
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

PEAK_GMODMUL = {"bls12-377": 72.0, "bls12-381": 67.0, "pallas": 165.0, "ed-on-bls12-377": 165.0}


def products(params, what):
    """field products per point of one call"""
    te = params["kind"] == "twisted-edwards"
    n = 4 if te else 3
    if what & 2 and params["cofactor"] != 1:
        q = params["order"]
        dbl, add = (9, 7) if te else (9, 10)
        n += q.bit_length() * dbl + bin(q).count("1") * add
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_points_report.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--curves", nargs="+", default=None)
    args = ap.parse_args()
    import msm_zprize_amd as m
    from msm_zprize_amd._native import MsmzCheckResult, check, lib
    m.startThreads()
    rows = []
    for params in m.curves.ALL_CURVES:
        if args.curves and params["label"] not in args.curves:
            continue
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        for logn in args.logn:
            n = 1 << logn
            pts = curve.Parallel.randomPointsFast(n, 11)
            for what, name in ((1, "curve"), (3, "curve+subgroup")):
                res = MsmzCheckResult()

                def call():
                    t0 = time.perf_counter()
                    check(lib().msmz_check_points(curve._ctx, pts.handle, 0, n, what, C.byref(res), None), "msmz_check_points")
                    return (time.perf_counter() - t0) * 1e3

                call()
                ms = statistics.median(call() for _ in range(args.reps))
                if (res.off_curve, res.off_subgroup) != (0, 0):
                    raise SystemExit(f"{params['label']}: a generated set failed the check: {res.off_curve}, {res.off_subgroup}")
                prod = products(params, what)
                rate = prod * n / (ms * 1e-3) / 1e9
                row = {"curve": params["label"], "log2n": logn, "what": name, "ms": round(ms, 4),
                       "mpoints_per_s": round(n / ms / 1e3, 3), "products_per_point": prod,
                       "gmodmul_per_s": round(rate, 3), "peak_gmodmul_per_s": PEAK_GMODMUL[params["label"]],
                       "fraction_of_peak": round(rate / PEAK_GMODMUL[params["label"]], 4), "reps": args.reps}
                rows.append(row)
                print(json.dumps(row), flush=True)
            pts.free()
        curve.close()
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
