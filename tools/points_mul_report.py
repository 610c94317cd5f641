#!/usr/bin/env python3
"""What msmz_points_mul and msmz_points_mul_opts cost.  All four curves, generated resident sets, ONE process.

    python tools/points_mul_report.py [--out FILE] [--reps R] [--logn 16 20] [--curves LABEL ...]

For every curve and size it times, as the median wall milliseconds of `reps` calls after one warm-up (the result handle of
every call is freed outside the timed region):
    mul             msmz_points_mul, resident full-width scalars (randomScalars), no addend
    mul+addend      the same with an addend set
    mul broadcast   one full-width scalar for every point, no addend
    subgroup check  msmz_check_points(SUBGROUP) of the same set: the yardstick.  A chain of the same length (BITS
                    doublings, wt(q) additions; Pallas, cofactor 1, runs none), no normalisation, no store.
and through msmz_points_mul_opts (the chain each call runs is points_mul_chain's):
    mul subgroup, mul+addend subgroup, mul broadcast subgroup
                    the three legs above under MSMZ_MUL_SUBGROUP: the GLV chain on the Weierstrass curves
    mul broadcast 128-bit   one scalar below 2^128 with scalar_bits = 128
    mul 64-bit      resident scalars below 2^64 with scalar_bits = 64
Beside each leg: the field products of the cost MODEL (squarings counted as products; points_mul_products of
csrc/mul_kernels.h: a scalar of Hamming weight BITS / 2, the addend, 19 / 18 products for the wave-wide normalisation;
points_mul_products_glv / _bounded for the legs with options)
and the fraction of the measured fe_mul peak (profiles/r01_ubench_fp_modmul.txt) that rate would be.  The model is a
model: a wave pays for the addition whenever ANY of its lanes has the bit set, which the count ignores.
One JSON line per leg, to stdout and appended to --out (default profiles/points_mul_report.jsonl).
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


GLV_PROVEN_BITS = {"bls12-377": 126, "pallas": 128, "bls12-381": 128}   # Fr::GLV_PROVEN_BITS (csrc/constants_gen.h)
MSMZ_MUL_SUBGROUP = 1


def mul_products(params, addend, bits=None):
    """field products per output point: the model of points_mul_products / points_mul_products_bounded (csrc/mul_kernels.h)"""
    bits = bits or params["order"].bit_length()
    if params["kind"] == "twisted-edwards":
        return bits * 9 + (bits // 2) * 7 + (7 if addend else 0) + 18
    return bits * 9 + (bits // 2) * 10 + (10 if addend else 0) + 19


def glv_products(params, addend):
    """points_mul_products_glv (csrc/mul_kernels.h); the curve without an endomorphism runs the plain chain"""
    h = GLV_PROVEN_BITS.get(params["label"])
    if not h:
        return mul_products(params, addend)
    return h * 9 + (3 * h // 4) * 10 + 1 + 14 + 3 + (10 if addend else 0) + 19


def check_products(params):
    """as tools/check_points_report.py: the chain [q]P and the curve equation"""
    te = params["kind"] == "twisted-edwards"
    n = 4 if te else 3
    if params["cofactor"] != 1:
        q = params["order"]
        n += q.bit_length() * 9 + bin(q).count("1") * (7 if te else 10)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_mul_report.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--curves", nargs="+", default=None)
    args = ap.parse_args()
    import msm_zprize_amd as m
    import random
    from msm_zprize_amd._native import MsmzCheckResult, MsmzMul, MsmzMulOpts, check, lib
    m.startThreads()
    rows = []
    for params in m.curves.ALL_CURVES:
        if args.curves and params["label"] not in args.curves:
            continue
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        u = (params["order"] * 5 // 7).to_bytes(32, "little")   # full width, about half its bits set
        u128 = ((1 << 128) * 5 // 7).to_bytes(32, "little")
        for logn in args.logn:
            n = 1 << logn
            pts = curve.Parallel.randomPointsFast(n, 11)
            add = curve.Parallel.randomPointsFast(n, 12)
            sc = curve.Parallel.randomScalars(n, 13)
            sc64 = curve.Parallel.scalarsFromBytes(random.Random(14).randbytes(8 * n), n, width=8)

            def mul(desc, flags=None, bits=0):
                h = C.c_uint64()
                opts = None if flags is None else MsmzMulOpts(flags, bits)
                t0 = time.perf_counter()
                if opts is None:
                    check(lib().msmz_points_mul(curve._ctx, C.byref(desc), n, C.byref(h)), "msmz_points_mul")
                else:
                    check(lib().msmz_points_mul_opts(curve._ctx, C.byref(desc), n, C.byref(opts), C.byref(h)), "msmz_points_mul_opts")
                ms = (time.perf_counter() - t0) * 1e3
                check(lib().msmz_free(curve._ctx, h.value), "msmz_free")
                return ms

            def subgroup():
                res = MsmzCheckResult()
                t0 = time.perf_counter()
                check(lib().msmz_check_points(curve._ctx, pts.handle, 0, n, 2, C.byref(res), None), "msmz_check_points")
                ms = (time.perf_counter() - t0) * 1e3
                if (res.off_curve, res.off_subgroup) != (0, 0):
                    raise SystemExit(f"{params['label']}: a generated set failed the check")
                return ms

            legs = [("mul", lambda: mul(MsmzMul(pts.handle, 0, sc.handle, 0, None, 0, 0)), mul_products(params, False)),
                    ("mul+addend", lambda: mul(MsmzMul(pts.handle, 0, sc.handle, 0, None, add.handle, 0)), mul_products(params, True)),
                    ("mul broadcast", lambda: mul(MsmzMul(pts.handle, 0, 0, 0, u, 0, 0)), mul_products(params, False)),
                    ("subgroup check", subgroup, check_products(params)),
                    ("mul subgroup", lambda: mul(MsmzMul(pts.handle, 0, sc.handle, 0, None, 0, 0), MSMZ_MUL_SUBGROUP),
                     glv_products(params, False)),
                    ("mul+addend subgroup", lambda: mul(MsmzMul(pts.handle, 0, sc.handle, 0, None, add.handle, 0), MSMZ_MUL_SUBGROUP),
                     glv_products(params, True)),
                    ("mul broadcast subgroup", lambda: mul(MsmzMul(pts.handle, 0, 0, 0, u, 0, 0), MSMZ_MUL_SUBGROUP),
                     glv_products(params, False)),
                    ("mul broadcast 128-bit", lambda: mul(MsmzMul(pts.handle, 0, 0, 0, u128, 0, 0), 0, 128),
                     mul_products(params, False, 128)),
                    ("mul 64-bit", lambda: mul(MsmzMul(pts.handle, 0, sc64.handle, 0, None, 0, 0), 0, 64),
                     mul_products(params, False, 64))]
            for name, call, prod in legs:
                call()
                ms = statistics.median(call() for _ in range(args.reps))
                rate = prod * n / (ms * 1e-3) / 1e9
                row = {"curve": params["label"], "log2n": logn, "leg": name, "ms": round(ms, 4),
                       "mpoints_per_s": round(n / ms / 1e3, 3), "model_products_per_point": prod,
                       "model_gmodmul_per_s": round(rate, 3), "peak_gmodmul_per_s": PEAK_GMODMUL[params["label"]],
                       "model_fraction_of_peak": round(rate / PEAK_GMODMUL[params["label"]], 4), "reps": args.reps}
                rows.append(row)
                print(json.dumps(row), flush=True)
            for a in (pts, add, sc, sc64):
                a.free()
        curve.close()
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
