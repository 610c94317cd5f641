#!/usr/bin/env python3
"""What msmz_matrix_mul costs, beside innerProduct over as many elements as the matrix has non-zeros: the same count of
products, 64 streamed bytes per element and no gather -- the project's own measured rate for a sum of products.
BLS12-377 and Pallas, generated resident sets, ONE process.

    python tools/matvec_report.py [--out FILE] [--reps R] [--lognnz 20 24] [--curves LABEL ...]

Per curve and non-zero count, with values and without, three structures at (nearly) equal nnz:
    one_per_row   n rows of one entry, a random column each (a gather)
    r1cs          n / 4 rows of three random columns plus column 0, which every row references; the plain product has
                  rows of four, the transposed one ONE row of n / 4 entries among short ones
    one_row       every non-zero in row 0
The legs of a comparison ALTERNATE inside one loop, call by call, after two warm-up calls of each; a call is timed by the
host clock around the whole C call, which ends behind its host wait, and a result handle is freed outside the timed
region.  Reported per leg: median, fastest and slowest of `reps` calls (the spread).  bytes: what the call must move --
per non-zero two indices (8), the gathered entry of x (32) and the value (32, if any), per output entry one record
written (32); the innerProduct leg 64 per element.  GB/s = bytes over the median; per_nnz_ns = median over nnz;
vs_inner_product = median over the innerProduct median of the same loop.  One JSON line per leg, to stdout and appended
to --out (default profiles/matvec_report.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def structures(nnz, seed):
    """name -> (rows, cols, (n_rows, n_cols)) as numpy uint32 arrays"""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = {}
    out["one_per_row"] = (np.arange(nnz, dtype=np.uint32), rng.integers(0, nnz, nnz, dtype=np.uint32), (nnz, nnz))
    n = nnz // 4
    rows = np.repeat(np.arange(n, dtype=np.uint32), 4)
    cols = rng.integers(1, n, 4 * n, dtype=np.uint32)
    cols[0::4] = 0
    out["r1cs"] = (rows, cols, (n, n))
    out["one_row"] = (np.zeros(nnz, dtype=np.uint32), rng.integers(0, nnz, nnz, dtype=np.uint32), (1, nnz))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matvec_report.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lognnz", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    args = ap.parse_args()
    import msm_zprize_amd as m
    m.startThreads()
    lines = []

    def clock(call):
        t0 = time.perf_counter()
        res = call()
        ms = (time.perf_counter() - t0) * 1e3
        if hasattr(res, "free"):
            res.free()
        return ms

    def compare(legs):
        for _, call in legs:
            clock(call)
            clock(call)
        times = {name: [] for name, _ in legs}
        for _ in range(args.reps):
            for name, call in legs:
                times[name].append(clock(call))
        return times

    for params in m.curves.ALL_CURVES:
        if params["label"] not in args.curves:
            continue
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        par = curve.Parallel
        for lognnz in args.lognnz:
            nnz = 1 << lognnz
            vals, x, f, g = (par.randomScalars(nnz, seed) for seed in (41, 42, 43, 44))
            for name, (rows, cols, shape) in structures(nnz, lognnz).items():
                for with_values in (True, False):
                    t0 = time.perf_counter()
                    mat = par.sparseMatrix(rows, cols, vals if with_values else None, shape=shape,
                                           orientations="both" if name == "r1cs" else "rows")
                    create_ms = (time.perf_counter() - t0) * 1e3
                    per = 8 + 32 + (32 if with_values else 0)
                    legs = [("matVec", lambda: par.matVec(mat, x), nnz * per + shape[0] * 32)]
                    if name == "r1cs":
                        legs.append(("matVec transpose", lambda: par.matVec(mat, x, transpose=True), nnz * per + shape[1] * 32))
                    legs.append(("innerProduct", lambda: par.innerProduct(f, g), nnz * 64))
                    times = compare([(leg, call) for leg, call, _ in legs])
                    base = statistics.median(times["innerProduct"])
                    for leg, _, nbytes in legs:
                        ms = statistics.median(times[leg])
                        row = {"curve": params["label"], "log2nnz": lognnz, "structure": name, "values": with_values, "leg": leg,
                               "shape": list(shape), "ms": round(ms, 4), "ms_min": round(min(times[leg]), 4),
                               "ms_max": round(max(times[leg]), 4), "reps": args.reps, "bytes": nbytes,
                               "bytes_per_nnz": round(nbytes / nnz, 1), "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                               "per_nnz_ns": round(ms * 1e6 / nnz, 4), "vs_inner_product": round(ms / base, 2),
                               "create_ms": round(create_ms, 1)}
                        lines.append(row)
                        print(json.dumps(row), flush=True)
                    mat.free()
            for arr in (vals, x, f, g):
                arr.free()
        curve.close()
    with open(args.out, "a") as fh:
        for row in lines:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
