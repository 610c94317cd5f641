#!/usr/bin/env python3
"""What msmz_scalars_eq_table / _mle_eval / _mle_bind / _sumcheck_round cost, each beside the route the older calls
give for the same thing.  BLS12-381 and BLS12-377, generated resident sets, ONE process.

    python tools/mle_report.py [--out FILE] [--reps R] [--logn 20 24] [--curves LABEL ...]

Per curve and size, four comparisons.  The two sides of a comparison ALTERNATE inside one loop, call by call, after two
warm-up calls of each; a call is timed by the host clock around the whole C call, which ends behind its host wait, and a
result handle is freed outside the timed region.  Reported per leg: median, fastest and slowest of `reps` calls.
    1  eqTable(r)                     | scalarPowers of the same length      one write stream, a few products per entry
    2  evaluateMle(f, r)              | innerProduct(f, g)                   the same read of f; eval generates g
    3  bindMle(f, r), high variable   | combineScalars(1 - r, f, r, f, h)    the same bytes moved
    4  sumcheckRound, 2 tables 1 term | 2 combineScalars (2 hi - lo) + 3 innerProduct: the older calls' route to the same
                                        three values g(0), g(1), g(2)
    4b sumcheckRound, 4 tables 2 terms (eq A B - eq C), no counterpart
bytes: what the leg must read and write (32 per record); GB/s = bytes over the median; hbm_fraction = GB/s over the
6290 GB/s a float4 copy reaches on this part.  One JSON line per leg, to stdout and appended to --out (default
profiles/mle_report.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GB_S = 6290.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_report.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--logn", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--curves", nargs="+", default=["bls12-381", "bls12-377"])
    args = ap.parse_args()
    import msm_zprize_amd as m
    m.startThreads()
    rows = []

    def clock(call):
        """call() -> what to free; the wall milliseconds of the call alone"""
        t0 = time.perf_counter()
        res = call()
        ms = (time.perf_counter() - t0) * 1e3
        for arr in res if isinstance(res, (list, tuple)) else (res,):
            if hasattr(arr, "free"):
                arr.free()
        return ms

    def compare(legs):
        """legs: [(name, call)] -> {name: [ms, ...]}, the legs alternating"""
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
        q = params["order"]
        par = curve.Parallel
        for logn in args.logn:
            n, h = 1 << logn, 1 << (logn - 1)
            point = [q * (3 + j) // (7 + 2 * j) for j in range(logn)]
            r = q * 5 // 7
            f, g, a, b = (par.randomScalars(n, seed) for seed in (31, 32, 33, 34))
            e = par.eqTable(point)

            def five_calls():
                """g(0) = <f_lo, g_lo>, g(1) = <f_hi, g_hi>, g(2) = <2 f_hi - f_lo, 2 g_hi - g_lo>"""
                f2 = par.combineScalars(q - 1, f, 2, f, h, 0, h)
                g2 = par.combineScalars(q - 1, g, 2, g, h, 0, h)
                par.innerProduct(f, g, h)
                par.innerProduct(f, g, h, h, h)
                par.innerProduct(f2, g2)
                return [f2, g2]

            rec = 32
            comparisons = [
                (1, [("eqTable", lambda: par.eqTable(point), n * rec),
                     ("scalarPowers", lambda: par.scalarPowers(r, n), n * rec)]),
                (2, [("evaluateMle", lambda: par.evaluateMle(f, point), n * rec),
                     ("innerProduct", lambda: par.innerProduct(f, g), 2 * n * rec)]),
                (3, [("bindMle high", lambda: par.bindMle(f, r), (n + h) * rec),
                     ("combineScalars (1 - r) lo + r hi", lambda: par.combineScalars((1 - r) % q, f, r, f, h, 0, h), (n + h) * rec),
                     ("bindMle low", lambda: par.bindMle(f, r, low=True), (n + h) * rec)]),
                (4, [("sumcheckRound 2 tables 1 term", lambda: par.sumcheckRound([f, g], [(None, 3)]), 2 * n * rec),
                     ("five calls: 2 combineScalars + 3 innerProduct", five_calls, (2 * (n + h) + 6 * h) * rec),
                     ("sumcheckRound 2 tables 1 term, low", lambda: par.sumcheckRound([f, g], [(None, 3)], low=True), 2 * n * rec)]),
                ("4b", [("sumcheckRound 4 tables 2 terms", lambda: par.sumcheckRound([e, f, a, b], [(1, 0b0111), (q - 1, 0b1001)]),
                         4 * n * rec)]),
            ]
            for number, legs in comparisons:
                times = compare([(name, call) for name, call, _ in legs])
                for name, _, nbytes in legs:
                    ms = statistics.median(times[name])
                    row = {"curve": params["label"], "log2n": logn, "comparison": number, "leg": name, "ms": round(ms, 4),
                           "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4), "reps": args.reps,
                           "bytes": nbytes, "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                           "hbm_fraction": round(nbytes / (ms * 1e-3) / 1e9 / HBM_GB_S, 3)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            for arr in (f, g, a, b, e):
                arr.free()
        curve.close()
    with open(args.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
