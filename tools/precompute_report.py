#!/usr/bin/env python3
"""Precomputed point sets against the plain handle: BLS12-377 G1, resident points and scalars.

    python tools/precompute_report.py [--out FILE] [--shape B:LOG2N ...] [--factor F ...] [--c C ...] [--reps R]

For every shape (default B in {1, 16} x n in {2^12, 2^14, 2^16, 2^18, 2^20}) and factor (default 2 and 0 = K, all
windows in one bucket set) it times the precomputation once, then the batched MSM (msmz_msm_batch_resident; B = 1 is
exactly msmz_msm_resident) over the plain and over the precomputed handle, checks that both give the same results, and
prints one JSON line per (shape, factor): median milliseconds of `reps` timed repetitions after one warm-up, the
precomputed set's c / copies / K / records and its memory footprint.  --c sweeps the precomputed set's window size
(default: the engine's choice); window sizes the set refuses are reported as such.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", action="append", default=None, help="B:LOG2N")
    ap.add_argument("--factor", action="append", type=int, default=None)
    ap.add_argument("--c", action="append", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shape] if a.shape else \
        [(b, lg) for lg in (12, 14, 16, 18, 20) for b in (1, 16)]
    factors = a.factor if a.factor else [2, 0]
    import msm_zprize_amd as m
    m.startThreads()
    curve = m.Weierstrass.create(m.curves.bls12377Params)
    par = curve.Parallel
    rec_bytes = 128   # BLS12-377 records at the padded point stride

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), r

    lines = []
    for B, lg in shapes:
        n = 1 << lg
        pts = par.randomPointsFast(n, 1)
        sc = par.randomScalars(B * n, 2)
        t_plain, r_plain = timed(lambda: par.msmBatchUnsafe(sc, pts, n))
        plog = par.lastBatchLog
        for f, cc in [(f, cc) for f in factors for cc in (a.c or [0])]:
            t0 = time.perf_counter()
            try:
                pre = par.precomputePoints(pts, n, {"c": cc} if cc else None, f)
            except m._native.MsmzError as e:
                rec = {"curve": "bls12-377", "B": B, "log2n": lg, "factor_arg": f, "c_arg": cc, "refused": e.status}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                continue
            t_pre = (time.perf_counter() - t0) * 1e3
            t_fast, r_fast = timed(lambda: par.msmBatchUnsafe(sc, pre, n))
            log = par.lastBatchLog
            if r_fast != r_plain:
                raise SystemExit(f"precomputed and plain disagree at B = {B}, n = 2^{lg}, factor {f}")
            info = pre.info
            rec = {"curve": "bls12-377", "B": B, "log2n": lg, "factor_arg": f, "c_arg": cc, "plain_ms": round(t_plain, 3),
                   "plain_c": plog.c, "plain_rounds": plog.rounds, "pre_ms": round(t_fast, 3),
                   "speedup": round(t_plain / t_fast, 3), "precompute_ms": round(t_pre, 2), "c": info["c"],
                   "glv": info["glv"], "copies": info["factor"], "K": info["K"], "records": info["records"],
                   "footprint_mb": round(info["records"] * rec_bytes / 2 ** 20, 1),
                   "plain_footprint_mb": round(n * 2 * rec_bytes / 2 ** 20, 1), "pre_rounds": log.rounds,
                   "pre_max_bucket": log.max_bucket}
            pre.free()
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        sc.free()
        pts.free()
    curve.close()
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
