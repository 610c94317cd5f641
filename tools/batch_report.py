#!/usr/bin/env python3
"""Batched MSM against a loop of single MSMs: BLS12-377 G1, resident points and scalars.

    python tools/batch_report.py [--out FILE] [--shape B:LOG2N ...] [--only-batch] [--reps R]

For every shape (default B in {1, 4, 16, 64} x n in {2^12, 2^14, 2^16}) it times one msmz_msm_batch_resident call of B
vectors of n scalars against B msmz_msm_resident calls (one resident scalar set per vector), checks that both give the
same B results, and prints one JSON line per shape: median milliseconds of `reps` timed repetitions after one warm-up.
--only-batch times the batched call alone (for a profiler run of one shape).
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
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shape] if a.shape else \
        [(b, lg) for lg in (12, 14, 16) for b in (1, 4, 16, 64)]
    import msm_zprize_amd as m
    m.startThreads()
    curve = m.Weierstrass.create(m.curves.bls12377Params)
    par = curve.Parallel
    lines = []
    for B, lg in shapes:
        n = 1 << lg
        pts = par.randomPointsFast(n, 1)
        sc = par.randomScalars(B * n, 2)

        def run_batch():
            return par.msmBatchUnsafe(sc, pts, n)

        def timed(fn):
            fn()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts), r

        t_batch, r_batch = timed(run_batch)
        log = par.lastBatchLog
        rec = {"curve": "bls12-377", "B": B, "log2n": lg, "batch_ms": round(t_batch, 3), "c": log.c, "K": log.K,
               "rounds": log.rounds, "n_entries": int(log.n_entries)}
        if not a.only_batch:
            raw = [bytes(sc_b) for sc_b in _vectors(curve, sc, B, n)]
            vec = [par.scalarsFromBytes(v, n) for v in raw]

            def run_loop():
                return [par.msmUnsafe(v, pts, n)["result"] for v in vec]

            t_loop, r_loop = timed(run_loop)
            if r_loop != r_batch:
                raise SystemExit(f"batch and loop disagree at B = {B}, n = 2^{lg}")
            rec.update({"loop_ms": round(t_loop, 3), "speedup": round(t_loop / t_batch, 2),
                        "batch_gadds_per_s": round(log.n_entries / t_batch / 1e6, 3)})
            for v in vec:
                v.free()
        sc.free()
        pts.free()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    curve.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def _vectors(curve, sc, B, n):
    import ctypes as C
    from msm_zprize_amd._native import check, lib
    for k in range(B):
        buf = C.create_string_buffer(32 * n)
        check(lib().msmz_download_scalars(curve._ctx, sc.handle, k * n, n, buf), "msmz_download_scalars")
        yield buf.raw


if __name__ == "__main__":
    main()
