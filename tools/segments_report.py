#!/usr/bin/env python3
"""Segmented MSM (msmz_msm_segments) against the calls it replaces: BLS12-377 G1, unsafe additions, resident scalars.

    python tools/segments_report.py [--out FILE] [--case a|b|c ...] [--reps R]

One process, one warm-up per call shape, then the median of `reps` timed repetitions (wall clock around the whole call:
every call ends with its own device-to-host fetch); the spread is (max - min) of the repetitions.  Every case checks
that both sides give the same results.  One JSON line per case, appended to profiles/segments_report.jsonl (or --out).

  a  16 equal segments of 2^16 with zero point offsets against msmz_msm_batch_resident of the same shapes: the yardstick
     is the existing batch; the segmented kernels add one descriptor load per workgroup
  b  the IPA pair, 2 x 2^19 over a 2^20 set ({n/2, 0, n/2} and {0, n/2, n/2}), against two msmz_msm_resident calls over
     separately uploaded halves
  c  16 segments with lengths spread over 2^15 .. 2^16 - 1 (one length class) against 16 single-segment calls
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


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3)}, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_report.jsonl"))
    ap.add_argument("--case", action="append", default=None, choices=["a", "b", "c"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    cases = a.case or ["a", "b", "c"]
    import msm_zprize_amd as m
    from msm_zprize_amd._native import check, lib
    m.startThreads()
    curve = m.Weierstrass.create(m.curves.bls12377Params)
    par = curve.Parallel
    fb = curve.fe_bytes
    recs = []

    def slice_points(pts, first, n):
        xy, inf = C.create_string_buffer(2 * fb * n), C.create_string_buffer(n)
        check(lib().msmz_download_points(curve._ctx, pts.handle, first, n, xy, inf), "msmz_download_points")
        return par.pointsFromBytes(xy.raw, n, inf.raw if any(inf.raw) else None)

    def slice_scalars(sc, first, n):
        buf = C.create_string_buffer(32 * n)
        check(lib().msmz_download_scalars(curve._ctx, sc.handle, first, n, buf), "msmz_download_scalars")
        return par.scalarsFromBytes(buf.raw, n)

    if "a" in cases:
        B, n = 16, 1 << 16
        pts, sc = par.randomPointsFast(n, 1), par.randomScalars(B * n, 2)
        segs = [(0, k * n, n) for k in range(B)]
        t_batch, r_batch = timed(lambda: par.msmBatchUnsafe(sc, pts, n), a.reps)
        t_seg, r_seg = timed(lambda: par.msmSegmentsUnsafe(sc, pts, segs), a.reps)
        t_batch2, _ = timed(lambda: par.msmBatchUnsafe(sc, pts, n), a.reps)   # the batch again: its own run-to-run drift
        if r_seg != r_batch:
            raise SystemExit("case a: segments and batch disagree")
        log = par.lastBatchLog
        recs.append({"case": "a", "shape": "16 x 2^16, zero point offsets", "segments": t_seg, "batch": t_batch,
                     "batch_again": t_batch2, "c": log.c, "K": log.K})
        pts.free(), sc.free()
    if "b" in cases:
        n, h = 1 << 20, 1 << 19
        pts, sc = par.randomPointsFast(n, 3), par.randomScalars(n, 4)
        lo_p, hi_p = slice_points(pts, 0, h), slice_points(pts, h, h)
        lo_s, hi_s = slice_scalars(sc, 0, h), slice_scalars(sc, h, h)
        t_seg, r_seg = timed(lambda: par.msmSegmentsUnsafe(sc, pts, [(h, 0, h), (0, h, h)]), a.reps)
        t_two, r_two = timed(lambda: [par.msmUnsafe(lo_s, hi_p, h)["result"], par.msmUnsafe(hi_s, lo_p, h)["result"]], a.reps)
        if r_seg != r_two:
            raise SystemExit("case b: segments and the two MSMs over uploaded halves disagree")
        recs.append({"case": "b", "shape": "IPA pair, 2 x 2^19 over a 2^20 set", "segments": t_seg,
                     "two_msm_resident_uploaded_halves": t_two})
        for x in (pts, sc, lo_p, hi_p, lo_s, hi_s):
            x.free()
    if "c" in cases:
        B, top = 16, 1 << 16
        rng = random.Random(5)
        lens = [rng.randrange(top // 2, top) for _ in range(B)]
        lens[0], lens[-1] = top // 2, top - 1
        pts, sc = par.randomPointsFast(top, 6), par.randomScalars(B * top, 7)
        segs = [(rng.randrange(0, top - n + 1), k * top + rng.randrange(0, top - n + 1), n) for k, n in enumerate(lens)]
        t_seg, r_seg = timed(lambda: par.msmSegmentsUnsafe(sc, pts, segs), a.reps)
        t_one, r_one = timed(lambda: [par.msmSegmentsUnsafe(sc, pts, [s])[0] for s in segs], a.reps)
        if r_seg != r_one:
            raise SystemExit("case c: one call and 16 single-segment calls disagree")
        recs.append({"case": "c", "shape": "16 segments, lengths 2^15 .. 2^16 - 1", "lengths": lens, "segments": t_seg,
                     "single_segment_calls": t_one})
        pts.free(), sc.free()
    curve.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
