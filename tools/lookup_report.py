#!/usr/bin/env python3
"""What msmz_scalars_lookup costs, beside innerProduct over as many entries as the column has: the same 32 column bytes
per entry streamed once and no gather -- the project's own measured rate for one pass over a scalar set.  BLS12-377 and
Pallas, ONE process.

    python tools/lookup_report.py [--out FILE] [--reps R] [--logcol 20 24] [--logtable 8 16 20] [--curves LABEL ...]

Per curve, column size and table size (a table of distinct random values below 2^250), three columns:
    uniform     every entry drawn uniformly from the table
    constant    one table value everywhere (what padding looks like)
    mostly_one  90 % one table value, the rest uniform, mixed lane by lane
each with positions (col_n words more to the host) and without.  The legs of a comparison ALTERNATE inside one loop, call
by call, after two warm-up calls of each; a call is timed by the host clock around the whole C call, which ends behind
its host wait, and a result handle is freed outside the timed region.  Reported per leg: median, fastest and slowest of
`reps` calls (the spread).  bytes: what the call must move at the least -- 32 per column entry and one table entry
gathered per probe (32), 4 per slot cleared and 4 per slot written, per table entry 32 read, 4 of count cleared and 32
written, with positions 4 per column entry twice (device, then host); the innerProduct leg 32 per entry.  per_entry_ns
= median over col_n; vs_inner_product = median over the innerProduct median of the same loop.  One JSON line per leg, to
stdout and appended to --out (default profiles/lookup_report.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def records(n, rng):
    """n random 32-byte little-endian values below 2^250, as an (n, 32) uint8 array"""
    import numpy as np
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] &= 3
    return a


def columns(table, n, rng):
    """(name, (n, 32) uint8 array over the rows of `table`), one column at a time"""
    import numpy as np
    uniform = rng.integers(0, len(table), n)
    yield "uniform", table[uniform]
    yield "constant", table[np.zeros(n, dtype=np.int64)]
    yield "mostly_one", table[np.where(rng.random(n) < 0.9, 0, uniform)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_report.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--logcol", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--logtable", type=int, nargs="+", default=[8, 16, 20])
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    args = ap.parse_args()
    import numpy as np
    import msm_zprize_amd as m
    m.startThreads()
    lines = []

    def clock(call):
        t0 = time.perf_counter()
        res = call()
        ms = (time.perf_counter() - t0) * 1e3
        if isinstance(res, tuple):
            res = res[0]
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
        rng = np.random.default_rng(17)
        for logtable in args.logtable:
            tn = 1 << logtable
            table = records(tn, rng)
            t = par.scalarsFromBytes(table.tobytes(), tn)
            slots = 2
            while slots < 2 * tn:
                slots *= 2
            for logcol in args.logcol:
                n = 1 << logcol
                for name, col in columns(table, n, rng):
                    f = par.scalarsFromBytes(col.tobytes(), n)
                    del col
                    legs = [("lookup", lambda: par.lookupMultiplicities(f, t)),
                            ("lookup positions", lambda: par.lookupMultiplicities(f, t, positions=True)),
                            ("innerProduct", lambda: par.innerProduct(f))]
                    _, info = par.lookupMultiplicities(f, t)
                    assert info["missing"] == 0
                    times = compare(legs)
                    base = statistics.median(times["innerProduct"])
                    for leg, _ in legs:
                        ms = statistics.median(times[leg])
                        nbytes = 32 * n if leg == "innerProduct" else 64 * n + 8 * slots + 68 * tn + (8 * n if "positions" in leg else 0)
                        row = {"curve": params["label"], "log2col": logcol, "log2table": logtable, "column": name, "leg": leg,
                               "ms": round(ms, 4), "ms_min": round(min(times[leg]), 4), "ms_max": round(max(times[leg]), 4),
                               "reps": args.reps, "bytes": nbytes, "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                               "per_entry_ns": round(ms * 1e6 / n, 4), "vs_inner_product": round(ms / base, 2),
                               "distinct": info["distinct"]}
                        lines.append(row)
                        print(json.dumps(row), flush=True)
                    f.free()
            t.free()
        curve.close()
    with open(args.out, "a") as fh:
        for row in lines:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
