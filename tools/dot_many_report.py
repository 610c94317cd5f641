#!/usr/bin/env python3
"""What msmz_scalars_dot_many buys: whole calls of it beside a loop of msmz_scalars_dot over the same (row, column)
pairs, in ONE process, the two sides alternating.

    python tools/dot_many_report.py [--out FILE] [--reps R] [--logn 12 16 20 24] [--shapes 1x1 8x1 40x2 128x1 16x8]
                                    [--curves bls12-377 pallas] [--parent-lib PATH]

The loop runs from another build of the library when --parent-lib (or the environment's MSMZ_PARENT_LIB) names one: the
parent commit's libmsmz.so, built in a checkout of that commit (msmz_scalars_dot is the yardstick and this change does
not touch it; the parent build shows that).  Without one the loop runs from the library under test and the lines say
"loop_lib": "same".  Each library gets its own context and its own vectors, generated on the device from the same
seeds, so both sides read the same values; their results are compared byte for byte before anything is timed.

Vectors: one scalar set per vector, at most MAX_DISTINCT sets per side -- larger families cycle through them (24 GiB per
side at 2^24, far beyond every cache).  Per shape and size: two warm-ups of each side, then `reps` rounds of (one
dot_many call, one loop), the host clock around each.  Per side: median, fastest and slowest.  products = rows cols n;
bytes = 32 n (rows + cols ceil(rows / RG)), the kernel's own reads; the loop's bytes are
64 n rows cols.  verdict: "wins" when the call's median is below the loop's fastest run, "inside" when it lies within the
loop's fastest .. slowest, "loses" when above the slowest.  One JSON line per shape and size, to stdout and appended to
--out (default profiles/dot_many_report.jsonl).
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
MAX_DISTINCT = 48
USED = ("msmz_create", "msmz_destroy", "msmz_random_scalars", "msmz_free", "msmz_scalars_dot")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_many_report.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--logn", type=int, nargs="+", default=[12, 16, 20, 24])
    ap.add_argument("--shapes", nargs="+", default=["1x1", "8x1", "40x2", "128x1", "16x8"])
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    ap.add_argument("--parent-lib", default=os.environ.get("MSMZ_PARENT_LIB"))
    args = ap.parse_args()
    from msm_zprize_amd import _native as N
    from msm_zprize_amd import curves

    new = N.lib()
    if args.parent_lib:
        old = C.CDLL(os.path.abspath(args.parent_lib))
        for name in USED:
            fn = getattr(old, name)
            fn.restype, fn.argtypes = N.EXPORTS[name]
    else:
        old = new
    rg = (C.c_uint32 * 8)()
    new.msmz_test_dot_many_geometry(None, None, rg)

    def ok(st, what):
        if st:
            raise RuntimeError(f"{what}: status {st}")

    def stats(ts):
        return {"ms": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}

    rows_out = []
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    for label in args.curves:
        cid = curves.BY_LABEL[label]["curve_id"]
        ctxs = []
        for lib in (new, old):
            ctx = C.c_void_p()
            ok(lib.msmz_create(C.byref(ctx), cid, (C.c_int * 1)(0), 1), "msmz_create")
            ctxs.append(ctx)
        for logn in args.logn:
            n = 1 << logn
            need = min(MAX_DISTINCT, max(r + c for r, c in shapes))
            sets = []
            for lib, ctx in zip((new, old), ctxs):
                hs = []
                for k in range(need):
                    h = C.c_uint64(0)
                    ok(lib.msmz_random_scalars(ctx, n, 100 + k, C.byref(h)), "msmz_random_scalars")
                    hs.append(h.value)
                sets.append(hs)
            for n_rows, n_cols in shapes:
                pick = lambda hs, k: hs[k % need]   # noqa: E731
                rk, ck = list(range(n_rows)), [n_rows + c for c in range(n_cols)]
                rv = (N.MsmzScalarVec * n_rows)(*[N.MsmzScalarVec(pick(sets[0], k), 0) for k in rk])
                cv = (N.MsmzScalarVec * n_cols)(*[N.MsmzScalarVec(pick(sets[0], k), 0) for k in ck])
                d = N.MsmzDotMany(rv, n_rows, cv, n_cols, n, 0)
                buf = C.create_string_buffer(32 * n_rows * n_cols)
                one = C.create_string_buffer(32)

                def call():
                    ok(new.msmz_scalars_dot_many(ctxs[0], C.byref(d), buf, 0, None), "msmz_scalars_dot_many")
                    return buf.raw

                def loop():
                    out = []
                    for r in rk:
                        for c in ck:
                            ok(old.msmz_scalars_dot(ctxs[1], pick(sets[1], r), 0, pick(sets[1], c), 0, n, one), "msmz_scalars_dot")
                            out.append(one.raw)
                    return b"".join(out)

                assert call() == loop(), "the call and the loop disagree"
                call(), loop()
                times = {"call": [], "loop": []}
                for _ in range(args.reps):
                    for name, fn in (("call", call), ("loop", loop)):
                        t0 = time.perf_counter()
                        fn()
                        times[name].append((time.perf_counter() - t0) * 1e3)
                a, b = stats(times["call"]), stats(times["loop"])
                products = n_rows * n_cols * n
                nbytes = 32 * n * (n_rows + n_cols * -(-n_rows // rg[n_cols - 1]))
                verdict = "wins" if a["ms"] < b["ms_min"] else "inside" if a["ms"] <= b["ms_max"] else "loses"
                row = {"curve": label, "log2n": logn, "rows": n_rows, "cols": n_cols, "rg": rg[n_cols - 1], "reps": args.reps,
                       "call": a, "loop": b, "loop_calls": n_rows * n_cols, "loop_lib": "parent" if old is not new else "same",
                       "speedup": round(b["ms"] / a["ms"], 2), "verdict": verdict,
                       "products": products, "gproducts_per_s": round(products / (a["ms"] * 1e-3) / 1e9, 1),
                       "bytes": nbytes, "gb_per_s": round(nbytes / (a["ms"] * 1e-3) / 1e9, 1),
                       "loop_gb_per_s": round(64 * products / (b["ms"] * 1e-3) / 1e9, 1)}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
            for lib, ctx, hs in zip((new, old), ctxs, sets):
                for h in hs:
                    ok(lib.msmz_free(ctx, h), "msmz_free")
        for lib, ctx in zip((new, old), ctxs):
            lib.msmz_destroy(ctx)
    with open(args.out, "a") as fh:
        for row in rows_out:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
