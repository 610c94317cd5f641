#!/usr/bin/env python3
"""Short scalars: what the scalar bit bound (msmz_opts.reserved[1]) buys.  BLS12-377 G1, no GLV, unsafe additions,
resident points and scalars, all in ONE process (boxes differ by ~2 %).

    python tools/short_scalars_report.py [--out FILE] [--reps R] [--shape B:LOG2N[:pre] ...] [--bits 64 128] [--c C ...]
    --parent-lib variants/libmsmz_parent.so: the same bound-0 calls on a library built from the parent commit as well

For every shape (default 2^16, 2^20, 16 x 2^16, and 16 x 2^16 over a set precomputed with factor 0) and scalars uniform
below 2^64 and below 2^128 it times the same resident scalars once with bound 0 and once with the true bound: median
milliseconds of `reps` calls after one warm-up, then one timed call with opts.timing for the stage times.  Both legs must
give the same results.  One JSON line per (shape, bits); --c adds legs at fixed window sizes (planning errors show there).
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

STAGES = ("digits", "scan", "scatter", "plan", "accumulate", "reduce", "final", "total")


def load(path):
    """a second libmsmz.so in this process (the parent's), with the argument types of the calls used here"""
    from msm_zprize_amd import _native
    lib = C.CDLL(path)
    for name, (res, args) in _native.EXPORTS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


class Session:
    def __init__(self, lib):
        from msm_zprize_amd._native import check
        self.lib, self.check = lib, check
        self.ctx = C.c_void_p()
        dev = (C.c_int * 1)(0)
        check(lib.msmz_create(C.byref(self.ctx), 0, dev, 1), "msmz_create")

    def close(self):
        self.lib.msmz_destroy(self.ctx)

    def handle(self, fn, *args):
        h = C.c_uint64()
        self.check(getattr(self.lib, fn)(self.ctx, *args, C.byref(h)), fn)
        return h.value

    def msm(self, ph, sh, n, B, c, bits, timing=0):
        from msm_zprize_amd._native import MsmzLog, MsmzOpts
        o = MsmzOpts()
        o.c, o.glv, o.safe, o.timing = c, 0, 0, timing
        o.reserved[1] = bits
        out = C.create_string_buffer(96 * B)
        inf = (C.c_int * B)()
        log = MsmzLog()
        t0 = time.perf_counter()
        st = self.lib.msmz_msm_batch_resident(self.ctx, ph, sh, n, B, C.byref(o), out, inf, C.byref(log))
        ms = (time.perf_counter() - t0) * 1e3
        self.check(st, "msmz_msm_batch_resident")
        return ms, out.raw, log

    def timed(self, reps, *args):
        self.msm(*args)
        ts = []
        for _ in range(reps):
            ms, raw, log = self.msm(*args)
            ts.append(ms)
        _, _, tlog = self.msm(*args, timing=1)
        return statistics.median(ts), raw, log, {k: round(tlog.stage_ms[i], 3) for i, k in enumerate(STAGES)}


def short_scalars(n, bits, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 32), dtype=np.uint8)
    s[:, :bits // 8] = rng.integers(0, 256, size=(n, bits // 8), dtype=np.uint8)
    return s.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", action="append", default=None, help="B:LOG2N or B:LOG2N:pre")
    ap.add_argument("--bits", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--c", type=int, nargs="*", default=[], help="extra legs at these window sizes (plain sets)")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    shapes = [s.split(":") for s in a.shape] if a.shape else [["1", "16"], ["1", "20"], ["16", "16"], ["16", "16", "pre"]]
    from msm_zprize_amd import _native
    cur = Session(_native.lib())
    par = Session(load(a.parent_lib)) if a.parent_lib else None
    lines = []
    for sh in shapes:
        B, lg, pre = int(sh[0]), int(sh[1]), len(sh) > 2
        n = 1 << lg
        for bits in a.bits:
            host = short_scalars(B * n, bits, 1000 * lg + bits)
            rec = {"curve": "bls12-377", "B": B, "log2n": lg, "precomputed": pre, "scalar_bits": bits}
            legs = [("bound0", cur, 0, 0), ("bounded", cur, bits, 0)]
            legs += [(f"bounded_c{c}", cur, bits, c) for c in (a.c if not pre else [])]
            if par:
                legs.append(("parent", par, 0, 0))
            results = {}
            for name, s, bound, c in legs:
                pts = s.handle("msmz_random_points", n, 1)
                sc = s.handle("msmz_upload_scalars", host, B * n)
                ph = pts
                if pre:
                    from msm_zprize_amd._native import MsmzOpts
                    o = MsmzOpts()
                    o.glv = 0
                    o.reserved[1] = bound
                    ph = s.handle("msmz_precompute_points", pts, n, C.byref(o), 0)
                    rcount = C.c_uint64()
                    s.check(s.lib.msmz_precomputed_info(s.ctx, ph, None, None, None, None, C.byref(rcount)), "info")
                    rec[name + "_set_records"] = rcount.value
                ms, raw, log, stages = s.timed(a.reps, ph, sc, n, B, c, bound)
                results[name] = raw
                rec[name + "_ms"] = round(ms, 3)
                rec[name] = {"c": log.c, "K": log.K, "rounds": log.rounds, "n_entries": int(log.n_entries), "stage_ms": stages}
                for h in {ph, pts, sc}:
                    s.check(s.lib.msmz_free(s.ctx, h), "msmz_free")
            if len(set(results.values())) != 1:
                raise SystemExit(f"legs disagree at B = {B}, n = 2^{lg}, {bits}-bit scalars")
            rec["speedup"] = round(rec["bound0_ms"] / rec["bounded_ms"], 2)
            if par:
                rec["bound0_vs_parent"] = round(rec["bound0_ms"] / rec["parent_ms"], 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    cur.close()
    if par:
        par.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
