#!/usr/bin/env python3
"""Imports: what it costs to get scalars to the engine from where the caller has them.  BLS12-377 G1, no GLV, unsafe
additions, resident points, all in ONE process (boxes differ by ~2 %).

    python tools/scalar_import_report.py [--out FILE] [--reps R] [--shape B:LOG2N ...] [--parent-lib variants/libmsmz_parent.so]

For every shape (default 2^16, 2^20, 16 x 2^16) and scalars uniform below 2^64 ("64") and below q ("full") every leg is
timed from "the scalars sit where the caller has them" to "the result is on the host": median milliseconds of `reps`
calls after one warm-up.  64-bit scalars run with scalarBits = 64 in every leg.  All legs must give the same results.
  host32     host buffer, 32-byte canonical, msmz_msm_batch (the route from before; --parent-lib: also on that library)
  host8      host buffer, 8-byte records: import + resident MSM + free            (64-bit scalars only)
  dev32/dev8 device tensor, 32- / 8-byte records: import + resident MSM + free
  devmont    device tensor, 32-byte Montgomery records: import + resident MSM + free
  resident   the scalars already are a handle (the floor)
and *_import_ms: the import call alone.  One JSON line per (shape, bits).
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

    def opts(self, bits):
        from msm_zprize_amd._native import MsmzOpts
        o = MsmzOpts()
        o.glv, o.safe = 0, 0
        o.reserved[1] = bits
        return o

    def msm_host(self, ph, host, n, B, bits):
        out, inf, o = C.create_string_buffer(96 * B), (C.c_int * B)(), self.opts(bits)
        self.check(self.lib.msmz_msm_batch(self.ctx, ph, host, n, B, C.byref(o), out, inf, None), "msmz_msm_batch")
        return out.raw

    def msm_resident(self, ph, sh, n, B, bits):
        out, inf, o = C.create_string_buffer(96 * B), (C.c_int * B)(), self.opts(bits)
        self.check(self.lib.msmz_msm_batch_resident(self.ctx, ph, sh, n, B, C.byref(o), out, inf, None), "msmz_msm_batch_resident")
        return out.raw

    def imported(self, ph, src, n, B, bits, import_ts):
        t0 = time.perf_counter()
        sh = self.handle("msmz_import_scalars", C.byref(src), B * n)
        import_ts.append((time.perf_counter() - t0) * 1e3)
        raw = self.msm_resident(ph, sh, n, B, bits)
        self.check(self.lib.msmz_free(self.ctx, sh), "msmz_free")
        return raw


def timed(reps, fn):
    raw = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        raw = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shape", action="append", default=None, help="B:LOG2N")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    shapes = [s.split(":") for s in a.shape] if a.shape else [["1", "16"], ["1", "20"], ["16", "16"]]
    import numpy as np
    import torch
    from msm_zprize_amd import _native, curves
    from msm_zprize_amd._native import MSMZ_SRC_DEFAULT_STREAM, MSMZ_SRC_DEVICE, MSMZ_SRC_MONTGOMERY, MsmzSrc
    q = curves.bls12377Params["order"]
    cur = Session(_native.lib())
    par = Session(load(a.parent_lib)) if a.parent_lib else None
    lines = []
    for sh in shapes:
        B, lg = int(sh[0]), int(sh[1])
        n = 1 << lg
        total = B * n
        for label in ("64", "full"):
            rng = np.random.default_rng(1000 * lg + B + len(label))
            s = np.zeros((total, 32), dtype=np.uint8)
            if label == "64":
                s[:, :8] = rng.integers(0, 256, size=(total, 8), dtype=np.uint8)
                bits = 64
            else:
                s[:, :31] = rng.integers(0, 256, size=(total, 31), dtype=np.uint8)   # below 2^248 < q
                bits = 0
            host32 = s.tobytes()
            vals = [int.from_bytes(host32[32 * i:32 * i + 32], "little") for i in range(total)]
            mont = b"".join(((v << 256) % q).to_bytes(32, "little") for v in vals)
            rec = {"curve": "bls12-377", "B": B, "log2n": lg, "scalars": label, "reps": a.reps}
            results = {}
            pts = cur.handle("msmz_random_points", n, 1)
            d32 = torch.frombuffer(bytearray(host32), dtype=torch.uint8).cuda()
            dmont = torch.frombuffer(bytearray(mont), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            dflags = MSMZ_SRC_DEVICE | MSMZ_SRC_DEFAULT_STREAM
            srcs = {"dev32": MsmzSrc(d32.data_ptr(), 0, 32, dflags, None, None),
                    "devmont": MsmzSrc(dmont.data_ptr(), 0, 32, dflags | MSMZ_SRC_MONTGOMERY, None, None)}
            keep = [d32, dmont]
            if label == "64":
                host8 = np.ascontiguousarray(s[:, :8]).tobytes()
                d8 = torch.frombuffer(bytearray(host8), dtype=torch.uint8).cuda()
                torch.cuda.synchronize()
                keep += [d8, host8]
                srcs["host8"] = MsmzSrc(C.cast(C.c_char_p(host8), C.c_void_p), 0, 8, 0, None, None)
                srcs["dev8"] = MsmzSrc(d8.data_ptr(), 0, 8, dflags, None, None)
            rec["host32_ms"], results["host32"] = timed(a.reps, lambda: cur.msm_host(pts, host32, n, B, bits))
            for name, src in srcs.items():
                its = []
                rec[name + "_ms"], results[name] = timed(a.reps, lambda: cur.imported(pts, src, n, B, bits, its))
                rec[name + "_import_ms"] = round(statistics.median(its[1:]), 4)
            sh_res = cur.handle("msmz_upload_scalars", host32, total)
            rec["resident_ms"], results["resident"] = timed(a.reps, lambda: cur.msm_resident(pts, sh_res, n, B, bits))
            for h in (pts, sh_res):
                cur.check(cur.lib.msmz_free(cur.ctx, h), "msmz_free")
            if par:
                ppts = par.handle("msmz_random_points", n, 1)
                rec["parent_host32_ms"], results["parent"] = timed(a.reps, lambda: par.msm_host(ppts, host32, n, B, bits))
                par.check(par.lib.msmz_free(par.ctx, ppts), "msmz_free")
                # once more on this library, after the parent's: the order of the legs must not decide the ratio
                pts2 = cur.handle("msmz_random_points", n, 1)
                again, _ = timed(a.reps, lambda: cur.msm_host(pts2, host32, n, B, bits))
                cur.check(cur.lib.msmz_free(cur.ctx, pts2), "msmz_free")
                rec["host32_again_ms"] = round(again, 3)
                rec["host32_vs_parent"] = round(min(rec["host32_ms"], again) / rec["parent_host32_ms"], 3)
            if len(set(results.values())) != 1:
                raise SystemExit(f"legs disagree at B = {B}, n = 2^{lg}, {label} scalars: "
                                 f"{[k for k, v in results.items() if v != results['host32']]}")
            for k in list(rec):
                if k.endswith("_ms"):
                    rec[k] = round(rec[k], 4)
            for name in srcs:
                rec[name + "_minus_resident_ms"] = round(rec[name + "_ms"] - rec["resident_ms"], 4)
                w = srcs[name].width
                rec[name + "_import_GBps"] = round(total * (w + 32) / (rec[name + "_import_ms"] * 1e-3) / 1e9, 1)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del keep
    cur.close()
    if par:
        par.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
