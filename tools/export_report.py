#!/usr/bin/env python3
"""Exports: what it costs to get resident scalars and points into device memory of the caller, in the form it wants.
All in ONE process on one GPU (boxes differ by ~2 %).

    python tools/export_report.py [--out profiles/export_report.jsonl] [--reps 5] [--scalars 16,20,24] [--points 20,22]

For BLS12-377 and Pallas scalars (default 2^16, 2^20, 2^24: canonical 32 bytes, width 8, Montgomery) and points
(default 2^20, 2^22: canonical, Montgomery, compressed) every leg is a whole call, from "the set is resident" to "the
bytes are in device memory and the GPU is idle": the median milliseconds of `reps` calls after one warm-up, with the
fastest and the slowest of them beside it.
  export       msmz_export_* into a packed device tensor (16-byte aligned: the kernel's 16-byte stores)
  export_word  the same call into the same tensor 4 bytes further on: pointer, stride and width are no longer all
               multiples of 16, so the kernel takes its word stores -- the A/B of the store width, same bytes
  clone        (a) the floor: a device-to-device copy of the same output bytes (torch.Tensor.clone)
  download     (b) the route without exports: msmz_download_* into host memory, then torch.frombuffer(...).cuda();
               canonical and compressed forms only (there is no Montgomery download)
The two export legs must write the same bytes, and for the canonical forms the bytes of the download.  One JSON line per
(kind, curve, size, form).
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


def timed(reps, fn, sync):
    """median, min, max milliseconds of `reps` calls of fn after one warm-up; `sync` drains the GPU around each"""
    fn()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scalars", default="16,20,24")
    ap.add_argument("--points", default="20,22")
    a = ap.parse_args()
    import torch   # (before the library: one HIP runtime per process)
    import msm_zprize_amd as m
    from msm_zprize_amd._native import (MSMZ_SRC_COMPRESSED, MSMZ_SRC_DEFAULT_STREAM, MSMZ_SRC_DEVICE, MSMZ_SRC_MONTGOMERY,
                                        MsmzDst, check, lib)
    if not torch.cuda.is_available():
        raise SystemExit("export_report: no GPU (nothing here is measured without one)")
    m.startThreads(device=0)
    L = lib()
    sync = torch.cuda.synchronize
    dflags = MSMZ_SRC_DEVICE | MSMZ_SRC_DEFAULT_STREAM
    lines = []

    def legs(rec, fn_name, ctx, handle, n, width, flags, download):
        """the four legs of one (set, form) into rec; download: () -> host bytes, or None"""
        room = torch.zeros(n * width + 16, dtype=torch.uint8, device="cuda")
        outs = {}
        for leg, off in (("export", 0), ("export_word", 4)):
            out = room[off:off + n * width]
            assert out.data_ptr() % 16 == off
            dst = MsmzDst(out.data_ptr(), 0, width, flags | dflags, None, None)
            t = timed(a.reps, lambda: check(getattr(L, fn_name)(ctx, handle, 0, n, C.byref(dst)), fn_name), sync)
            rec.update({leg + "_" + k: v for k, v in t.items()})
            outs[leg] = out.clone()
        if not torch.equal(outs["export"], outs["export_word"]):
            raise SystemExit(f"the two store widths disagree: {rec}")
        keep = []
        rec.update({"clone_" + k: v for k, v in timed(a.reps, lambda: keep.append(outs["export"].clone()) or keep.pop(), sync).items()})
        if download:
            def route():
                keep.append(torch.frombuffer(download(), dtype=torch.uint8).cuda())
                return keep.pop()
            rec.update({"download_" + k: v for k, v in timed(a.reps, route, sync).items()})
            if not torch.equal(route(), outs["export"]):
                raise SystemExit(f"export and download disagree: {rec}")
            rec["export_vs_download"] = round(rec["export_ms"] / rec["download_ms"], 4)
        rec["bytes_out"] = n * width
        rec["export_vs_clone"] = round(rec["export_ms"] / rec["clone_ms"], 2)
        rec["word_vs_vec16"] = round(rec["export_word_ms"] / rec["export_ms"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for label, params, make in (("bls12-377", m.curves.bls12377Params, m.Weierstrass), ("pallas", m.curves.pallasParams, m.Weierstrass)):
        curve = make.create(params)
        ctx, fb = curve._ctx, curve.fe_bytes
        for lg in [int(x) for x in a.scalars.split(",") if x]:
            n = 1 << lg
            full = curve.Parallel.randomScalars(n, 1000 + lg)
            narrow = curve.Parallel.scalarsFromTensor(torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, device="cuda"))

            def dl_scalars():
                buf = bytearray(32 * n)
                check(L.msmz_download_scalars(ctx, full.handle, 0, n, (C.c_char * len(buf)).from_buffer(buf)), "msmz_download_scalars")
                return buf
            for form, arr, width, flags, dl in (("canonical32", full, 32, 0, dl_scalars), ("width8", narrow, 8, 0, None),
                                                ("montgomery", full, 32, MSMZ_SRC_MONTGOMERY, None)):
                legs({"kind": "scalars", "curve": label, "log2n": lg, "form": form, "reps": a.reps}, "msmz_export_scalars", ctx,
                     arr.handle, n, width, flags, dl)
            full.free()
            narrow.free()
        for lg in [int(x) for x in a.points.split(",") if x]:
            n = 1 << lg
            pts = curve.Parallel.randomPointsFast(n, 2000 + lg)

            def dl_points():
                buf = bytearray(2 * fb * n)
                check(L.msmz_download_points(ctx, pts.handle, 0, n, (C.c_char * len(buf)).from_buffer(buf), None), "msmz_download_points")
                return buf

            def dl_compressed():
                buf = bytearray(fb * n)
                check(L.msmz_download_points_compressed(ctx, pts.handle, 0, n, (C.c_char * len(buf)).from_buffer(buf), None, 0),
                      "msmz_download_points_compressed")
                return buf
            for form, width, flags, dl in (("canonical", 2 * fb, 0, dl_points), ("montgomery", 2 * fb, MSMZ_SRC_MONTGOMERY, None),
                                           ("compressed", fb, MSMZ_SRC_COMPRESSED, dl_compressed)):
                legs({"kind": "points", "curve": label, "log2n": lg, "form": form, "reps": a.reps}, "msmz_export_points", ctx,
                     pts.handle, n, width, flags, dl)
            pts.free()
        curve.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
