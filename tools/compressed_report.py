#!/usr/bin/env python3
"""What compressed point sets cost.  All four curves, generated resident sets, ONE process.

    python tools/compressed_report.py [--out FILE] [--reps R] [--logn 16 20 22] [--curves LABEL ...]

For every curve and size, medians of `reps` whole calls (wall clock around the C ABI call, after one warm-up), each leg
beside its comparison in the same run:
  import_host      msmz_import_points of compressed records in host memory   | the same points as x || y from host memory
  import_device    ... of compressed records in device memory (a torch tensor) | the same points as x || y from device memory
  download         msmz_download_points_compressed                            | msmz_download_points
The uncompressed import is the path that existed before compressed records did.  Beside the device import: the field
products of its arithmetic (F::SQRT_PRODUCTS of the square root plus the products of decompress around it, squarings
counted as products; the inversion of the twisted-Edwards denominator is not counted) and the fraction of the measured
fe_mul rate of profiles/r01_ubench_fp_modmul.txt (14 x 28-bit limbs: 72 G/s BLS12-377, 67 G/s BLS12-381; 9 x 29-bit
limbs: 165 G/s) that rate is.  One JSON line per (curve, size), to stdout and appended to --out (default
profiles/compressed_report.jsonl).
"""
import torch  # noqa: F401  (before libmsmz.so: one HIP runtime per process)

import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GMODMUL = {"bls12-377": 72.0, "bls12-381": 67.0, "pallas": 165.0, "ed-on-bls12-377": 165.0}
TAG = {"bls12-377": "Bls377Fp", "pallas": "PallasFp", "bls12-381": "Bls381Fp", "ed-on-bls12-377": "Ed377Fp"}


def products(params):
    """field products per decompressed point: to Montgomery form, the right-hand side, fe_sqrt, the sign of the root, and
    what store_resident adds (the endomorphism image / the Niels form)"""
    text = open(os.path.join(ROOT, "msm_zprize_amd", "csrc", "constants_gen.h")).read()
    body = text[text.index("struct %s {" % TAG[params["label"]]):]
    root = int(re.search(r"SQRT_PRODUCTS = (\d+);", body).group(1))
    around = 1 + 2 + 1 + 1 if params["kind"] == "weierstrass" else 1 + 3 + 1 + 2
    return root + around


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compressed_report.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--curves", nargs="+", default=None)
    args = ap.parse_args()
    import msm_zprize_amd as m
    from msm_zprize_amd._native import MSMZ_SRC_COMPRESSED, MSMZ_SRC_DEVICE, MsmzSrc, check, lib
    m.startThreads()
    L = lib()
    rows = []
    for params in m.curves.ALL_CURVES:
        if args.curves and params["label"] not in args.curves:
            continue
        fb = params["fe_bytes"]
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        for logn in args.logn:
            n = 1 << logn
            pts = curve.Parallel.randomPointsFast(n, 11)
            rec, xy, inf = C.create_string_buffer(fb * n), C.create_string_buffer(2 * fb * n), C.create_string_buffer(n)
            dl_c = lambda: check(L.msmz_download_points_compressed(curve._ctx, pts.handle, 0, n, rec, inf, 0), "download_compressed")
            dl_u = lambda: check(L.msmz_download_points(curve._ctx, pts.handle, 0, n, xy, inf), "download")
            t_dl_c, t_dl_u = median_ms(dl_c, args.reps), median_ms(dl_u, args.reps)
            d_rec = torch.frombuffer(bytearray(rec.raw), dtype=torch.uint8).cuda()
            d_xy = torch.frombuffer(bytearray(xy.raw), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()

            def imp(ptr, width, flags):
                def call():
                    src = MsmzSrc(ptr, 0, width, flags, None, None)
                    h = C.c_uint64(0)
                    check(L.msmz_import_points(curve._ctx, C.byref(src), n, C.byref(h)), "import")
                    check(L.msmz_free(curve._ctx, h.value), "free")
                return call

            t_h_c = median_ms(imp(C.cast(rec, C.c_void_p), fb, MSMZ_SRC_COMPRESSED), args.reps)
            t_h_u = median_ms(imp(C.cast(xy, C.c_void_p), 2 * fb, 0), args.reps)
            t_d_c = median_ms(imp(d_rec.data_ptr(), fb, MSMZ_SRC_COMPRESSED | MSMZ_SRC_DEVICE), args.reps)
            t_d_u = median_ms(imp(d_xy.data_ptr(), 2 * fb, MSMZ_SRC_DEVICE), args.reps)
            prod = products(params)
            rate = n * prod / (t_d_c * 1e-3) / 1e9
            row = {"curve": params["label"], "logn": logn, "reps": args.reps,
                   "import_host_ms": {"compressed": round(t_h_c, 3), "uncompressed": round(t_h_u, 3)},
                   "import_device_ms": {"compressed": round(t_d_c, 3), "uncompressed": round(t_d_u, 3)},
                   "download_ms": {"compressed": round(t_dl_c, 3), "uncompressed": round(t_dl_u, 3)},
                   "products_per_point": prod, "gproducts_per_s": round(rate, 2),
                   "fe_mul_peak_gps": PEAK_GMODMUL[params["label"]], "of_peak": round(rate / PEAK_GMODMUL[params["label"]], 3)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            pts.free()
            del d_rec, d_xy
        curve.close()
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
