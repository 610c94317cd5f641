"""Level times of the bucket reduction's upper levels, row form against the 4-lane and the per-lane forms.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/reduce_rows_levels.py run
  python tools/reduce_rows_levels.py table DIR/*/*kernel_trace.csv

`run` drives BucketReduce::levels through msmz_test_reduce (BLS12-377): 30 problems of 1024 entries, whose levels have
7680, 1920, 480, 120 and 30 groups, once with every level on k_reduce_rows, once on k_reduce_quad16, once on
k_reduce_quad; then the last levels of the flagship shape (30 problems of 16 entries) in k_reduce_tail.  Each call is
repeated; `table` prints the median duration of every (kernel, grid) pair of the trace."""
import ctypes as C
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 5


def run():
    import numpy as np
    import msm_zprize_amd as m
    from msm_zprize_amd import _native
    m.startThreads()
    curve = m.Weierstrass.create(m.curves.bls12377Params)
    fb = curve.fe_bytes
    from oracle import bigint_ref as BR
    from oracle import params as P
    A = BR.AffineWeierstrass(P.BLS12_377)
    g, acc = [], A.one
    for _ in range(64):                                        # G, 2G, ..., 64G
        g.append(acc)
        acc = A.add(acc, A.one)
    rec = np.frombuffer(b"".join(q[0].to_bytes(fb, "little") + q[1].to_bytes(fb, "little") for q in g), dtype=np.uint8)
    rec = rec.reshape(64, 2 * fb)

    def levels(nprob, n_in, tail_n, quad16_max, rows_max):
        n = 2 * nprob * n_in
        pts = np.ascontiguousarray(rec[np.arange(n) % 61])   # 61 distinct points: no equal neighbours
        a = _native.MsmzTestReduceArgs()
        a.mode, a.nsets, a.n_in, a.n_points = 3, nprob, n_in, n
        a.tail_n, a.quad16_max, a.rows_max = tail_n, quad16_max, rows_max
        a.points_xy = pts.tobytes()
        out = np.zeros((nprob, 2 * fb), dtype=np.uint8)
        a.out_xy = out.ctypes.data
        st = _native.lib().msmz_test_reduce(curve._ctx, C.byref(a))
        assert st == 0, st
        return out.tobytes()

    for _ in range(REPS):
        ref = levels(30, 1024, 1, 1 << 20, 1 << 20)            # every level: k_reduce_rows
        assert levels(30, 1024, 1, 1 << 20, 1) == ref          # k_reduce_quad16 (the single-group tail aside)
        assert levels(30, 1024, 1, 1, 1) == ref                # k_reduce_quad
        t = levels(30, 16, 4096, 0, 1 << 20)                   # k_reduce_rows on 120 and 30 groups, the tail copies
        assert levels(30, 16, 4096, 0, 1) == t                 # k_reduce_tail does both levels
    curve.close()
    print("ok")


def table(path):
    rows = list(csv.DictReader(open(path)))
    per = {}
    for r in rows:
        name = r["Kernel_Name"]
        if "k_reduce" not in name:
            continue
        name = name.split("<")[0].split("::")[-1].split(" ")[-1]
        wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 0)
        grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
        per.setdefault((name, grid // max(wg, 1), wg), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':22s} {'workgroups':>10s} {'threads':>8s} {'launches':>8s} {'median us':>10s} {'min us':>8s}")
    for (name, wgs, wg), d in sorted(per.items()):
        print(f"{name:22s} {wgs:10d} {wg:8d} {len(d):8d} {statistics.median(d):10.1f} {min(d):8.1f}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    else:
        raise SystemExit(__doc__)
