#!/usr/bin/env python3
"""What msmz_scalars_expr costs, beside the chain of combineScalars calls that produces the same bytes without it and
beside a device-to-device copy of the least bytes the call can move.  BLS12-377 and Pallas, ONE process.

    python tools/expr_report.py [--out FILE] [--reps R] [--logn 16 20 24] [--curves LABEL ...] [--gates G1 G2 G3 G4]
                                [--legs fused chain copy] [--variant NAME]

Four gates over columns of random scalars made on the device:
    G1  the PLONK arithmetic gate q_L a + q_R b + q_M a b + q_O c + q_C: 8 columns, 5 terms, degree 3
    G2  one wire of the permutation step, Z(wX)(w + beta sigma + gamma) - Z(X)(w + beta id + gamma), as a sum of
        products: 6 terms, one rotated operand
    G3  a^5 + c b - a[+1]: a repeated factor
    G4  32 terms of degree 8 over 16 columns
and two more that are not run unless --gates names them, for the A/B of the register-resident kernel: few operands and no
repeated factor, where loading every operand once saves nothing
    X1  c_x x + c_y y: 2 operands
    X2  a b + c d: 4 operands
Legs, alternating call by call inside one loop after two warm-up calls of each, every one into buffers made beforehand:
    fused   evaluateExpression(columns, terms, out=dst)
    chain   what a caller does without it: combineScalars calls -- a product of k columns in k - 1 passes (k with a
            coefficient other than 1), each term added by the pass that ends it, a rotated operand copied into place
            first by two calls (body and wrap), a constant added as c times a vector of ones the caller keeps
    copy    a device-to-device copy that moves (distinct operands + 1) 32 n bytes in all, read plus written: the byte
            floor of the fused call as this process measures it
A call is timed by the host clock around the whole call, which ends behind its host wait.  Reported per leg: median,
fastest and slowest of `reps` calls.  products = the field products of the fused call (the factors of all terms, n
times); products_per_s is that over the fused median.  Before timing, the chain's result is compared with the fused one
through innerProduct of both and, up to 2^16 entries, byte for byte.  --variant tags the lines (another build of the
library, named by MSMZ_LIB, measured beside the default one).  One JSON line per leg, to stdout and appended to --out (default
profiles/expr_report.jsonl).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gates(q, rng):
    import expr_util as E
    return {"G1": (8, E.plonk_gate()), "G2": (4, E.permutation_wire(rng.randrange(q), rng.randrange(q), q)),
            "G3": (2, E.sbox_gate(rng.randrange(q), q)), "G4": (16, E.stress_gate(q, rng)),
            "X1": (2, [(rng.randrange(q), [0]), (rng.randrange(q), [1])]), "X2": (4, [(None, [0, 1]), (None, [2, 3])])}


def chain(par, cols, terms, n, acc, tmp, rotated, ones):
    """the combineScalars route to the bytes of evaluateExpression(cols, terms, out=acc); -> the number of calls"""
    import expr_util as E
    calls = 0
    for (col, rot), buf in rotated.items():         # rotated copy: body, then wrap
        par.combineScalars(1, cols[col], N=n - rot, firstX=rot, out=buf)
        par.combineScalars(1, cols[col], N=rot, out=buf, firstOut=n - rot)
        calls += 2
    first = True
    for c, fs in terms:
        c = 1 if c is None else c
        ops = [cols[col] if rot % n == 0 else rotated[(col, rot % n)] for col, rot in map(E.factor, fs)] or [ones]
        if len(ops) == 1:
            co = c
        elif c == 1:
            co, ops = ops[0], ops[1:]
        else:
            par.combineScalars(c, ops[0], out=tmp)
            calls += 1
            co, ops = tmp, ops[1:]
        for f in ops[:-1]:
            par.combineScalars(co, f, out=tmp)
            calls += 1
            co = tmp
        if first:
            par.combineScalars(co, ops[-1], out=acc)
        else:
            par.combineScalars(1, acc, co, ops[-1], out=acc)
        calls += 1
        first = False
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expr_report.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--curves", nargs="+", default=["bls12-377", "pallas"])
    ap.add_argument("--gates", nargs="+", default=["G1", "G2", "G3", "G4"])
    ap.add_argument("--legs", nargs="+", default=["fused", "chain", "copy"])
    ap.add_argument("--variant", default="default")
    args = ap.parse_args()
    import torch
    import expr_util as E
    import msm_zprize_amd as m
    from msm_zprize_amd._native import lib
    import ctypes as C
    m.startThreads()
    threads, slots = C.c_uint32(0), C.c_uint32(0)
    lib().msmz_test_expr_geometry(C.byref(threads), C.byref(slots))
    lines = []

    def clock(call):
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    for params in m.curves.ALL_CURVES:
        if params["label"] not in args.curves:
            continue
        q = params["order"]
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        par = curve.Parallel
        for logn in args.logn:
            n = 1 << logn
            pool = [par.randomScalars(n, 100 + k) for k in range(16)]
            ones = par.scalarPowers(1, n)
            acc, tmp, dst = (par.randomScalars(n, 7) for _ in range(3))
            for name, (nc, terms) in gates(q, random.Random(5)).items():
                if name not in args.gates:
                    continue
                cols = pool[:nc]
                ops = E.operands(terms, n)
                rotated = {op: par.randomScalars(n, 9) for op in ops if op[1]}
                products = n * sum(len(fs) for _, fs in terms)
                floor_bytes = (len(ops) + 1) * 32 * n
                src_t = torch.empty(floor_bytes // 2, dtype=torch.uint8, device="cuda")
                dst_t = torch.empty_like(src_t)

                def copy():
                    dst_t.copy_(src_t)
                    torch.cuda.synchronize()

                legs = {"fused": lambda: par.evaluateExpression(cols, terms, out=dst),
                        "chain": lambda: chain(par, cols, terms, n, acc, tmp, rotated, ones),
                        "copy": copy}
                legs = [(leg, legs[leg]) for leg in args.legs]
                calls = None
                if "fused" in args.legs and "chain" in args.legs:
                    par.evaluateExpression(cols, terms, out=dst)
                    calls = chain(par, cols, terms, n, acc, tmp, rotated, ones)
                    assert par.innerProduct(dst) == par.innerProduct(acc) and par.innerProduct(dst, dst) == par.innerProduct(acc, acc)
                    if logn <= 16:
                        assert curve.Scalar.toBigints(dst) == curve.Scalar.toBigints(acc)
                for _, call in legs:
                    call()
                    call()
                times = {leg: [] for leg, _ in legs}
                for _ in range(args.reps):
                    for leg, call in legs:
                        times[leg].append(clock(call))
                for leg, _ in legs:
                    ms = statistics.median(times[leg])
                    row = {"curve": params["label"], "log2n": logn, "gate": name, "leg": leg, "variant": args.variant,
                           "register_slots": slots.value, "ms": round(ms, 4), "ms_min": round(min(times[leg]), 4),
                           "ms_max": round(max(times[leg]), 4), "reps": args.reps, "terms": len(terms), "operands": len(ops),
                           "floor_bytes": floor_bytes}
                    if leg == "fused":
                        row.update(products=products, products_per_s=round(products / (ms * 1e-3), 0),
                                   gb_per_s=round(floor_bytes / (ms * 1e-3) / 1e9, 1))
                    if leg == "chain":
                        row["calls"] = calls
                    if leg == "copy":
                        row["gb_per_s"] = round(floor_bytes / (ms * 1e-3) / 1e9, 1)
                    lines.append(row)
                    print(json.dumps(row), flush=True)
                del src_t, dst_t
                for buf in rotated.values():
                    buf.free()
            for a in pool + [ones, acc, tmp, dst]:
                a.free()
        curve.close()
    with open(args.out, "a") as fh:
        for row in lines:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
