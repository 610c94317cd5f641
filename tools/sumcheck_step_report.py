#!/usr/bin/env python3
"""What msmz_scalars_sumcheck_step buys: whole sumcheck protocols and single steps, the step route beside the two-call
route (sumcheckRound, then bindMle of every table) in ONE process on the same build, with the same challenges.

    python tools/sumcheck_step_report.py [--out FILE] [--reps R] [--vars 12 16 20 24] [--step-vars 20 24]

Shapes (those of tools/mle_report.py): "2x1" two tables, one term f g; "4x2" four tables, eq A B - eq C.  BLS12-377 at
every size, BLS12-381 in one row (4x2 at v = 20).  Both routes bind in place in the high order, so neither allocates:
    protocol, step route      sumcheckProve: one sumcheckRound, then v sumcheckStep
    protocol, two-call route  v times (sumcheckRound, bindMle of every table with out = the table), then the claim on the
                              host from the one entry left of every table
    single step               sumcheckStep into other arrays | bindMle of every table into those arrays + sumcheckRound
A challenge is a fixed function of the round's values, the same on both routes, and both routes are checked to return the
same polynomials and claim before anything is timed.  The tables are generated on the device afresh before every timed
protocol, outside the timed region.  The two sides ALTERNATE, call by call, after two warm-ups of each; a leg is timed by
the host clock around the whole route.  Per leg: median, fastest and slowest of `reps` runs.  bytes (single steps only):
what the route must read and write, 32 per record -- 1.5 N T for the step, 2 N T for bind + round.  One JSON line per
leg, to stdout and appended to --out (default profiles/sumcheck_step_report.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GB_S = 6290.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumcheck_step_report.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--vars", type=int, nargs="+", default=[12, 16, 20, 24])
    ap.add_argument("--step-vars", type=int, nargs="+", default=[20, 24])
    args = ap.parse_args()
    import msm_zprize_amd as m
    m.startThreads()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def compare(legs, setup):
        """legs: [(name, run(state))], setup() -> (state, arrays to free) before every run, untimed -> {name: [ms, ...]}"""
        def once(run):
            state, mine = setup()
            t0 = time.perf_counter()
            run(state)
            ms = (time.perf_counter() - t0) * 1e3
            for a in mine:
                a.free()
            return ms
        for _, run in legs:
            once(run), once(run)
        times = {name: [] for name, _ in legs}
        for _ in range(args.reps):
            for name, run in legs:
                times[name].append(once(run))
        return times

    def stats(ts):
        return {"ms": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "reps": len(ts)}

    for label, sizes, step_sizes, shapes in (("bls12-377", args.vars, args.step_vars, ("2x1", "4x2")), ("bls12-381", [20], [], ("4x2",))):
        params = m.curves.BY_LABEL[label]
        curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        q, par = params["order"], curve.Parallel

        def challenge(values):
            return (sum(values) * 0x9E3779B97F4A7C15 + 0x1234567) % q

        def terms_of(shape):
            return [(None, 0b11)] if shape == "2x1" else [(1, 0b0111), (q - 1, 0b1001)]

        def claim_of(tables, terms):
            ones = [curve.Scalar.toBigints(f, 0, 1)[0] for f in tables]
            total = 0
            for c, mask in terms:
                p = 1 if c is None else c
                for j, x in enumerate(ones):
                    if (mask >> j) & 1:
                        p = p * x % q
                total += p
            return total % q

        for shape in shapes:
            nt, terms = int(shape[0]), terms_of(shape)
            for v in sizes:
                n = 1 << v

                def fresh():
                    tables = [par.randomScalars(n, 40 + k) for k in range(nt)]
                    return tables, tables

                def step_route(tables):
                    return par.sumcheckProve(tables, terms, v, challenge)

                def two_call_route(tables):
                    polys, rs = [], []
                    for k in range(v):
                        polys.append(par.sumcheckRound(tables, terms, v - k))
                        rs.append(challenge(polys[-1]))
                        for f in tables:
                            par.bindMle(f, rs[-1], v - k, out=f)
                    return polys, rs, claim_of(tables, terms)

                both = []
                for route in (step_route, two_call_route):
                    tables, mine = fresh()
                    both.append(route(tables))
                    for a in mine:
                        a.free()
                assert both[0] == both[1], "the two routes disagree"
                times = compare([("protocol, step route", step_route), ("protocol, two-call route", two_call_route)], fresh)
                for name, ts in times.items():
                    emit({"curve": label, "log2n": v, "shape": shape, "leg": name, **stats(ts),
                          "calls": 1 + v if "step" in name else v * (1 + nt) + nt})
            for v in step_sizes:
                n, h = 1 << v, 1 << (v - 1)
                tables = [par.randomScalars(n, 40 + k) for k in range(nt)]
                outs = [par.randomScalars(h, 50 + k) for k in range(nt)]
                r = q * 5 // 7

                def one_step(_):
                    return par.sumcheckStep(tables, terms, v, r, out=outs)

                def bind_then_round(_):
                    for f, o in zip(tables, outs):
                        par.bindMle(f, r, v, out=o)
                    return par.sumcheckRound(outs, terms, v - 1)

                assert one_step(None)[1] == bind_then_round(None)
                times = compare([("sumcheckStep", one_step), ("bindMle per table + sumcheckRound", bind_then_round)], lambda: (None, ()))
                for name, ts in times.items():
                    nbytes = (3 * h if name == "sumcheckStep" else 4 * h) * nt * 32
                    s = stats(ts)
                    emit({"curve": label, "log2n": v, "shape": shape, "leg": name, **s, "bytes": nbytes,
                          "gb_per_s": round(nbytes / (s["ms"] * 1e-3) / 1e9, 1),
                          "hbm_fraction": round(nbytes / (s["ms"] * 1e-3) / 1e9 / HBM_GB_S, 3)})
                for a in tables + outs:
                    a.free()
        curve.close()
    with open(args.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
