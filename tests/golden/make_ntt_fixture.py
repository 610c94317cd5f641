"""Writes the two fixtures of the transform's host bindings, from Python integers only.
tests/golden/ntt_js_fixture.json: the inputs of js/scripts/msm-ntt.mjs (64 scalars of BLS12-377 that hold 0, 1, q - 1
and the value with full low words; a vector of 2048 follows from them by a rule) and what a number-theoretic transform
over Python integers mod oracle.params' group order owes for them: sampled entries of a two-pass transform, a coset,
short inputs in a batch, the default roots.
tests/golden/ntt_args_parity.json: a table of calls of ntt_args (msm_zprize_amd/parallel.py) / nttArgs (js/parallel.mjs),
good and bad, with what each must give: the checked arguments, or the kind of error.  Run from the repository root:
    python tests/golden/make_ntt_fixture.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ntt_util as N           # noqa: E402
import scalar_ops_util as S    # noqa: E402

LABEL, LOG_N, SMALL = "bls12-377", 11, 6
SAMPLES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2046, 2047, 777]   # output indices of the long transform that are kept


def long_input(q, xs, n):
    """the 2^LOG_N entries of the two-pass transform, by a rule the script repeats: X_i = x[i mod 2^SMALL] (i + 1) mod q"""
    return [xs[i % len(xs)] * (i + 1) % q for i in range(n)]


def build():
    q = S.order(LABEL)
    n, m = 1 << LOG_N, 1 << SMALL
    xs = N.inputs(LABEL, m, 2029)
    g = random.Random(71).randrange(2, q)
    text = lambda vals: [str(v) for v in vals]
    w, ws = N.root(LABEL, LOG_N), N.root(LABEL, SMALL)
    short = []
    for k in range(2):
        short += N.transform(q, xs[16 * k:16 * k + 16], m, ws)
    forward = N.transform(q, long_input(q, xs, n), n, w)
    return {
        "curve": LABEL, "logN": LOG_N, "small": SMALL, "shift": str(g), "x": text(xs),
        "roots": text([N.root(LABEL, k) for k in (0, 1, SMALL, LOG_N, 31, 47)]), "rootLogs": [0, 1, SMALL, LOG_N, 31, 47],
        "samples": SAMPLES, "forward": text(forward[k] for k in SAMPLES),
        "coset": text(N.transform(q, xs, m, ws, shift=g)),
        "cosetInverse": text(N.transform(q, xs, m, ws, inverse=True, shift=g)),
        "short": text(short),
        "mirrored": text(N.transform(q, xs, m, pow(ws, -1, q))),
    }


# ------------------------------------------------------------------------------------------------ the argument table
Q = 1009   # the "group order" of the table: small, so out-of-range values are short
ARRAYS = {"x": (1, 4096, "scalars"), "y": (2, 5000, "scalars"), "x2": (1, 4096, "scalars"), "pts": (4, 100, "points"),
          "big": (5, (1 << 32) - 1, "scalars")}


def big(v):
    return {"big": str(v)}


def cases():
    """[label, {x, logN, inverse, shift, root, nIn, count, first, out, firstOut}]: arrays by name (ARRAYS), field elements
    as {"big": decimal}, everything else as it is; an absent key takes the default"""
    rows = [("ok plain", dict(x="x", logN=12)), ("ok all", dict(x="x", logN=10, inverse=True, shift=big(5), root=big(7), count=4)),
            ("ok short batch", dict(x="x", logN=10, nIn=100, count=40, first=96)), ("ok in place", dict(x="x", logN=11, out="x")),
            ("ok in place alias", dict(x="x", logN=11, out="x2")), ("ok apart", dict(x="x", logN=11, out="x", firstOut=2048)),
            ("ok short apart", dict(x="x", logN=11, nIn=1024, out="x", firstOut=1024)), ("ok other", dict(x="x", logN=12, out="y", firstOut=904)),
            ("ok n=1", dict(x="x", logN=0, count=4096)), ("ok 2^31", dict(x="big", logN=31)), ("ok shift q-1", dict(x="x", logN=3, shift=big(Q - 1)))]
    for name, v in (("points", "pts"), ("null", None), ("number", 7), ("string", "x!")):
        rows.append((f"x={name}", dict(x=v, logN=3)))
        if v is not None:
            rows.append((f"out={name}", dict(x="x", logN=3, out=v)))
    for key in ("shift", "root"):
        for name, v in (("float", 1.5), ("string", "1"), ("bool", True), ("q", big(Q)), ("neg", big(-1)), ("2^256", big(1 << 256))):
            rows.append((f"{key}={name}", dict(x="x", logN=3, **{key: v})))
    rows += [("shift=0", dict(x="x", logN=3, shift=big(0))), ("root=0", dict(x="x", logN=3, root=big(0))),
             ("inverse=1", dict(x="x", logN=3, inverse=1)), ("inverse=string", dict(x="x", logN=3, inverse="yes"))]
    for v in (-1, 32, True, 1.5, "3", None, 13):
        rows.append((f"logN={v!r}", dict(x="x", logN=v)))
    for v in (0, -1, True, 1.5, "1", 513):
        rows.append((f"count={v!r}", dict(x="x", logN=3, count=v)))
    rows += [("count*n=2^32", dict(x="big", logN=20, count=1 << 12)), ("count*n beyond", dict(x="x", logN=12, count=2))]
    for v in (0, 9, -1, 1.5, "4", True):
        rows.append((f"nIn={v!r}", dict(x="x", logN=3, nIn=v)))
    rows.append(("inverse short", dict(x="x", logN=3, nIn=4, inverse=True)))
    for key in ("first", "firstOut"):
        for v in (-1, 1.5, "1", True, None):
            rows.append((f"{key}={v!r}", dict(x="x", logN=3, out="y", **{key: v})))
    rows += [("first beyond", dict(x="x", logN=3, first=4089)), ("firstOut without", dict(x="x", logN=3, firstOut=1)),
             ("firstOut beyond", dict(x="x", logN=3, out="y", firstOut=4993)),
             ("overlap +1", dict(x="x", logN=11, out="x", firstOut=1)), ("overlap -1", dict(x="x", logN=11, first=1, out="x")),
             ("overlap end", dict(x="x", logN=11, out="x", firstOut=2047)), ("overlap short same start", dict(x="x", logN=11, nIn=1024, out="x")),
             ("overlap short inside", dict(x="x", logN=11, nIn=1024, first=5, out="x")),
             ("overlap alias", dict(x="x", logN=11, nIn=1024, out="x2", firstOut=1023)),
             ("double x+logN", dict(x=None, logN=99)), ("double shift+count", dict(x="x", logN=3, shift=big(0), count=0))]
    return rows


def run_python(row):
    """one row through ntt_args -> {"ok": the checked arguments} or {"err": "TypeError" | "ValueError"}"""
    from msm_zprize_amd.parallel import DeviceArray, ntt_args

    def arr(v):
        return DeviceArray(None, *ARRAYS[v][:2], ARRAYS[v][2]) if isinstance(v, str) and v in ARRAYS else v

    def num(v):
        return int(v["big"]) if isinstance(v, dict) else v

    a = dict(inverse=False, shift=None, root=None, nIn=None, count=1, first=0, out=None, firstOut=0)
    a.update(row)
    try:
        t = ntt_args(arr(a["x"]), a["logN"], a["inverse"], num(a["shift"]), num(a["root"]), a["nIn"], a["count"], a["first"],
                     arr(a["out"]), a["firstOut"], Q)
    except (TypeError, ValueError) as e:
        return {"err": type(e).__name__}
    for key in ("root", "shift"):
        t[key] = None if t[key] is None else str(int.from_bytes(t[key], "little"))
    return {"ok": t}


def build_args():
    return {"order": str(Q), "arrays": {k: list(v) for k, v in ARRAYS.items()},
            "cases": [[label, row, run_python(row)] for label, row in cases()]}


def dump(name, lines):
    """a JSON object, one key (or one table row) per line: a diff of it can be read"""
    with open(os.path.join(HERE, name), "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


def main():
    dump("ntt_js_fixture.json", [f"{json.dumps(k)}: {json.dumps(v)}" for k, v in build().items()])
    table = build_args()
    rows = ",\n".join(json.dumps(c) for c in table["cases"])
    dump("ntt_args_parity.json", [f'"order": {json.dumps(table["order"])}', f'"arrays": {json.dumps(table["arrays"])}',
                                  f'"cases": [\n{rows}\n]'])


if __name__ == "__main__":
    main()
