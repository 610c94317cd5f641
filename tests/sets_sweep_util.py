"""The sweep of the resident-set operations (tests/test_sets_sweep_cpu.py, tests/test_sets_sweep_gpu.py): seeded PROGRAMS
of calls on one context -- one call writes a set, the next reads a range of it at an offset, a third overwrites part of it
in place, handles are freed and their size is allocated again -- each held, step by step, against a MODEL in Python
integers.  The layout is that of tests/msm_sweep_util.py: dimensions, a rule table, a greedy covering, directed cases, and
`cases(seed)`.

The model is a dict from a test-side set name to a list of ints (a matrix: its triples); one function per operation
updates it and returns the call's scalar results, each through the reference its family's tests already use
(scalar_scan_util, ntt_util, mle_util, sumcheck_step_util, matrix_util, lookup_util, expr_util, oracle.prng); the one
thing written out here is a x + b y of combineScalars and the sum of innerProduct, which no util module has.

A step's dimensions (DIMS):
  op      an entry of Parallel (msm_zprize_amd/parallel.py), or scalarsInto / free;
  fam     the family that wrote the entries the step's FIRST operand reads (the families of every entry are tracked; a
          step holds (fam, op) for every family found in that window); a fresh upload is a family of its own; "-" for an
          operation without a resident operand;
  window  of the first operand: the whole set; "tail": first > 0 and the range ends with the set; "middle": first > 0 and
          entries behind the range that the call must leave alone;
  dest    a new handle; "range": a range of an existing set apart from everything the call reads; "inplace": exactly
          where include/msmz.h allows it (the operand's own range; the low half for bindMle and sumcheckStep); "-" for a
          call that writes no set;
  size    the length of the first operand: 1, 2, a wave, a workgroup, the inversion chunk and a tile, each with - 1 and
          + 1 (size_classes(): from the geometry hooks of include/msmz_test.h), or for the power-of-two operations 2^k,
          k = 0 .. the transform's one-pass limit + 1;
  curve   all four.
RULES restates which combinations include/msmz.h allows; targets() lists every pair (fam, op), (op, dest), (op, size),
(op, curve) and every triple (op, window, dest), each either allowed or dropped by a named rule; cases(seed) covers the
allowed ones greedily and strings the steps into programs.  No set is longer than two tiles plus one.

At most one step in ten is a call the header refuses (a partial overlap, a range beyond its set, a destination on the
high half of a bindMle, on the gathered operand of matVec / lookup / a rotated column): it carries the status the
header names, and the runner asserts that status, the untouched *out_handle and the unchanged set.

Nothing here touches a GPU except run_program and what it calls."""
import ctypes as C
import random

import expr_util as EX
import lookup_util as LK
import matrix_util as MX
import mle_util as MLE
import ntt_util as NT
import scalar_ops_util as S
import scalar_scan_util as SC
import sumcheck_step_util as SS
from oracle import prng

CURVES = S.ALL
TE = "ed-on-bls12-377"
WAVE = 64          # lanes of a wave on CDNA
MSMZ_ERR_ARG = 1
GUARD = 8          # entries downloaded on either side of a written range

FAMILIES = ["upload", "random", "scalar", "scan", "ntt", "mle", "matrix", "lookup", "expr"]
# op -> (family, reads a resident operand, the destination kinds include/msmz.h allows, power-of-two sizes)
OPS = {
    "scalarsFromBytes": ("upload", False, ["new"], False),
    "scalarsInto": ("upload", False, ["range"], False),
    "randomScalars": ("random", False, ["new"], False),
    "scalarPowers": ("scalar", False, ["new"], False),
    "eqTable": ("mle", False, ["new"], True),
    "combineScalars": ("scalar", True, ["new", "range", "inplace"], False),
    "innerProduct": ("scalar", True, ["-"], False),
    "invertScalars": ("scan", True, ["new", "range", "inplace"], False),
    "scalarRecurrence": ("scan", True, ["new", "range", "inplace"], False),
    "prefixSums": ("scan", True, ["new", "range", "inplace"], False),
    "prefixProducts": ("scan", True, ["new", "range", "inplace"], False),
    "divideByLinear": ("scan", True, ["new"], False),
    "evaluateExpression": ("expr", True, ["new", "range", "inplace"], False),
    "ntt": ("ntt", True, ["new", "range", "inplace"], True),
    "evaluateMle": ("mle", True, ["-"], True),
    "sumcheckRound": ("mle", True, ["-"], True),
    "bindMle": ("mle", True, ["new", "range", "inplace"], True),
    "sumcheckStep": ("mle", True, ["range", "inplace"], True),
    "sparseMatrix": ("matrix", True, ["new"], False),
    "matVec": ("matrix", True, ["new", "range"], False),
    "lookupMultiplicities": ("lookup", True, ["new", "range"], False),
    "scalarsToBytes": ("upload", True, ["-"], False),
    "free": ("upload", True, ["-"], False),
}
WINDOWS = ["whole", "tail", "middle"]
DESTS = ["new", "range", "inplace", "-"]
# the operation that makes a set of a family and of any length from an upload (the other families: Builder.produce)
PRODUCER_OP = {"matrix": "matVec", "lookup": "lookupMultiplicities", "expr": "evaluateExpression"}

_geometry = None


def geometry():
    """the tile and chunk sizes, from the hooks of include/msmz_test.h (they need no context and no GPU)"""
    global _geometry
    if _geometry is None:
        from msm_zprize_amd._native import lib
        L = lib()

        def hook(name, k):
            v = [C.c_uint32(0) for _ in range(k)]
            getattr(L, name)(*[C.byref(x) for x in v])
            return [x.value for x in v]
        g = {}
        g["dot_tile"], _ = hook("msmz_test_scalar_dot_geometry", 2)
        g["rec_tile"], _, g["inv_chunk"] = hook("msmz_test_scalar_scan_geometry", 3)
        _, g["mle_tile"], g["round_tile"] = hook("msmz_test_mle_geometry", 3)
        g["step_tile"], = hook("msmz_test_sumcheck_step_geometry", 1)
        g["mat_tile"], _, _ = hook("msmz_test_matrix_geometry", 3)
        _, g["workgroup"] = hook("msmz_test_lookup_geometry", 2)
        g["expr_workgroup"], _ = hook("msmz_test_expr_geometry", 2)
        g["pass_log"] = NT.pass_log(L)
        _geometry = g
    return _geometry


def tiles():
    """the distinct tile sizes of the dot, recurrence and multilinear kernels, smallest first"""
    g = geometry()
    return sorted({g["dot_tile"], g["rec_tile"], g["mle_tile"]})


def size_classes():
    """name -> n for the operations of any length, name -> 2^k for the power-of-two ones"""
    g = geometry()
    any_n = {"1": 1, "2": 2}
    for name, v in [("wave", WAVE), ("workgroup", g["workgroup"]), ("inv_chunk", g["inv_chunk"])]:
        any_n[f"{name}-1"], any_n[f"{name}+1"] = v - 1, v + 1
    for k, t in enumerate(tiles()):   # "tile" is the smallest of them; a second distinct one would be "tile#2"
        name = "tile" if k == 0 else f"tile#{k + 1}"
        any_n[f"{name}-1"], any_n[name], any_n[f"{name}+1"] = t - 1, t, t + 1
    pow2 = {f"2^{k}": 1 << k for k in range(g["pass_log"] + 2)}
    return any_n, pow2


def max_set():
    g = geometry()
    return 2 * max(g["dot_tile"], g["rec_tile"], g["mle_tile"]) + 1


def dims():
    any_n, pow2 = size_classes()
    return {"op": list(OPS), "fam": FAMILIES + ["-"], "window": WINDOWS + ["-"], "dest": DESTS,
            "size": list(any_n) + list(pow2), "curve": list(CURVES)}


def size_of(cls):
    any_n, pow2 = size_classes()
    return any_n[cls] if cls in any_n else pow2[cls]


# ------------------------------------------------------------------------------------------------ the rule table
# (name, the dimensions it reads, the lines of include/msmz.h it restates, predicate: True = forbidden)
RULES = [
    ("no-operand", ("op", "fam"), "msmz_upload_scalars / _random_scalars / _scalars_powers / _eq_table / _import_scalars_into: "
     "no resident operand", lambda c: (c["fam"] == "-") != (not OPS[c["op"]][1])),
    ("no-operand-window", ("op", "window"), "the same: no operand, no window",
     lambda c: (c["window"] == "-") != (not OPS[c["op"]][1])),
    ("dest-kinds", ("op", "dest"), "the output rules of each call: msmz_scalars_combine and those that follow it; gathered "
     "operands (msmz_matrix_mul, msmz_scalars_lookup) have no in-place form; msmz_scalars_sumcheck_step creates no handle; "
     "dot, mle_eval, sumcheck_round, export and free write no set", lambda c: c["dest"] not in OPS[c["op"]][2]),
    ("power-of-two", ("op", "size"), "msmz_scalars_ntt: n = 2^log_n; the multilinear calls: 2^n_vars entries",
     lambda c: OPS[c["op"]][3] != c["size"].startswith("2^")),
    ("one-variable", ("op", "size"), "msmz_scalars_mle_bind / _sumcheck_round / _sumcheck_step: n_vars >= 1",
     lambda c: c["op"] in ("bindMle", "sumcheckRound", "sumcheckStep") and c["size"] == "2^0"),
    ("two-adicity", ("op", "size", "curve"), "msmz_scalars_ntt: log_n > S is MSMZ_ERR_UNSUPPORTED, S = 1 on ed-on-bls12-377 "
     "(tests/test_ntt_gpu.py, test_twisted_edwards_field_has_two_transforms)",
     lambda c: c["op"] == "ntt" and c["curve"] == TE and c["size"].startswith("2^") and int(c["size"][2:]) > 1),
    ("free-whole", ("op", "window"), "msmz_free frees a handle, not a range", lambda c: c["op"] == "free" and c["window"] != "whole"),
]
TARGET_KINDS = [("fam", "op"), ("op", "dest"), ("op", "size"), ("op", "curve"), ("op", "window", "dest")]


def violated(partial):
    """the first rule a (partial) choice of dimensions breaks, or None"""
    for name, fields, _, pred in RULES:
        if all(f in partial for f in fields) and pred(partial):
            return name
    return None


def targets():
    """{target: None if some step may hold it, else the rule that forbids it}; a target is a tuple of (dimension, value)"""
    D = dims()
    out = {}

    def walk(names, chosen):
        if not names:
            out[tuple(chosen.items())] = violated(chosen)
            return
        for v in D[names[0]]:
            walk(names[1:], {**chosen, names[0]: v})
    for kind in TARGET_KINDS:
        walk(list(kind), {})
    return out


def _holds(step):
    """the targets a step of a program holds (a refusal holds none)"""
    if step.get("refuse"):
        return []
    d = step["dims"]
    held = []
    for kind in TARGET_KINDS:
        if kind[0] == "fam":
            held += [(("fam", f), ("op", d["op"])) for f in d["fams"] or ["-"]]
        else:
            held.append(tuple((k, d[k]) for k in kind))
    return held


def complete(partial, rng):
    """a full choice of dimensions that extends `partial` and breaks no rule, or None"""
    D = dims()
    for _ in range(200):
        c = dict(partial)
        for name in D:
            if name not in c:
                c[name] = rng.choice(D[name])
        if violated(c) is None:
            return c
    return None


# ------------------------------------------------------------------------------------------------ values
def upload_values(label, step):
    """the values of an upload: seeded, with 0, 1 and q - 1 on the first and last indices of every window a later step
    was made to read, and on both sides of every tile edge inside it"""
    if "values" in step:
        return list(step["values"])
    q, n = S.order(label), step["n"]
    vals = S.random_below_2_250(n, random.Random(step["seed"]))
    for first, m in step["windows"]:
        last = first + m - 1
        if m == 1:
            vals[first] = (0, 1, q - 1)[step["seed"] % 3]
            continue
        for k, v in enumerate((0, 1, q - 1)):
            if k < m:
                vals[last - k] = (q - 1, 1, 0)[k]
                vals[first + k] = v
        for tile in tiles():
            for e in range(first + tile, last, tile):
                vals[e - 1], vals[e] = q - 1, 0
                if e - 2 > first:
                    vals[e - 2] = 1
                if e + 1 < last:
                    vals[e + 1] = 1
    return vals


def _le(v):
    return None if v is None else int(v).to_bytes(32, "little")


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """name -> list of ints, name -> the triples of a matrix; apply(step) -> the scalar results of the call"""

    def __init__(self, label):
        self.label, self.q = label, S.order(label)
        self.sets, self.mats = {}, {}

    def read(self, ref, n):
        name, first = ref
        v = self.sets[name][first:first + n]
        assert len(v) == n, (ref, n)
        return v

    def write(self, step, values):
        name, first = step["out"], step["first_out"]
        if step["new"]:
            assert name not in self.sets and first == 0
            self.sets[name] = list(values)
        else:
            assert first + len(values) <= len(self.sets[name])
            self.sets[name][first:first + len(values)] = values

    def apply(self, step):
        self.destination_rules(step)
        return getattr(self, "_" + step["op"])(step, step["args"])

    def destination_rules(self, st):
        """what include/msmz.h asks of the destination of a valid step, which the generator has to keep: apart from every
        range the call reads, or exactly on one where the call allows that"""
        a, op = st["args"], st["op"]
        if st["new"] or st["out"] is None or op in ("sumcheckStep", "scalarsInto"):   # (sumcheckStep: in its own model)
            return
        out = (st["out"], st["first_out"], st["m"])
        meet = lambda r: r[0] == out[0] and r[1] < out[1] + out[2] and out[1] < r[1] + r[2]   # noqa: E731
        n = a.get("n")
        if op in ("combineScalars", "invertScalars", "scalarRecurrence", "prefixSums", "prefixProducts"):
            rules = [((r[0], r[1], n), True) for r in (a.get(k) for k in ("x", "y", "a", "b")) if isinstance(r, list)]
        elif op == "evaluateExpression":
            named = {c: [] for c in range(len(a["columns"]))}
            for _, fs in a["terms"]:
                for c, rot in fs:
                    named[c].append(rot % n)
            rules = [((col[0], col[1], n), not any(named[c])) for c, col in enumerate(a["columns"]) if named[c]]
        elif op == "ntt":
            rules = [((a["x"][0], a["x"][1], a["count"] * a["n_in"]), a["n_in"] == 1 << a["log_n"])]
        elif op == "bindMle":
            whole = (a["x"][0], a["x"][1], a["count"] << a["n_vars"])
            if a["count"] == 1 and not a["low"] and out[:2] == whole[:2]:
                return
            rules = [(whole, False)]
        elif op == "matVec":
            shape = self.mats[a["matrix"]][3]
            rules = [((a["x"][0], a["x"][1], shape[0] if a["transpose"] else shape[1]), False)]
        elif op == "lookupMultiplicities":
            rules = [((a["x"][0], a["x"][1], n), False), ((a["column"][0], a["column"][1], a["col_n"]), False)]
        else:
            raise AssertionError(("no destination rule for", op))
        for r, exact_allowed in rules:
            assert not meet(r) or (exact_allowed and r == out), (op, out, r)

    # sources and data movement
    def _scalarsFromBytes(self, st, a):
        self.write(st, upload_values(self.label, a))

    def _scalarsInto(self, st, a):
        self.write(st, upload_values(self.label, a))

    def _randomScalars(self, st, a):
        self.write(st, [prng.scalar(a["seed"], i, self.q) for i in range(a["n"])])

    def _scalarPowers(self, st, a):   # init * ratio^i: the exclusive recurrence with a broadcast multiplier
        self.write(st, SC.recurrence(self.q, a["n"], a["ratio"], None, init=a["base"], exclusive=True)[0])

    def _eqTable(self, st, a):
        self.write(st, MLE.eq(a["point"], self.q, a["scale"]))

    def _scalarsToBytes(self, st, a):
        return {"bytes": S.encode(self.read(a["x"], a["n"]))}

    def _free(self, st, a):
        if a["x"][0] in self.mats:
            del self.mats[a["x"][0]]
        else:
            del self.sets[a["x"][0]]

    # element-wise
    def _coeff(self, c, n):
        if c is None:
            return [1] * n
        return [c] * n if isinstance(c, int) else self.read(tuple(c), n)

    def _combineScalars(self, st, a):
        n, q = a["n"], self.q
        out = [c * v % q for c, v in zip(self._coeff(a["a"], n), self.read(a["x"], n))]
        if a["y"] is not None:
            out = [(o + c * v) % q for o, c, v in zip(out, self._coeff(a["b"], n), self.read(a["y"], n))]
        self.write(st, out)

    def _innerProduct(self, st, a):
        x = self.read(a["x"], a["n"])
        y = [1] * a["n"] if a["y"] is None else self.read(a["y"], a["n"])
        return {"value": sum(u * v for u, v in zip(x, y)) % self.q}

    def _invertScalars(self, st, a):
        out, zeros = SC.inverse(self.q, self.read(a["x"], a["n"]))
        self.write(st, out)
        return {"zeros": zeros}

    def _evaluateExpression(self, st, a):
        cols = [self.read(c, a["n"]) for c in a["columns"]]
        self.write(st, EX.model(cols, [(c, [tuple(f) for f in fs]) for c, fs in a["terms"]], a["n"], self.q))

    # scans
    def _scalarRecurrence(self, st, a):
        n = a["n"]
        mult = a["a"] if a["a"] is None or isinstance(a["a"], int) else self.read(tuple(a["a"]), n)
        add = None if a["b"] is None else self.read(tuple(a["b"]), n)
        out, last = SC.recurrence(self.q, n, mult, add, a["init"], a["reverse"], a["exclusive"])
        self.write(st, out)
        return {"last": last}
    _prefixSums = _prefixProducts = _scalarRecurrence

    def _divideByLinear(self, st, a):
        out, last = SC.synthetic_division(self.q, self.read(tuple(a["b"]), a["n"]), a["a"])
        self.write(st, out)
        return {"last": last}

    # transforms
    def _ntt(self, st, a):
        n, q = 1 << a["log_n"], self.q
        w = NT.root(self.label, a["log_n"])
        out = []
        for k in range(a["count"]):
            out += NT.transform(q, self.read((a["x"][0], a["x"][1] + k * a["n_in"]), a["n_in"]), n, w, a["inverse"], a["shift"])
        self.write(st, out)

    # multilinear
    def _evaluateMle(self, st, a):
        return {"value": MLE.mle_eval(self.read(a["x"], 1 << len(a["point"])), a["point"], self.q)}

    def _sumcheckRound(self, st, a):
        tabs = [self.read(t, 1 << a["n_vars"]) for t in a["tables"]]
        return {"values": MLE.round_poly(tabs, [tuple(t) for t in a["terms"]], self.q, a["low"])}

    def _bindMle(self, st, a):
        n, out = 1 << a["n_vars"], []
        for k in range(a["count"]):
            out += MLE.bind(self.read((a["x"][0], a["x"][1] + k * n), n), a["r"], self.q, a["low"])
        self.write(st, out)

    def _sumcheckStep(self, st, a):
        tabs = [self.read(t, 1 << a["n_vars"]) for t in a["tables"]]
        h = 1 << (a["n_vars"] - 1)
        meet = lambda u, nu, v, nv: u[0] == v[0] and u[1] < v[1] + nv and v[1] < u[1] + nu   # noqa: E731
        for j, o in enumerate(a["outs"]):   # the destination rules of the call, which the generator has to keep
            assert not any(meet(o, h, p, h) for p in a["outs"][:j]), st
            assert not any(meet(o, h, t, 2 * h) for k, t in enumerate(a["tables"]) if k != j), st
            assert not meet(o, h, a["tables"][j], 2 * h) or (o == a["tables"][j] and not a["low"]), st
        bound, degree, values = SS.step(tabs, [tuple(t) for t in a["terms"]], a["r"], self.q, a["low"])
        for (name, first), f in zip(a["outs"], bound):
            self.sets[name][first:first + len(f)] = f
        return {"degree": degree, "values": values}

    # matrices and lookups
    def _sparseMatrix(self, st, a):
        vals = None if a["values"] is None else self.read(a["values"], a["nnz"])
        r = random.Random(a["seed"])
        rows = [r.randrange(a["shape"][0]) for _ in range(a["nnz"])]
        cols = [r.randrange(a["shape"][1]) for _ in range(a["nnz"])]
        self.mats[st["out"]] = (rows, cols, vals, a["shape"], a["orientations"])

    def _matVec(self, st, a):
        rows, cols, vals, shape, _ = self.mats[a["matrix"]]
        n_in, n_out = (shape[0], shape[1]) if a["transpose"] else (shape[1], shape[0])
        self.write(st, MX.matvec(rows, cols, vals, self.read(a["x"], n_in), n_out, self.q, a["transpose"]))

    def _lookupMultiplicities(self, st, a):
        m, pos, info = LK.model(self.read(a["x"], a["n"]), self.read(a["column"], a["col_n"]))
        self.write(st, m)
        return {"info": info, "positions": pos if a["positions"] else None}


def written(step):
    """the ranges [(set, first, length)] a valid step writes"""
    a = step["args"]
    if step["op"] == "sumcheckStep":
        return [(name, first, 1 << (a["n_vars"] - 1)) for name, first in a["outs"]]
    if step.get("out") is None or step["op"] in ("sparseMatrix",):
        return []
    return [(step["out"], step["first_out"], step["m"])]


def _names(args):
    """the set and matrix names the arguments of a step mention"""
    out = []
    for v in args.values() if isinstance(args, dict) else args:
        if isinstance(v, str) and v[:1] in "sm" and v[1:].isdigit():
            out.append(v)
        elif isinstance(v, (list, dict)):
            out += _names(v)
    return out


def expected(label, program):
    """the model run over a program once: per step the scalar results and the bytes of every written range with GUARD
    entries on either side, then every live set whole.  A refusal leaves the model as it was: what is compared there is
    the destination set, whole."""
    M = Model(label)
    per_step = []
    for st in program["steps"]:
        if st.get("refuse"):
            name = st["out"]
            assert all(r in M.sets or r in M.mats for r in _names(st["args"])), st   # (refused, but about live sets)
            assert st["refuse"] != "on-a-rotated-column" or st["args"]["n"] >= 2, st   # (one entry: every rotation is 0)
            per_step.append({"results": None, "ranges": [] if st["new"] else [(name, 0, S.encode(M.sets[name]))]})
            continue
        results = M.apply(st)
        ranges = []
        for name, first, m in written(st):
            lo, hi = max(0, first - GUARD), min(len(M.sets[name]), first + m + GUARD)
            for lo, hi in program.get("probes") or [(lo, hi)]:   # (a directed program names the ranges it downloads)
                ranges.append((name, lo, S.encode(M.sets[name][lo:hi])))
        per_step.append({"results": results, "ranges": ranges})
    return per_step, {name: S.encode(v) for name, v in M.sets.items()}, M


# ------------------------------------------------------------------------------------------------ the generator
class Builder:
    """strings steps into one program: tracks the length of every live set and the family that wrote each entry"""

    def __init__(self, label, rng):
        self.label, self.q, self.rng = label, S.order(label), rng
        self.steps, self.len, self.by, self.mats = [], {}, {}, {}   # by: the operation that wrote each entry of a set
        self.n_names = self.depth = 0
        self.fresh_only = False   # operands from fresh sets only: under a step whose destination is already fixed
        self.want = {}        # what a directed case asks of its next step beyond the dimensions
        self.freed = []       # lengths of freed sets: housekeeping allocates the last one again
        self.max_log = min(NT.two_adicity(label), geometry()["pass_log"] + 1)

    # ---- bookkeeping
    def name(self, prefix="s"):
        self.n_names += 1
        return f"{prefix}{self.n_names}"

    def scalar(self, edge=True):
        r = self.rng.random()
        if edge and r < 0.15:
            return self.rng.choice([0, 1, self.q - 1])
        return self.rng.randrange(2, self.q)

    def emit(self, op, args, dims, out=None, first_out=0, m=0, new=False, refuse=None):
        fam = OPS[op][0]
        st = {"op": op, "args": args, "out": out, "first_out": first_out, "m": m, "new": new, "dims": dims}
        if refuse:
            st["refuse"], st["status"] = refuse, MSMZ_ERR_ARG
            st["dims"] = dict(dims, refusal=refuse)
            self.steps.append(st)
            return st
        if new and op != "sparseMatrix":
            self.len[out], self.by[out] = m, [op] * m
        for name, first, k in written(st):
            self.by[name][first:first + k] = [op] * k
        self.steps.append(st)
        return st

    def apart(self, name, first, m, reads):
        return all(r[0] != name or first + m <= r[1] or r[1] + r[2] <= first for r in reads)

    # ---- operands
    def upload(self, n, windows=()):
        """a fresh upload of n entries; `windows`: the ranges later steps were made to read, which get the edge values"""
        name = self.name()
        args = {"n": n, "seed": self.rng.randrange(1 << 30), "windows": [list(w) for w in windows]}
        self.emit("scalarsFromBytes", args, self.dims_of("scalarsFromBytes", [], "-", "new", n), out=name, m=n, new=True)
        return name

    def dims_of(self, op, writers, window, dest, n):
        """the dimensions of a step; `writers`: the operations that wrote the entries its first operand reads"""
        fams = {OPS[w][0] for w in writers}
        any_n, pow2 = size_classes()
        table = pow2 if OPS[op][3] else any_n
        cls = next((k for k, v in table.items() if v == n), "other")
        return {"op": op, "fams": sorted(fams), "producers": sorted(writers), "window": window, "dest": dest, "size": cls,
                "curve": self.label}

    def window_at(self, window, n):
        """(set length, first) of a fresh set for a window of n entries"""
        cap = max_set()
        lead = self.rng.randrange(1, 40)
        tail = self.rng.randrange(1, 40)
        if window == "whole" or n + 80 > cap:   # (a second operand near the cap: the whole of a fresh set)
            return n, 0
        if window == "tail":
            return min(cap, n + lead), min(cap, n + lead) - n
        lead = min(lead, cap - n - 1)
        return min(cap, n + lead + tail), lead

    def obtain(self, fam, window, n, reuse=True):
        """(set, first): a window of n entries of kind `window` in which family `fam` wrote something (None: any)"""
        names = [s for s in self.len if s not in self.mats]
        self.rng.shuffle(names)
        for name in names if reuse and not self.fresh_only else []:
            L = self.len[name]
            if window == "whole" and L == n:
                first = 0
            elif window == "tail" and L > n:
                first = L - n
            elif window == "middle" and L >= n + 2:
                first = self.rng.randrange(1, L - n)
            else:
                continue
            if fam is None or fam in {OPS[w][0] for w in set(self.by[name][first:first + n])}:
                return name, first
        L, first = self.window_at(window, n)
        return self.produce(fam or "upload", L, first, n), first

    def any_range(self, n, reads=()):
        """(set, first) of n entries of any live set, or of a fresh upload -- for the second operands"""
        names = [s for s in self.len if self.len[s] >= n]
        if names and self.rng.random() < 0.7 and not self.fresh_only:
            name = self.rng.choice(names)
            return name, self.rng.randrange(self.len[name] - n + 1)
        L, first = self.window_at(self.rng.choice(WINDOWS), n)
        return self.upload(L, [(first, n)]), first

    def produce(self, fam, L, first, n):
        """a new set of L entries in which family `fam` wrote entries of [first, first + n)"""
        if fam == "upload" and self.rng.random() < 0.25:   # an upload overwritten in the window by host bytes
            base = self.upload(L)
            self.step("scalarsInto", None, "-", "range", n, force=(base, first))
            return base
        if fam == "upload":
            return self.upload(L, [(first, n)])
        if fam == "random":
            return self.random_set(L)
        if fam == "scalar" and self.rng.random() < 0.5:
            return self.step("combineScalars", "upload", "whole", "new", L)["out"]
        if fam == "scalar":
            return self.powers(L)
        if fam == "scan":
            op = self.rng.choice(["invertScalars", "scalarRecurrence", "prefixSums", "prefixProducts", "divideByLinear"])
            return self.step(op, "upload", "whole", "new", L)["out"]
        if fam in ("ntt", "mle"):
            pow2 = L & (L - 1) == 0
            if pow2 and fam == "ntt" and L.bit_length() - 1 <= self.max_log:
                return self.step("ntt", "upload", "whole", "new", L)["out"]
            if pow2 and fam == "mle" and self.rng.random() < 0.7:
                return self.eq_table(L)
            # any other length: the family writes a power of two inside the window of an uploaded set
            p = 1 << min(n.bit_length() - 1, self.max_log if fam == "ntt" else 30)
            base = self.upload(L, [(first, n)])
            self.fresh_only = True   # (a live set of the source's length may be `base` itself: its destination)
            if fam == "ntt":
                self.step("ntt", "upload", "whole", "range", p, force=(base, first))
            elif self.rng.random() < 0.5:
                self.step("bindMle", "upload", "whole", "range", 2 * p, force=(base, first))
            else:
                self.step("sumcheckStep", "upload", "whole", "range", 2 * p, force=(base, first))
            self.fresh_only = False
            return base
        return self.step(PRODUCER_OP[fam], "upload", "whole", "new", L)["out"]

    def random_set(self, L):
        name = self.name()
        self.emit("randomScalars", {"n": L, "seed": self.rng.randrange(1 << 30)},
                  self.dims_of("randomScalars", [], "-", "new", L), out=name, m=L, new=True)
        return name

    def powers(self, L):
        name = self.name()
        self.emit("scalarPowers", {"n": L, "ratio": self.scalar(), "base": self.scalar()},
                  self.dims_of("scalarPowers", [], "-", "new", L), out=name, m=L, new=True)
        return name

    def eq_table(self, L):
        name = self.name()
        self.emit("eqTable", {"point": [self.scalar() for _ in range(L.bit_length() - 1)], "scale": self.scalar(False)},
                  self.dims_of("eqTable", [], "-", "new", L), out=name, m=L, new=True)
        return name

    def destination(self, kind, m, reads, inplace=None, force=None):
        """(set or None for a new handle, first_out)"""
        if force:
            return force
        if kind in ("new", "-"):
            return None, 0
        if kind == "inplace":
            return inplace
        names = [s for s in self.len if self.len[s] >= m]
        self.rng.shuffle(names)
        for name in sorted(names, key=lambda s: s not in {r[0] for r in reads}):   # the operands' own sets first
            L = self.len[name]
            for first in (L - m, 0, self.rng.randrange(L - m + 1)):
                if self.apart(name, first, m, reads) and (first > 0 or L > m):
                    return name, first
        L, first = self.window_at("middle", m)
        return self.upload(L), first

    def refusal(self, op, args, dims, x, n, m):
        """the same call with a destination the header refuses: a partial overlap with the operand, or, where the operand
        leaves no room for one, a range beyond the set"""
        name, first = x
        L = self.len[name]
        if n >= 2 and first + 1 + m <= L:
            self.emit(op, args, dims, out=name, first_out=first + 1, m=m, refuse="partial-overlap")
        elif n >= 2 and first >= 1 and first - 1 + m <= L:
            self.emit(op, args, dims, out=name, first_out=first - 1, m=m, refuse="partial-overlap")
        else:
            self.emit(op, args, dims, out=name, first_out=L - m + 1, m=m, refuse="beyond-the-set")

    # ---- one step of every operation
    def step(self, op, fam, window, dest, n, force=None, refuse=False):
        self.depth += 1
        st = getattr(self, "_" + op)(fam, window, dest, n, force, refuse)
        self.depth -= 1
        if self.depth == 0:   # (not under a step that has chosen its operands already)
            self.housekeeping()
        return st

    def housekeeping(self):
        """free the oldest sets once more than eight are live, so that handles and their memory come back"""
        while len(self.len) > 8:
            for name in list(self.len)[:2]:
                self.free(name)
            # ... and the size of the last one again, so that a new handle may land on the freed one's address
            L = self.freed.pop()
            self.rng.choice([self.upload, self.random_set, self.powers])(L)

    def free(self, name):
        L = self.len[name]
        fams = set(self.by[name])
        self.emit("free", {"x": [name, 0]}, self.dims_of("free", fams, "whole", "-", L))
        del self.len[name], self.by[name]
        self.freed.append(L)

    def operand(self, fam, window, n):
        name, first = self.obtain(fam, window, n)
        return (name, first), set(self.by[name][first:first + n])

    def _simple(self, op, fam, window, dest, n, force, refuse, args_of, m=None, extra_reads=()):
        """an operation of one window x, a result of m entries, in place exactly on x"""
        x, fams = self.operand(fam, window, n)
        m = n if m is None else m
        args = args_of(x)
        reads = [(x[0], x[1], n)] + list(extra_reads)
        d = self.dims_of(op, fams, window, dest, n)
        if refuse:
            self.refusal(op, args, d, x, n, m)
        out, first_out = self.destination(dest, m, reads, inplace=x, force=force)
        new = out is None
        return self.emit(op, args, d, out=self.name() if new else out, first_out=first_out, m=m, new=new)

    def _scalarsFromBytes(self, fam, window, dest, n, force, refuse):
        self.upload(n, [(0, n)])
        return self.steps[-1]

    def _scalarsInto(self, fam, window, dest, n, force, refuse):
        out, first_out = self.destination("range", n, [], force=force)
        args = {"n": n, "seed": self.rng.randrange(1 << 30), "windows": [[0, n]]}
        return self.emit("scalarsInto", args, self.dims_of("scalarsInto", [], "-", "range", n), out=out, first_out=first_out, m=n)

    def _randomScalars(self, fam, window, dest, n, force, refuse):
        self.produce("random", n, 0, n)
        return self.steps[-1]

    def _scalarPowers(self, fam, window, dest, n, force, refuse):
        self.powers(n)
        return self.steps[-1]

    def _eqTable(self, fam, window, dest, n, force, refuse):
        self.eq_table(n)
        return self.steps[-1]

    def _scalarsToBytes(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, window, n)
        return self.emit("scalarsToBytes", {"x": list(x), "n": n}, self.dims_of("scalarsToBytes", fams, window, "-", n))

    def _free(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, "whole", n)
        self.free(x[0])
        return self.steps[-1]

    def _combineScalars(self, fam, window, dest, n, force, refuse):
        kinds = ["none", "host", "resident"]
        two = self.rng.random() < 0.6

        def coeff(kind):
            return None if kind == "none" else self.scalar() if kind == "host" else list(self.any_range(n))

        def args_of(x):
            a = {"n": n, "x": list(x), "a": coeff(self.rng.choice(kinds)), "y": None, "b": None}
            if two:
                a["y"], a["b"] = list(self.any_range(n)), coeff(self.rng.choice(kinds))
            return a
        # the destination lies apart from every input range, or exactly on x: the second operands are known only after
        # args_of ran, so they are collected from the arguments
        x, fams = self.operand(fam, window, n)
        args = args_of(x)
        reads = [(x[0], x[1], n)] + [(r[0], r[1], n) for r in (args["a"], args["y"], args["b"]) if isinstance(r, list)]
        d = self.dims_of("combineScalars", fams, window, dest, n)
        if dest == "inplace" and not all(r[0] != x[0] or r[1:] == (x[1], n) or self.apart(x[0], x[1], n, [r]) for r in reads):
            # another operand meets x partly: read it from a copy elsewhere (a fresh upload)
            for key in ("a", "y", "b"):
                if isinstance(args[key], list) and args[key][0] == x[0] and tuple(args[key]) != x:
                    args[key] = [self.upload(n, [(0, n)]), 0]
            reads = [(x[0], x[1], n)]
        if refuse:
            self.refusal("combineScalars", args, d, x, n, n)
        out, first_out = self.destination(dest, n, reads, inplace=x, force=force)
        new = out is None
        return self.emit("combineScalars", args, d, out=self.name() if new else out, first_out=first_out, m=n, new=new)

    def _innerProduct(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, window, n)
        y = list(self.any_range(n)) if self.rng.random() < 0.7 else None
        return self.emit("innerProduct", {"n": n, "x": list(x), "y": y}, self.dims_of("innerProduct", fams, window, "-", n))

    def _invertScalars(self, fam, window, dest, n, force, refuse):
        return self._simple("invertScalars", fam, window, dest, n, force, refuse, lambda x: {"n": n, "x": list(x)})

    def _evaluateExpression(self, fam, window, dest, n, force, refuse):
        rotated = dest != "inplace" and (self.want.pop("rotated", False) or self.rng.random() < 0.6)
        rotated = rotated and n >= 2   # (in a column of one entry every rotation is 0 mod n)
        x, fams = self.operand(fam, window, n)
        ncols = self.rng.randrange(1, 5)
        cols = [list(x)] + [list(self.any_range(n)) for _ in range(ncols - 1)]
        rots = EX.rotations(n) if rotated else [0, n, -n]
        terms = []
        for _ in range(self.rng.randrange(1, 5)):
            factors = [[self.rng.randrange(ncols), self.rng.choice(rots)] for _ in range(self.rng.randrange(0, 5))]
            terms.append([self.rng.choice([None, self.scalar()]), factors])
        terms.append([self.scalar(False), [[0, 0]]])   # the first operand is always read
        if dest == "inplace":   # out = y out + gate: column 0 at rotation 0 only, every other column apart from it
            terms = [[c, [[k, 0] for k, _ in fs]] for c, fs in terms]
            cols = [cols[0]] + [c if self.apart(c[0], c[1], n, [(x[0], x[1], n)]) or tuple(c) == x else [self.upload(n, [(0, n)]), 0]
                                for c in cols[1:]]
        args = {"n": n, "columns": cols, "terms": terms}
        reads = [(c[0], c[1], n) for c in cols]
        d = self.dims_of("evaluateExpression", fams, window, dest, n)
        d["rotated"] = rotated
        if refuse:
            if rotated:   # a rotated column is gathered: a destination exactly on it is refused too
                args = dict(args, terms=terms + [[None, [[0, 1]]]])
                self.emit("evaluateExpression", args, d, out=x[0], first_out=x[1], m=n, refuse="on-a-rotated-column")
                args = {"n": n, "columns": cols, "terms": terms}
            else:
                self.refusal("evaluateExpression", args, d, x, n, n)
        out, first_out = self.destination(dest, n, reads, inplace=x, force=force)
        new = out is None
        return self.emit("evaluateExpression", args, d, out=self.name() if new else out, first_out=first_out, m=n, new=new)

    def _recurrence(self, op, fam, window, dest, n, force, refuse, mode, reverse, exclusive, init):
        _, mult, addend = SC.MODE[mode]
        x, fams = self.operand(fam, window, n)
        other = list(self.any_range(n)) if (mult == "resident" and addend) else None
        if other and dest == "inplace" and other[0] == x[0] and tuple(other) != x and not self.apart(x[0], x[1], n, [(other[0], other[1], n)]):
            other = [self.upload(n, [(0, n)]), 0]
        a = None if mult is None else (self.scalar() if mult == "broadcast" else list(x))
        b = (other if mult == "resident" else list(x)) if addend else None
        args = {"n": n, "a": a, "b": b, "init": init, "reverse": reverse, "exclusive": exclusive, "mode": mode}
        reads = [(r[0], r[1], n) for r in (a, b) if isinstance(r, list)]
        d = self.dims_of(op, fams, window, dest, n)
        if refuse:
            self.refusal(op, args, d, x, n, n)
        out, first_out = self.destination(dest, n, reads, inplace=x, force=force)
        new = out is None
        return self.emit(op, args, d, out=self.name() if new else out, first_out=first_out, m=n, new=new)

    def _scalarRecurrence(self, fam, window, dest, n, force, refuse):
        mode = self.rng.choice(SC.MODES)[0]
        init = self.rng.choice([None, self.scalar()])
        return self._recurrence("scalarRecurrence", fam, window, dest, n, force, refuse, mode, self.rng.random() < 0.5,
                                self.rng.random() < 0.5, init)

    def _prefixSums(self, fam, window, dest, n, force, refuse):
        return self._recurrence("prefixSums", fam, window, dest, n, force, refuse, "sums", self.rng.random() < 0.3,
                                self.rng.random() < 0.5, None)

    def _prefixProducts(self, fam, window, dest, n, force, refuse):
        return self._recurrence("prefixProducts", fam, window, dest, n, force, refuse, "products", self.rng.random() < 0.3,
                                self.rng.random() < 0.5, None)

    def _divideByLinear(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, window, n)
        args = {"n": n, "a": self.scalar(), "b": list(x)}
        return self.emit("divideByLinear", args, self.dims_of("divideByLinear", fams, window, "new", n), out=self.name(), m=n, new=True)

    def _ntt(self, fam, window, dest, n, force, refuse):
        log_n = n.bit_length() - 1
        assert 1 << log_n == n and log_n <= self.max_log
        inverse = self.rng.random() < 0.4
        count = self.rng.choice([1, 1, 2, 3])
        count = self.want.pop("count", count)
        if dest == "range" or force:
            count = 1
        while count > 1 and count * n > max_set() - 80:   # (room for a window that is not the whole set)
            count -= 1
        n_in = n
        if not inverse and dest != "inplace" and n > 1 and self.rng.random() < 0.5:
            n_in = self.rng.randrange(1, n)
        shift = self.scalar(False) if self.rng.random() < 0.5 else None
        x, fams = self.operand(fam, window, count * n_in)
        args = {"log_n": log_n, "x": list(x), "n_in": n_in, "count": count, "inverse": inverse, "shift": shift}
        d = self.dims_of("ntt", fams, window, dest, n)
        if refuse:
            self.refusal("ntt", args, d, x, count * n_in, count * n)
        out, first_out = self.destination(dest, count * n, [(x[0], x[1], count * n_in)], inplace=x, force=force)
        new = out is None
        return self.emit("ntt", args, d, out=self.name() if new else out, first_out=first_out, m=count * n, new=new)

    def _evaluateMle(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, window, n)
        args = {"x": list(x), "point": [self.scalar() for _ in range(n.bit_length() - 1)]}
        return self.emit("evaluateMle", args, self.dims_of("evaluateMle", fams, window, "-", n))

    def _terms(self, nt):
        terms = SS.mixed_terms(nt, self.q, self.rng)
        return [[c, mask] for c, mask in terms]

    def _sumcheckRound(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, window, n)
        nt = self.rng.randrange(1, 7)
        tables = [list(x)] + [list(self.any_range(n)) for _ in range(nt - 1)]
        args = {"tables": tables, "n_vars": n.bit_length() - 1, "terms": self._terms(nt), "low": self.rng.random() < 0.5}
        return self.emit("sumcheckRound", args, self.dims_of("sumcheckRound", fams, window, "-", n))

    def _bindMle(self, fam, window, dest, n, force, refuse):
        v, h = n.bit_length() - 1, n // 2
        count = 1 if dest == "inplace" or force or dest == "range" else self.want.pop("count", self.rng.choice([1, 2, 3]))
        while count > 1 and count * n > max_set() - 80:   # (room for a window that is not the whole set)
            count -= 1
        low = dest != "inplace" and self.rng.random() < 0.5
        x, fams = self.operand(fam, window, count * n)
        args = {"x": list(x), "n_vars": v, "count": count, "low": low, "r": self.scalar()}
        d = self.dims_of("bindMle", fams, window, dest, n)
        if refuse:   # the high half of the source
            self.emit("bindMle", args, d, out=x[0], first_out=x[1] + h, m=count * h, refuse="high-half")
        out, first_out = self.destination(dest, count * h, [(x[0], x[1], count * n)], inplace=x, force=force)
        new = out is None
        return self.emit("bindMle", args, d, out=self.name() if new else out, first_out=first_out, m=count * h, new=new)

    def _sumcheckStep(self, fam, window, dest, n, force, refuse):
        v, h = n.bit_length() - 1, n // 2
        nt = self.rng.randrange(1, 7)
        x, fams = self.operand(fam, window, n)
        tables, reads = [list(x)], [(x[0], x[1], n)]
        if force:
            reads.append((force[0], force[1], h))   # (no other table where the first one's destination is to be)
        for _ in range(nt - 1):   # every table apart from the others: each is bound where the rules of the call allow
            name, first = self.obtain(None, self.rng.choice(WINDOWS), n)
            if not self.apart(name, first, n, reads):
                name, first = self.upload(n, [(0, n)]), 0
            tables.append([name, first])
            reads.append((name, first, n))
        low = dest != "inplace" and self.rng.random() < 0.5
        outs = []
        for j, t in enumerate(tables):
            if dest == "inplace":
                outs.append(list(t))
            else:
                o = self.destination("range", h, reads, force=force if j == 0 else None)
                outs.append(list(o))
                reads.append((o[0], o[1], h))
        args = {"tables": tables, "outs": outs, "n_vars": v, "terms": self._terms(nt), "low": low, "r": self.scalar(),
                "in_place": dest == "inplace"}
        if refuse:   # in place in the low order: the pairs of the bound table lie over its own sources
            self.emit("sumcheckStep", dict(args, low=True, in_place=True, outs=[list(t) for t in tables]),
                      self.dims_of("sumcheckStep", fams, window, dest, n), out=x[0], first_out=x[1], m=h, refuse="low-in-place")
        return self.emit("sumcheckStep", args, self.dims_of("sumcheckStep", fams, window, dest, n), m=h)

    def _matrix(self, values, nnz, shape, orientations):
        name = self.name("m")
        args = {"values": values, "nnz": nnz, "shape": list(shape), "orientations": orientations, "seed": self.rng.randrange(1 << 30)}
        return name, args

    def _sparseMatrix(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, window, n)   # the values: one per non-zero
        top = min(2 * n + 2, max_set() + 1)
        shape = (self.rng.randrange(1, top), self.rng.randrange(1, top))
        name, args = self._matrix(list(x), n, shape, self.rng.choice(["rows", "cols", "both"]))
        st = self.emit("sparseMatrix", args, self.dims_of("sparseMatrix", fams, window, "new", n), out=name, m=0, new=True)
        self.mats[name] = (shape, args["orientations"])
        # the matrix is checked through its products: one per orientation it was built for, into new sets
        for transpose in {"rows": [False], "cols": [True], "both": [False, True]}[args["orientations"]]:
            n_in, n_out = (shape[0], shape[1]) if transpose else (shape[1], shape[0])
            v = list(self.any_range(n_in))
            writers = set(self.by[v[0]][v[1]:v[1] + n_in]) | {"sparseMatrix"}
            self.emit("matVec", {"matrix": name, "x": v, "transpose": transpose}, self.dims_of("matVec", writers, "other", "new", n_in),
                      out=self.name(), m=n_out, new=True)
        self.emit("free", {"x": [name, 0]}, self.dims_of("free", set(), "other", "-", 0))
        del self.mats[name]
        return st

    def _matVec(self, fam, window, dest, n, force, refuse):
        transpose = self.rng.random() < 0.5
        x, fams = self.operand(fam, window, n)
        n_out = n   # (a square matrix: the result has as many entries as x)
        shape = (n, n_out) if transpose else (n_out, n)
        values = self.rng.choice([None, "resident"])
        nnz = self.rng.choice([n, max(1, n // 2), min(max_set(), 2 * n)])
        values = list(self.any_range(nnz)) if values else None
        name, margs = self._matrix(values, nnz, shape, "cols" if transpose else "rows")
        self.emit("sparseMatrix", margs, self.dims_of("sparseMatrix", set() if values is None else set(self.by[values[0]][values[1]:values[1] + nnz]),
                                                      "other", "new", nnz), out=name, m=0, new=True)
        self.mats[name] = (shape, margs["orientations"])
        args = {"matrix": name, "x": list(x), "transpose": transpose}
        d = self.dims_of("matVec", fams | {"sparseMatrix"}, window, dest, n)   # (it reads the matrix too)
        if refuse:   # x is gathered: a destination exactly on it is refused
            self.emit("matVec", args, d, out=x[0], first_out=x[1], m=n_out, refuse="on-the-gathered-operand")
        out, first_out = self.destination(dest, n_out, [(x[0], x[1], n)], force=force)
        new = out is None
        st = self.emit("matVec", args, d, out=self.name() if new else out, first_out=first_out, m=n_out, new=new)
        self.emit("free", {"x": [name, 0]}, self.dims_of("free", set(), "other", "-", 0))
        del self.mats[name]
        return st

    def _lookupMultiplicities(self, fam, window, dest, n, force, refuse):
        x, fams = self.operand(fam, window, n)   # the table
        col_n = self.rng.choice([1, n, WAVE + 1, geometry()["workgroup"] + 1, min(max_set(), 2 * n + 3)])
        # most of the column is drawn from the table when it is a range of the table's own set; otherwise any range
        column = [x[0], self.rng.randrange(self.len[x[0]] - col_n + 1)] if self.len[x[0]] >= col_n and self.rng.random() < 0.6 \
            else list(self.any_range(col_n))
        args = {"n": n, "x": list(x), "column": column, "col_n": col_n, "positions": self.rng.random() < 0.5}
        reads = [(x[0], x[1], n), (column[0], column[1], col_n)]
        d = self.dims_of("lookupMultiplicities", fams, window, dest, n)
        if refuse:
            self.emit("lookupMultiplicities", args, d, out=x[0], first_out=x[1], m=n, refuse="on-the-gathered-operand")
        out, first_out = self.destination(dest, n, reads, force=force)
        new = out is None
        return self.emit("lookupMultiplicities", args, d, out=self.name() if new else out, first_out=first_out, m=n, new=new)


REFUSABLE = {"sumcheckStep", "combineScalars", "invertScalars", "scalarRecurrence", "prefixSums", "prefixProducts", "evaluateExpression", "ntt",
             "bindMle", "matVec", "lookupMultiplicities"}
STEPS_PER_PROGRAM = 6   # covering steps; the steps that make their operands come on top


def specs(seed=1):
    """the greedy covering: full choices of dimensions, each picked for the most targets not yet held among a few random
    completions of the first target still open"""
    rng = random.Random(seed)
    allowed = [t for t, why in targets().items() if why is None]
    open_ = set(allowed)
    out = []

    def would_hold(c):
        return {tuple((k, c[k]) for k in kind) for kind in TARGET_KINDS}
    for t in sorted(allowed, key=repr):
        if t not in open_:
            continue
        best, gain = None, -1
        for _ in range(12):
            c = complete(dict(t), rng)
            if c is None:
                continue
            g = len(would_hold(c) & open_)
            if g > gain:
                best, gain = c, g
        assert best is not None, t
        open_ -= would_hold(best)
        out.append(best)
    return out


# the directed cases: what the covering has no dimension for
DIRECTED = [
    # one set through four families in place and back out: every step reads what the one before wrote
    dict(curve="bls12-377", chain=[("scalarPowers", "-", "-", "new", "tile+1"), ("invertScalars", "scalar", "whole", "inplace", "tile+1"),
                                   ("prefixProducts", "scan", "middle", "inplace", "tile-1"), ("evaluateExpression", "scan", "tail", "inplace", "workgroup+1"),
                                   ("innerProduct", "expr", "whole", "-", "tile+1")]),
    # a transform, a bind and a step in place on one power-of-two set
    dict(curve="pallas", chain=[("ntt", "upload", "whole", "new", "2^11"), ("ntt", "ntt", "whole", "inplace", "2^11"),
                                ("bindMle", "ntt", "whole", "inplace", "2^11"), ("sumcheckStep", "mle", "tail", "inplace", "2^10"),
                                ("evaluateMle", "mle", "tail", "-", "2^9"),
                                ("ntt", "mle", "middle", "new", "2^6", dict(count=3)),   # three vectors, three tables
                                ("bindMle", "ntt", "whole", "new", "2^5", dict(count=3))]),
    dict(curve=TE, chain=[("ntt", "upload", "middle", "range", "2^1"), ("lookupMultiplicities", "ntt", "middle", "range", "wave+1"),
                          ("matVec", "lookup", "middle", "new", "wave-1"), ("free", "matrix", "whole", "-", "wave-1")]),
    # one refusal of every kind, whatever the seed draws
    dict(curve="bls12-377", chain=[("evaluateExpression", "upload", "middle", "range", "wave+1", dict(refuse=True, rotated=True)),
                                   ("combineScalars", "expr", "middle", "inplace", "wave-1", dict(refuse=True)),
                                   ("invertScalars", "scalar", "whole", "new", "1", dict(refuse=True)),
                                   ("bindMle", "scan", "tail", "new", "2^1", dict(refuse=True)),
                                   ("matVec", "mle", "whole", "range", "1", dict(refuse=True)),
                                   ("lookupMultiplicities", "matrix", "whole", "new", "1", dict(refuse=True)),
                                   ("sumcheckStep", "lookup", "whole", "inplace", "2^2", dict(refuse=True))]),
    dict(curve="bls12-381", chain=[("randomScalars", "-", "-", "new", "inv_chunk+1"), ("divideByLinear", "random", "tail", "new", "inv_chunk-1"),
                                   ("sparseMatrix", "scan", "whole", "new", "inv_chunk-1"), ("scalarsInto", "-", "-", "range", "2"),
                                   ("scalarsToBytes", "upload", "middle", "-", "wave+1")]),
]


def _build(label, chain, rng, refusals):
    b = Builder(label, rng)
    for op, fam, window, dest, size, *more in chain:
        b.want = dict(more[0]) if more else {}
        refuse = b.want.pop("refuse", False) or (op in REFUSABLE and dest != "-" and rng.random() < refusals)
        b.step(op, None if fam == "-" else fam, window, dest, size_of(size), refuse=refuse)
    return b.steps


MSMZ_ERR_UNSUPPORTED = 4
BLOCK = 1 << 16   # a multi-device context deals its sets in blocks of 2^16 entries (include/msmz.h)


def two_engine_program(label="bls12-377", seed=1):
    """The directed program for a context of two engines: n = 2^16 + 300, so that the second engine holds 300 entries, from
    the operations csrc/multi.h runs per engine -- powers, combine, inverse, dot, unrotated expressions -- every first 0
    and every destination a new handle or the whole of a set that an earlier step of the program made (what include/msmz.h
    allows there).  A recurrence is in the list with the status the header names for it, MSMZ_ERR_UNSUPPORTED.  After every
    step the runner downloads the range that ends at the block edge and the range that starts at it."""
    rng = random.Random(seed * 104729)
    b = Builder(label, rng)
    n, q = BLOCK + 300, b.q
    d = lambda op, writers, dest: b.dims_of(op, writers, "whole", dest, n)   # noqa: E731
    s1 = b.powers(n)
    s2 = b.name()
    b.emit("scalarsFromBytes", {"n": n, "seed": 77, "windows": [[0, BLOCK], [BLOCK, 300]]}, d("scalarsFromBytes", [], "new"),
           out=s2, m=n, new=True)
    s3 = b.name()
    b.emit("combineScalars", {"n": n, "x": [s1, 0], "a": b.scalar(False), "y": [s1, 0], "b": [s2, 0]}, d("combineScalars", ["scalarPowers"], "new"),
           out=s3, m=n, new=True)
    b.emit("invertScalars", {"n": n, "x": [s3, 0]}, d("invertScalars", ["combineScalars"], "inplace"), out=s3, m=n)
    b.emit("combineScalars", {"n": n, "x": [s1, 0], "a": None, "y": [s3, 0], "b": q - 1}, d("combineScalars", ["scalarPowers"], "inplace"),
           out=s1, m=n)
    rec = {"n": n, "a": [s1, 0], "b": [s3, 0], "init": None, "reverse": False, "exclusive": False, "mode": "general"}
    st = b.emit("scalarRecurrence", rec, d("scalarRecurrence", ["combineScalars"], "new"), out=b.name(), m=n, new=True, refuse="multi-device")
    st["status"] = MSMZ_ERR_UNSUPPORTED
    terms = [[b.scalar(False), [[0, 0], [1, 0]]], [None, [[2, 0], [2, 0], [0, 0]]], [q - 1, [[1, 0]]], [b.scalar(False), []]]
    b.emit("evaluateExpression", {"n": n, "columns": [[s3, 0], [s1, 0], [s2, 0]], "terms": terms},
           dict(d("evaluateExpression", ["invertScalars"], "inplace"), rotated=False), out=s3, m=n)
    b.emit("innerProduct", {"n": n, "x": [s1, 0], "y": [s3, 0]}, d("innerProduct", ["combineScalars"], "-"))
    b.emit("innerProduct", {"n": n, "x": [s3, 0], "y": None}, d("innerProduct", ["evaluateExpression"], "-"))
    b.free(s2)
    s4 = b.name()   # the same size again
    b.emit("scalarsFromBytes", {"n": n, "seed": 78, "windows": [[0, BLOCK], [BLOCK, 300]]}, d("scalarsFromBytes", [], "new"),
           out=s4, m=n, new=True)
    b.emit("combineScalars", {"n": n, "x": [s4, 0], "a": [s3, 0], "y": None, "b": None}, d("combineScalars", ["scalarsFromBytes"], "inplace"),
           out=s4, m=n)
    s5 = b.name()
    b.emit("evaluateExpression", {"n": n, "columns": [[s4, 0], [s1, 0]], "terms": [[None, [[0, 0], [1, 0]]], [2, [[1, 0]]]]},
           dict(d("evaluateExpression", ["combineScalars"], "new"), rotated=False), out=s5, m=n, new=True)
    return {"id": "two-engine", "curve": label, "directed": True, "steps": b.steps, "probes": [(BLOCK - 300, BLOCK), (BLOCK, BLOCK + 300)]}


def cases(seed=1):
    """the programs of the sweep, a pure function of the seed: [{"id", "curve", "directed", "steps"}]"""
    rng = random.Random(seed * 7919)
    by_curve = {label: [] for label in CURVES}
    for c in specs(seed):
        by_curve[c["curve"]].append((c["op"], c["fam"], c["window"], c["dest"], c["size"]))
    programs = []
    for label in CURVES:
        chain = by_curve[label]
        for k in range(0, len(chain), STEPS_PER_PROGRAM):
            programs.append({"curve": label, "directed": False, "steps": _build(label, chain[k:k + STEPS_PER_PROGRAM], rng, 0.35)})
    for d in DIRECTED:
        programs.append({"curve": d["curve"], "directed": True, "steps": _build(d["curve"], d["chain"], rng, 0.0)})
    for k, p in enumerate(programs):
        p["id"] = k
    return programs


# ------------------------------------------------------------------------------------------------ the runner (GPU)
def _lib():
    from msm_zprize_amd._native import lib
    return lib()


class Run:
    """the device side of one program: test-side names -> resident arrays"""

    def __init__(self, curve, label):
        self.curve, self.par, self.label, self.q = curve, curve.Parallel, label, S.order(label)
        self.arr, self.mat = {}, {}

    def handle(self, ref):
        return self.arr[ref[0]].handle

    def raw(self, name, first, n):
        buf = C.create_string_buffer(32 * n)
        assert _lib().msmz_download_scalars(self.curve._ctx, self.arr[name].handle, first, n, buf) == 0
        return buf.raw

    def adopt(self, st, handle):
        from msm_zprize_amd.parallel import DeviceArray
        if st["new"]:
            assert handle not in (0, None)
            self.arr[st["out"]] = DeviceArray(self.curve, handle, st["m"], "scalars")
        else:
            assert handle == self.arr[st["out"]].handle, ("*out_handle changed", st["op"])

    def out_handle(self, st):
        return C.c_uint64(0 if st["new"] else self.arr[st["out"]].handle)

    def call(self, st):
        """-> (status, the scalar results as the model names them)"""
        return getattr(self, "_" + st["op"])(st, st["args"])

    def _source(self, st, arr):
        self.arr[st["out"]] = arr
        return 0, None

    def _scalarsFromBytes(self, st, a):
        return self._source(st, self.par.scalarsFromBytes(S.encode(upload_values(self.label, a)), a["n"]))

    def _scalarsInto(self, st, a):
        from msm_zprize_amd._native import MsmzSrc
        raw = S.encode(upload_values(self.label, a))
        src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
        return _lib().msmz_import_scalars_into(self.curve._ctx, self.arr[st["out"]].handle, st["first_out"], C.byref(src), a["n"]), None

    def _randomScalars(self, st, a):
        return self._source(st, self.par.randomScalars(a["n"], a["seed"]))

    def _scalarPowers(self, st, a):
        return self._source(st, self.par.scalarPowers(a["ratio"], a["n"], a["base"]))

    def _eqTable(self, st, a):
        return self._source(st, self.par.eqTable(a["point"], a["scale"]))

    def _scalarsToBytes(self, st, a):
        return 0, {"bytes": self.par.scalarsToBytes(self.arr[a["x"][0]], a["x"][1], a["n"])}

    def _free(self, st, a):
        (self.mat if a["x"][0] in self.mat else self.arr).pop(a["x"][0]).free()
        return 0, None

    def _term(self, v, c, keep):
        from msm_zprize_amd._native import MsmzScalarTerm
        if isinstance(c, list):
            return MsmzScalarTerm(self.handle(v), v[1], self.handle(c), c[1], None)
        keep.append(_le(c))
        return MsmzScalarTerm(self.handle(v), v[1], 0, 0, keep[-1])

    def _combineScalars(self, st, a):
        keep = []
        x = self._term(a["x"], a["a"], keep)
        y = None if a["y"] is None else self._term(a["y"], a["b"], keep)
        h = self.out_handle(st)
        status = _lib().msmz_scalars_combine(self.curve._ctx, C.byref(x), None if y is None else C.byref(y), a["n"], st["first_out"], C.byref(h))
        return self._finish(st, status, h, None)

    def _finish(self, st, status, h, results):
        if st.get("refuse") or status != 0:
            return status, {"out_handle": h.value}
        self.adopt(st, h.value)
        return status, results

    def _innerProduct(self, st, a):
        y = a["y"]
        return 0, {"value": self.par.innerProduct(self.arr[a["x"][0]], None if y is None else self.arr[y[0]], a["n"], a["x"][1],
                                                 0 if y is None else y[1])}

    def _invertScalars(self, st, a):
        h, zeros = self.out_handle(st), C.c_uint64(1 << 50)
        status = _lib().msmz_scalars_inverse(self.curve._ctx, self.handle(a["x"]), a["x"][1], a["n"], st["first_out"], C.byref(h), C.byref(zeros))
        return self._finish(st, status, h, {"zeros": zeros.value})

    def _evaluateExpression(self, st, a):
        from msm_zprize_amd import _native as N
        cols = (N.MsmzExprColumn * len(a["columns"]))(*[N.MsmzExprColumn(self.handle(c), c[1]) for c in a["columns"]])
        keep = [_le(c) for c, _ in a["terms"]]
        facs = [(N.MsmzExprFactor * max(1, len(fs)))(*[N.MsmzExprFactor(c, r) for c, r in fs]) for _, fs in a["terms"]]
        terms = (N.MsmzExprTerm * len(a["terms"]))(*[N.MsmzExprTerm(k, fa if fs else None, len(fs), 0)
                                                      for (_, fs), fa, k in zip(a["terms"], facs, keep)])
        e = N.MsmzExpr(cols, len(a["columns"]), len(a["terms"]), terms, a["n"], 0)
        h = self.out_handle(st)
        status = _lib().msmz_scalars_expr(self.curve._ctx, C.byref(e), st["first_out"], C.byref(h))
        return self._finish(st, status, h, None)

    def _scalarRecurrence(self, st, a):
        from msm_zprize_amd._native import MsmzScalarRec
        ra, rb = a["a"], a["b"]
        a_res, a_host = (ra, None) if isinstance(ra, list) else (None, _le(ra))
        init = _le(a["init"])
        rec = MsmzScalarRec(self.handle(a_res) if a_res else 0, a_res[1] if a_res else 0, a_host, self.handle(rb) if rb else 0,
                            rb[1] if rb else 0, init, (1 if a["reverse"] else 0) | (2 if a["exclusive"] else 0))
        h, last = self.out_handle(st), C.create_string_buffer(32)
        status = _lib().msmz_scalars_recurrence(self.curve._ctx, C.byref(rec), a["n"], st["first_out"], C.byref(h), last)
        return self._finish(st, status, h, {"last": int.from_bytes(last.raw, "little")})
    _prefixSums = _prefixProducts = _scalarRecurrence

    def _divideByLinear(self, st, a):
        out, last = self.par.divideByLinear(self.arr[a["b"][0]], a["a"], a["n"], a["b"][1])
        self.arr[st["out"]] = out
        return 0, {"last": last}

    def _ntt(self, st, a):
        from msm_zprize_amd._native import MsmzNtt
        shift = _le(a["shift"])
        flags = (1 if a["inverse"] else 0) | (2 if a["shift"] is not None else 0)
        t = MsmzNtt(self.handle(a["x"]), a["x"][1], a["log_n"], flags, a["n_in"], a["count"], None, shift)
        h = self.out_handle(st)
        status = _lib().msmz_scalars_ntt(self.curve._ctx, C.byref(t), st["first_out"], C.byref(h))
        return self._finish(st, status, h, None)

    def _evaluateMle(self, st, a):
        return 0, {"value": self.par.evaluateMle(self.arr[a["x"][0]], a["point"], a["x"][1])}

    def _pairs(self, refs):
        return [(self.arr[name], first) for name, first in refs]

    def _sumcheckRound(self, st, a):
        return 0, {"values": self.par.sumcheckRound(self._pairs(a["tables"]), [tuple(t) for t in a["terms"]], a["n_vars"], a["low"])}

    def _bindMle(self, st, a):
        from msm_zprize_amd._native import MsmzMleBind
        r = _le(a["r"])
        b = MsmzMleBind(self.handle(a["x"]), a["x"][1], a["n_vars"], a["count"], 1 if a["low"] else 0, r)
        h = self.out_handle(st)
        status = _lib().msmz_scalars_mle_bind(self.curve._ctx, C.byref(b), st["first_out"], C.byref(h))
        return self._finish(st, status, h, None)

    def _sumcheckStep(self, st, a):
        from msm_zprize_amd import _native as N
        T, nt = N.MsmzSumcheckTable, len(a["tables"])
        tabs = (T * nt)(*[T(self.handle(t), t[1]) for t in a["tables"]])
        outs = None if a["in_place"] else (T * nt)(*[T(self.handle(o), o[1]) for o in a["outs"]])
        keep = [_le(c) for c, _ in a["terms"]]
        terms = (N.MsmzSumcheckTerm * len(keep))(*[N.MsmzSumcheckTerm(k, mask) for k, (_, mask) in zip(keep, a["terms"])])
        r = _le(a["r"])
        s = N.MsmzSumcheckStep(tabs, outs, nt, a["n_vars"], terms, len(keep), 1 if a["low"] else 0, r)
        size = 32 * (N.MSMZ_SUMCHECK_MAX_DEGREE + 1)
        degree, buf = C.c_uint32(77), C.create_string_buffer(b"\x5a" * size, size)
        status = _lib().msmz_scalars_sumcheck_step(self.curve._ctx, C.byref(s), C.byref(degree), buf)
        if st.get("refuse") or status != 0:   # (no handle to look at: the degree and the bytes are as they were)
            same = degree.value == 77 and buf.raw == b"\x5a" * len(buf.raw)
            return status, {"out_handle": self.arr[st["out"]].handle if same else None}
        d = degree.value
        assert buf.raw[32 * (d + 1):] == b"\x5a" * (len(buf.raw) - 32 * (d + 1)), "bytes beyond degree + 1 values"
        return status, {"degree": d, "values": [int.from_bytes(buf.raw[32 * k:32 * k + 32], "little") for k in range(d + 1)]}

    def _sparseMatrix(self, st, a):
        r = random.Random(a["seed"])
        rows = [r.randrange(a["shape"][0]) for _ in range(a["nnz"])]
        cols = [r.randrange(a["shape"][1]) for _ in range(a["nnz"])]
        v = a["values"]
        self.mat[st["out"]] = self.par.sparseMatrix(rows, cols, None if v is None else self.arr[v[0]], tuple(a["shape"]),
                                                     a["orientations"], 0 if v is None else v[1])
        return 0, None

    def _matVec(self, st, a):
        from msm_zprize_amd._native import MsmzMatvec
        v = MsmzMatvec(self.mat[a["matrix"]].handle, self.handle(a["x"]), a["x"][1], 1 if a["transpose"] else 0)
        h = self.out_handle(st)
        status = _lib().msmz_matrix_mul(self.curve._ctx, C.byref(v), st["first_out"], C.byref(h))
        return self._finish(st, status, h, None)

    def _lookupMultiplicities(self, st, a):
        from msm_zprize_amd import _native as N
        pos = (C.c_uint32 * a["col_n"])(*([0x5a5a5a5a] * a["col_n"])) if a["positions"] else None
        l = N.MsmzLookup(self.handle(a["x"]), a["x"][1], a["n"], self.handle(a["column"]), a["column"][1], a["col_n"], pos, 0)
        res, h = N.MsmzLookupResult(), self.out_handle(st)
        status = _lib().msmz_scalars_lookup(self.curve._ctx, C.byref(l), st["first_out"], C.byref(h), C.byref(res))
        info = {"missing": int(res.n_missing), "distinct": int(res.n_distinct),
                "firstMissing": None if res.first_missing == N.NO_INDEX else int(res.first_missing)}
        return self._finish(st, status, h, {"info": info, "positions": list(pos) if a["positions"] else None})

    def close(self):
        for a in list(self.arr.values()) + list(self.mat.values()):
            a.free()
        self.arr, self.mat = {}, {}


_expected = {}


def expected_of(label, program):
    """the model of a program, computed once and shared by every test that runs it; left unchanged"""
    key = (label, program["id"])
    if key not in _expected:
        _expected[key] = expected(label, program)[:2]
    return _expected[key]


def run_program(curve, program, want=None):
    """every step on `curve`: the status and every returned scalar at once, the written range with GUARD entries on either
    side byte for byte after every step, every live set whole after the last.  -> the bytes of every live set"""
    label = program["curve"]
    per_step, final = want or expected_of(label, program)
    run = Run(curve, label)
    try:
        for k, (st, exp) in enumerate(zip(program["steps"], per_step)):
            where = (program["id"], k, st["op"], st["dims"])
            status, results = run.call(st)
            if st.get("refuse"):
                assert status == st["status"], (where, "status", status)
                assert results["out_handle"] == (0 if st["new"] else run.arr[st["out"]].handle), (where, "*out_handle")
            else:
                assert status == 0, (where, "status", status)
                assert results == exp["results"], (where, results, exp["results"])
            for name, lo, raw in exp["ranges"]:
                got = run.raw(name, lo, len(raw) // 32)
                if got != raw:
                    bad = [lo + i for i in range(len(raw) // 32) if got[32 * i:32 * i + 32] != raw[32 * i:32 * i + 32]]
                    raise AssertionError((where, name, "entries that differ", len(bad), bad[:6], "written", written(st)))
        assert set(run.arr) == set(final), (program["id"], sorted(run.arr), sorted(final))
        got = {name: run.raw(name, 0, len(raw) // 32) for name, raw in final.items()}
        wrong = [name for name in final if got[name] != final[name]]
        assert not wrong, (program["id"], "live sets that differ at the end", wrong)
        return got
    finally:
        run.close()
