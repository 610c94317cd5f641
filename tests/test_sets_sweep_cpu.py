"""The program list of the resident-set sweep (tests/sets_sweep_util.py), without a GPU: (a) the list holds every target
its rule table allows, (b) nothing is dropped without a named rule and the list does not shrink, (c) refusals stay a small
share, (d) every family and every operation is both a producer and a consumer, (e) the model, on three programs small
enough to work out by hand, equals plain modular arithmetic written out here."""
import collections

import pytest

import sets_sweep_util as U
from oracle import params as P

SEED = 1
N_PROGRAMS, N_STEPS = 50, 1384   # cases(1): 45 programs of the covering and 5 directed ones; every step, refusals included


@pytest.fixture(scope="module")
def programs():
    import msm_zprize_amd.build as b
    b.build(verbose=False)   # (the sizes come from the library's geometry hooks; they need no GPU)
    return U.cases(SEED)


def _steps(programs):
    return [s for p in programs for s in p["steps"]]


def test_programs_are_a_pure_function_of_the_seed(programs):
    assert U.cases(SEED) == programs
    assert U.cases(SEED + 1) != programs
    assert [p["id"] for p in programs] == list(range(len(programs)))


def test_a_every_target_is_reached(programs):
    held = set()
    for s in _steps(programs):
        held.update(U._holds(s))
    allowed = [t for t, why in U.targets().items() if why is None]
    missing = [t for t in allowed if t not in held]
    assert not missing, missing[:10]
    # the dimensions: 23 operations, 9 families and none, 3 windows and none, 4 destination kinds, 4 curves; the sizes are
    # 1, 2, three kernels' edges +- 1, the tile - 1 / exactly / + 1, and 2^0 .. 2^(pass limit + 1)
    D = U.dims()
    assert [len(D[k]) for k in ("op", "fam", "window", "dest", "curve")] == [23, 10, 4, 4, 4]
    any_n, pow2 = U.size_classes()
    g = U.geometry()
    assert {1, 2, U.WAVE - 1, U.WAVE + 1, g["workgroup"] - 1, g["workgroup"] + 1, g["inv_chunk"] - 1, g["inv_chunk"] + 1} <= set(any_n.values())
    for t in (g["dot_tile"], g["rec_tile"], g["mle_tile"]):
        assert {t - 1, t, t + 1} <= set(any_n.values())
    assert sorted(pow2.values()) == [1 << k for k in range(g["pass_log"] + 2)]
    assert len(allowed) > 600


def test_b_no_silent_shrinkage(programs):
    names = {name for name, _, _, _ in U.RULES}
    for name, fields, cite, _ in U.RULES:
        assert cite and set(fields) <= set(U.dims()), name
    dropped = {t: why for t, why in U.targets().items() if why is not None}
    assert dropped and all(why in names for why in dropped.values())
    # a rule that forbids nothing would hide a typo; "two-adicity" reads three dimensions that no target lists together: it
    # steers complete(), and is held against the generated steps at the end of this test
    assert set(dropped.values()) == names - {"two-adicity"}
    assert U.violated({"op": "ntt", "size": "2^2", "curve": U.TE}) == "two-adicity"
    assert U.violated({"op": "ntt", "size": "2^1", "curve": U.TE}) is None
    assert (len(programs), len(_steps(programs))) == (N_PROGRAMS, N_STEPS)
    # every set within two tiles plus one; every valid step valid by construction: the model runs it without a skip
    for p in programs:
        per_step, final, _ = U.expected(p["curve"], p)
        assert len(per_step) == len(p["steps"])
        assert all(len(raw) // 32 <= U.max_set() for raw in final.values())
    assert max(s["m"] for s in _steps(programs)) <= U.max_set()
    # the two-adicity rule holds in what was generated, not only in the table
    for p in programs:
        for s in p["steps"]:
            assert not (s["op"] == "ntt" and p["curve"] == U.TE and s["args"]["log_n"] > 1)


def test_b_valid_by_construction_for_other_seeds():
    """the model asserts the destination rules of include/msmz.h on every valid step it runs (Model.destination_rules,
    and the rules of sumcheckStep in its own function): they hold for other seeds' programs too, not by the luck of one"""
    for seed in (2, 3):
        for p in U.cases(seed):
            per_step, _, _ = U.expected(p["curve"], p)
            assert len(per_step) == len(p["steps"])


def test_b_every_variant_of_every_operation(programs):
    """what a step draws beyond its dimensions, each present for seed 1"""
    valid = [s for s in _steps(programs) if not s.get("refuse")]
    of = lambda *ops: [s["args"] for s in valid if s["op"] in ops]   # noqa: E731
    comb = of("combineScalars")
    assert any(a["y"] is None for a in comb) and any(a["y"] is not None for a in comb)
    for key in ("a", "b"):
        used = [a[key] for a in comb if key == "a" or a["y"] is not None]
        assert any(c is None for c in used) and any(isinstance(c, int) for c in used) and any(isinstance(c, list) for c in used), key
    rec = of("scalarRecurrence")
    assert {a["mode"] for a in rec} == {m[0] for m in U.SC.MODES}
    for key in ("reverse", "exclusive"):
        assert {a[key] for a in rec} == {False, True}, key
    assert any(a["init"] is None for a in rec) and any(a["init"] is not None for a in rec)
    assert of("prefixSums") and of("prefixProducts") and of("divideByLinear")
    ntt = of("ntt")
    assert {a["inverse"] for a in ntt} == {False, True} and {a["shift"] is None for a in ntt} == {False, True}
    assert any(a["n_in"] < 1 << a["log_n"] for a in ntt) and {1, 2, 3} <= {a["count"] for a in ntt}
    bind = of("bindMle")
    assert {a["low"] for a in bind} == {False, True} and any(a["count"] > 1 for a in bind)
    step = of("sumcheckStep")
    assert {len(a["tables"]) for a in step} == set(range(1, 7)) and {a["low"] for a in step} == {False, True}
    assert {a["in_place"] for a in step} == {False, True}
    assert {len(a["tables"]) for a in of("sumcheckRound")} == set(range(1, 7))
    assert {a["y"] is None for a in of("innerProduct")} == {False, True}
    mv = of("matVec")
    assert {a["transpose"] for a in mv} == {False, True}
    mats = of("sparseMatrix")
    assert {a["values"] is None for a in mats} == {False, True} and {a["orientations"] for a in mats} == {"rows", "cols", "both"}
    assert {a["positions"] for a in of("lookupMultiplicities")} == {False, True}
    expr = [s for s in valid if s["op"] == "evaluateExpression"]
    assert {s["dims"]["rotated"] for s in expr} == {False, True}
    assert any(s["dims"]["dest"] == "inplace" for s in expr)
    # every matrix a covering step builds is multiplied before it is freed: the step that holds the target is checked
    for p in programs:
        steps = p["steps"]
        for k, s in enumerate(steps):
            if s["op"] == "sparseMatrix":
                after = [t for t in steps[k + 1:] if t["op"] in ("matVec", "free") and (t["args"].get("matrix") == s["out"] or t["args"].get("x", [None])[0] == s["out"])]
                assert after and after[0]["op"] == "matVec" and not after[0].get("refuse") or \
                    (len(after) > 1 and after[1]["op"] == "matVec" and not after[1].get("refuse")), (p["id"], k)


def test_c_refusals_are_at_most_one_step_in_ten(programs):
    steps = _steps(programs)
    refused = [s for s in steps if s.get("refuse")]
    assert 0 < len(refused) <= len(steps) // 10
    kinds = collections.Counter(s["refuse"] for s in refused)
    assert set(kinds) == {"partial-overlap", "beyond-the-set", "high-half", "on-the-gathered-operand", "on-a-rotated-column",
                          "low-in-place"}
    assert all(s["status"] == U.MSMZ_ERR_ARG and not s["new"] for s in refused)
    # a refusal is followed by the valid call it was made from (a fresh destination may be uploaded in between)
    for p in programs:
        for k, s in enumerate(p["steps"]):
            if s.get("refuse"):
                after = next(t for t in p["steps"][k + 1:] if t["op"] != "scalarsFromBytes")
                assert after["op"] == s["op"] and not after.get("refuse")
                assert after["args"] == s["args"] or s["refuse"] in ("on-a-rotated-column", "low-in-place")


def test_d_producers_and_consumers(programs):
    """every family, and every operation that writes a set, wrote entries that a later step's first operand reads; every
    operation that reads a set read some.  (innerProduct, evaluateMle, sumcheckRound, scalarsToBytes and free write no
    set; the five sources read none.)"""
    valid = [s for s in _steps(programs) if not s.get("refuse")]
    producers = {w for s in valid for w in s["dims"]["producers"]}
    consumers = {s["op"] for s in valid if s["dims"]["producers"]}
    writes = {op for op, (_, _, dests, _) in U.OPS.items() if dests != ["-"]}
    reads = {op for op, (_, reads, _, _) in U.OPS.items() if reads}
    assert producers == writes, (writes - producers, producers - writes)
    assert consumers == reads, reads - consumers
    assert {U.OPS[w][0] for w in producers} == set(U.FAMILIES)
    assert {f for s in valid for f in s["dims"]["fams"]} == set(U.FAMILIES)
    # free and re-allocation of equal size inside one program
    again = 0
    for p in programs:
        freed, live = collections.Counter(), {}
        for s in p["steps"]:
            if s.get("refuse"):
                continue
            if s["op"] == "free":
                freed[live.pop(s["args"]["x"][0], None)] += 1
            elif s["new"] and s["op"] != "sparseMatrix":
                again += 1 if freed[s["m"]] else 0
                live[s["out"]] = s["m"]
    assert again >= 20, again


# ---------------------------------------------------------------------------------------------- (e) the model by hand
def _step(op, args, out=None, first_out=0, m=0, new=False):
    return {"op": op, "args": args, "out": out, "first_out": first_out, "m": m, "new": new, "dims": {}}


def _upload(name, values):
    return _step("scalarsFromBytes", {"n": len(values), "values": values}, out=name, m=len(values), new=True)


def _run(label, steps):
    per_step, _, model = U.expected(label, {"id": "hand", "curve": label, "steps": steps})
    return [s["results"] for s in per_step], model.sets


@pytest.mark.parametrize("label", U.CURVES)
def test_e_combine_inverse_dot_by_hand(label):
    """s = [3, 5, 7, 11, q - 1]; s[2..4) = 2 s[1..3) + s[0..2) (a destination that partly meets neither: x is [1, 3), the
    destination [2, 4) -- so the model must read before it writes); then s[0..2) inverted in place; then <s[0..3), s[2..5)>"""
    q = P.CURVES[label]["order"]
    steps = [_upload("s", [3, 5, 7, 11, q - 1]),
             _step("combineScalars", {"n": 2, "x": ["s", 1], "a": 2, "y": ["s", 0], "b": None}, out="t", m=2, new=True),
             _step("combineScalars", {"n": 2, "x": ["t", 0], "a": None, "y": None, "b": None}, out="s", first_out=2, m=2),
             _step("invertScalars", {"n": 2, "x": ["s", 0]}, out="s", first_out=0, m=2),
             _step("innerProduct", {"n": 3, "x": ["s", 0], "y": ["s", 2]})]
    results, sets = _run(label, steps)
    third, fifth = pow(3, -1, q), pow(5, -1, q)
    assert sets["t"] == [2 * 5 + 3, 2 * 7 + 5]
    assert sets["s"] == [third, fifth, 13, 19, q - 1]
    assert results[3] == {"zeros": 0}
    assert results[4] == {"value": (third * 13 + fifth * 19 + 13 * (q - 1)) % q}


@pytest.mark.parametrize("label", U.CURVES)
def test_e_transform_bind_scan_by_hand(label):
    """the transform of length 2 is (a + b, a - b) on every curve (the root is q - 1); binding [u, v] to r gives
    u + r (v - u); the exclusive prefix sums of [x, y, z] from 10 are [10, 10 + x, 10 + x + y] and the last value is the
    full sum"""
    q = P.CURVES[label]["order"]
    a, b, r = 9, 4, 6
    steps = [_upload("s", [1, a, b, 1]),
             _step("ntt", {"log_n": 1, "x": ["s", 1], "n_in": 2, "count": 1, "inverse": False, "shift": None}, out="s", first_out=1, m=2),
             _step("bindMle", {"x": ["s", 0], "n_vars": 2, "count": 1, "low": False, "r": r}, out="s", first_out=0, m=2),
             _step("prefixSums", {"n": 3, "a": None, "b": ["s", 1], "init": 10, "reverse": False, "exclusive": True, "mode": "sums"},
                   out="p", m=3, new=True),
             _step("ntt", {"log_n": 1, "x": ["p", 0], "n_in": 1, "count": 1, "inverse": False, "shift": 3}, out="c", m=2, new=True)]
    results, sets = _run(label, steps)
    f = [1, a + b, a - b, 1]                       # after the transform
    bound = [(f[0] + r * (f[2] - f[0])) % q, (f[1] + r * (f[3] - f[1])) % q]
    assert sets["s"] == bound + [a - b, 1]
    x, y, z = bound[1], a - b, 1
    assert sets["p"] == [10, (10 + x) % q, (10 + x + y) % q] and results[3] == {"last": (10 + x + y + z) % q}
    assert sets["c"] == [10, 10]                   # one coefficient, zero-padded: the constant polynomial on the coset


@pytest.mark.parametrize("label", U.CURVES)
def test_e_lookup_matvec_expression_by_hand(label):
    """table [7, 8, 7], column [8, 7, 7, 5]: multiplicities [2, 1, 0], positions [1, 0, 0, none], one missing at 3; a 2 x 3
    matrix against them; out_i = 2 x_i x_(i+1) - x_(i-1), cyclic; host bytes over the middle; a download; a free"""
    q = P.CURVES[label]["order"]
    steps = [_upload("t", [7, 8, 7, 8, 7, 7, 5]),
             _step("lookupMultiplicities", {"n": 3, "x": ["t", 0], "column": ["t", 3], "col_n": 4, "positions": True},
                   out="m", m=3, new=True),
             _step("evaluateExpression", {"n": 3, "columns": [["m", 0]], "terms": [[2, [[0, 0], [0, 1]]], [q - 1, [[0, -1]]]]},
                   out="e", m=3, new=True),
             _step("scalarsInto", {"n": 1, "values": [4]}, out="e", first_out=1, m=1),
             _step("scalarsToBytes", {"x": ["e", 1], "n": 2}),
             _step("free", {"x": ["t", 0]})]
    results, sets = _run(label, steps)
    assert sets["m"] == [2, 1, 0]
    assert results[1] == {"info": {"missing": 1, "firstMissing": 3, "distinct": 2}, "positions": [1, 0, 0, 0xffffffff]}
    e = [(2 * 2 * 1 - 0) % q, (2 * 1 * 0 - 2) % q, (2 * 0 * 2 - 1) % q]
    assert sets["e"] == [e[0], 4, e[2]]
    assert results[4] == {"bytes": (4).to_bytes(32, "little") + e[2].to_bytes(32, "little")}
    assert "t" not in sets
    # the matrix of the model: triples from the step's seed, the product by the definition
    mat = _step("sparseMatrix", {"values": ["e", 0], "nnz": 3, "shape": [2, 3], "orientations": "rows", "seed": 5}, out="M", new=True)
    mv = _step("matVec", {"matrix": "M", "x": ["m", 0], "transpose": False}, out="y", m=2, new=True)
    _, model = U.expected(label, {"id": "hand", "curve": label, "steps": steps + [mat, mv]})[1:]
    rows, cols, vals, shape, _ = model.mats["M"]
    assert vals == sets["e"] and shape == [2, 3]
    want = [0, 0]
    for i, j, v in zip(rows, cols, vals):
        want[i] = (want[i] + v * [2, 1, 0][j]) % q
    assert model.sets["y"] == want
