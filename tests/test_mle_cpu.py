"""Multilinear polynomials without a GPU: the host-callable part of csrc/mle_kernels.h compiled for the CPU
(tests/native/mle_test.cpp, the same templates the kernels instantiate) against Python integers (tests/mle_util.py) --
one thread's run of eq values, the bind of one pair, the round body of one pair index with the host's coefficient
preparation; the Python argument checks of eqTable / evaluateMle / bindMle / sumcheckRound; the exports and the
behaviour without a device.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import mle_util as M
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "mle_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "mle_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


@pytest.fixture(scope="module")
def driver():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "mle_kernels.h", "scalar_kernels.h", "sqrt.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])

    def run(lines):
        """request lines -> one list of ints per answer line"""
        out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) >= len(lines)
        return [[int(v, 16) for v in line.split()] for line in out[:len(lines)]]

    return run


def _geometry():
    return [int(v) for v in subprocess.run([EXE], input="geometry\n", capture_output=True, text=True, check=True).stdout.split()]


def _points(q, v, rng):
    """points of v variables with r_j over {0, 1, q - 1, random}: all-0/1 points (the table is an indicator), one of
    each constant, and mixtures"""
    pts = [[0] * v, [1] * v, [q - 1] * v, [rng.randrange(2, q) for _ in range(v)],
           [(0, 1)[(j * 5 + 1) % 3 == 0] for j in range(v)],
           [(0, 1, q - 1, rng.randrange(2, q))[j % 4] for j in range(v)]]
    return pts if v else [[]]


@pytest.mark.parametrize("label", S.ALL)
def test_eq_run_small_tables(driver, label):
    """fr_eq_run for v = 0 .. 6 at every run of the table: the whole table == the Python model, for scale over
    {1, 0, q - 1, random}; a 0/1 point gives the indicator of one index exactly"""
    q = S.order(label)
    rng = random.Random(S.ALL.index(label) + 300)
    run = _geometry()[0]
    assert run == 8
    lines, want = [], []
    for v in range(7):
        for point in _points(q, v, rng):
            for scale in (1, 0, q - 1, rng.randrange(2, q)):
                table = M.eq(point, q, scale)
                for g in range(0, 1 << v, run):
                    lines.append(f"{label} eq {v} {g} {scale:x} " + " ".join(f"{r:x}" for r in point))
                    want.append(table[g:g + run])
    got = driver(lines)
    bad = [(line, g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]
    for v in (1, 3, 6):   # the indicator: exactly one entry is the scale
        point = [(13 >> j) & 1 for j in range(v)]
        index = sum(b << j for j, b in enumerate(point))
        assert M.eq(point, q, 7) == [7 if i == index else 0 for i in range(1 << v)]


@pytest.mark.parametrize("label", S.ALL)
def test_eq_run_31_variables(driver, label):
    """a run of a 31-variable table at index 0, 8 (the run after the first: index 1 lies in run 0), 2^31 - 8 and an
    index with alternating bits: every high variable's factor is selected by its index bit, both ways"""
    q = S.order(label)
    rng = random.Random(S.ALL.index(label) + 310)
    v = 31
    alternating = 0x55555555 & ~7 & ((1 << 31) - 1)
    lines, want = [], []
    for point in _points(q, v, rng):
        for g in (0, 8, (1 << 31) - 8, alternating, alternating ^ (((1 << 31) - 1) & ~7)):
            assert g % 8 == 0 and g < 1 << 31
            lines.append(f"{label} eq {v} {g} 1 " + " ".join(f"{r:x}" for r in point))
            want.append([M.eq_at(point, g + k, q) for k in range(8)])
    got = driver(lines)
    bad = [(line[:40], g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]
    assert want[0][:2] == [1, 0] and want[1] == [0] * 8   # the all-zero point: the indicator of index 0 (entries 0 and 1)


@pytest.mark.parametrize("label", S.ALL)
def test_bind_of_one_pair(driver, label):
    """lo + r (hi - lo) over the planted rows (sums of exactly q, q - 1, 0; the carry-chain values) for r over
    {0, 1, q - 1, random}"""
    q = S.order(label)
    rng = random.Random(S.ALL.index(label) + 320)
    rows = S.planted_pairs(q, rng)
    lines, want = [], []
    for r in (0, 1, q - 1, rng.randrange(2, q)):
        for lo, hi in rows:
            lines.append(f"{label} bind {lo:x} {hi:x} {r:x}")
            want.append([(lo + r * (hi - lo)) % q])
    assert driver(lines) == want


@pytest.mark.parametrize("label", S.ALL)
def test_round_body(driver, label):
    """fr_sc_pair over a few pair indices == round_poly, for every table count 1 .. max, the mask sets above and
    coefficients over {NULL, 0, q - 1, random}: terms of different degree in one call come out canonical (the Montgomery
    correction lives in each term's coefficient)"""
    q = S.order(label)
    rng = random.Random(S.ALL.index(label) + 330)
    _, _, _, max_tables, max_degree, _ = _geometry()
    assert (max_tables, max_degree) == (6, 4)
    rows = S.planted_pairs(q, rng)
    lines, want = [], []
    for nt in range(1, max_tables + 1):
        for masks in M.mask_sets(nt, max_degree):
            for coeffs in ([None] * 2, [0, q - 1], [q - 1, rng.randrange(2, q)], [rng.randrange(2, q), None]):
                terms = list(zip(coeffs, masks))
                npairs = 3
                # tables as lists in the LOW order: entry 2i = lo, 2i + 1 = hi
                tables = []
                for j in range(nt):
                    t = []
                    for p in range(npairs):
                        lo, hi = rows[(7 * j + 3 * p + nt) % len(rows)] if (j + p) % 2 else (rng.randrange(q), rng.randrange(q))
                        t += [lo, hi]
                    tables.append(t)
                words = " ".join(f"{tables[j][2 * p]:x} {tables[j][2 * p + 1]:x}" for p in range(npairs) for j in range(nt))
                tw = " ".join(f"{m:x} " + ("-" if c is None else f"{c:x}") for c, m in terms)
                lines.append(f"{label} round {nt} {npairs} {len(terms)} {words} {tw}")
                want.append(M.round_poly(tables, terms, q, low=True))
    got = driver(lines)
    bad = [(line[:60], g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]
    assert any(len(w) == 3 for w in want) and any(len(w) == 5 for w in want) and any(len(w) == 2 for w in want)


def test_model_is_consistent():
    """the Python model against itself: sum eq = 1, evaluation by binding in either order, g(0) + g(1) = the sum, and the
    round of a bound table continues the previous one"""
    q = S.order("pallas")
    rng = random.Random(1)
    v = 4
    point = [rng.randrange(q) for _ in range(v)]
    f = [rng.randrange(q) for _ in range(1 << v)]
    g = [rng.randrange(q) for _ in range(1 << v)]
    assert sum(M.eq(point, q)) % q == 1 and M.eq(point, q)[5] == M.eq_at(point, 5, q)
    lo = list(f)
    for r in point:                      # variable 0 first
        lo = M.bind(lo, r, q, low=True)
    hi = list(f)
    for r in reversed(point):            # the high variable first
        hi = M.bind(hi, r, q)
    assert lo == hi == [M.mle_eval(f, point, q)]
    for low in (False, True):
        evals = M.round_poly([f, g], [(None, 0b11)], q, low)
        assert (evals[0] + evals[1]) % q == sum(a * b for a, b in zip(f, g)) % q
        r = rng.randrange(q)
        nxt = M.round_poly([M.bind(f, r, q, low), M.bind(g, r, q, low)], [(None, 0b11)], q, low)
        assert (nxt[0] + nxt[1]) % q == M.interpolate(evals, r, q)


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=64, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


Q = 1009


def test_eq_table_and_eval_args():
    from msm_zprize_amd.parallel import eq_table_args, mle_eval_args
    a = eq_table_args([3, 5], 1, Q)
    assert a == {"nVars": 2, "point": (3).to_bytes(32, "little") + (5).to_bytes(32, "little"), "scale": None}
    assert eq_table_args([], 7, Q) == {"nVars": 0, "point": b"", "scale": (7).to_bytes(32, "little")}
    assert eq_table_args((0,) * 31, 0, Q)["nVars"] == 31
    for bad in (None, 5, "ab", [1.0], [True], [None], b"\x01"):
        with pytest.raises(TypeError):
            eq_table_args(bad, 1, Q)
    for bad in (None, 1.5, True, b"\x01"):
        with pytest.raises(TypeError):
            eq_table_args([1], bad, Q)
    for point, scale in (([Q], 1), ([-1], 1), ([1, 1 << 256], 1), ([1], Q), ([1], -1), ([0] * 32, 1)):
        with pytest.raises(ValueError):
            eq_table_args(point, scale, Q)
    f = _arr(64)
    assert mle_eval_args(f, [1, 2, 3], 56, Q)["first"] == 56
    assert mle_eval_args(f, [], 63, Q)["nVars"] == 0
    assert mle_eval_args(f, [0] * 6, 0, Q)["nVars"] == 6
    for bad in (None, 7, _arr(64, 2, "points")):
        with pytest.raises(TypeError):
            mle_eval_args(bad, [1], 0, Q)
    with pytest.raises(TypeError):
        mle_eval_args(f, 5, 0, Q)
    for point, first in (([1, 2, 3], 57), ([0] * 7, 0), ([Q], 0), ([1], -1), ([1], True), ([1], 1.0), ([], 64), ([0] * 32, 0)):
        with pytest.raises(ValueError):
            mle_eval_args(f, point, first, Q)


def _bind(f, r=5, nVars=None, count=1, low=False, first=0, out=None, firstOut=0):
    from msm_zprize_amd.parallel import mle_bind_args
    return mle_bind_args(f, r, nVars, count, low, first, out, firstOut, Q)


def test_mle_bind_args():
    f, g = _arr(64, 1), _arr(100, 2)
    a = _bind(f)
    assert (a["nVars"], a["count"], a["flags"], a["N"], a["r"]) == (6, 1, 0, 32, (5).to_bytes(32, "little"))
    assert _bind(f, count=4)["nVars"] == 4 and _bind(f, count=4)["N"] == 32
    assert _bind(f, low=True)["flags"] == 1
    assert _bind(f, nVars=3, first=40, count=3)["N"] == 12
    assert _bind(f, out=f)["firstOut"] == 0                              # in place: the low half
    assert _bind(f, nVars=4, first=16, out=f, firstOut=16)["N"] == 8     # ... of a table inside the array
    assert _bind(f, nVars=4, first=16, out=f, firstOut=8)["N"] == 8      # apart, ending where the source begins
    assert _bind(f, nVars=4, first=16, out=f, firstOut=32)["N"] == 8     # apart, beginning where the source ends
    assert _bind(f, nVars=4, count=2, low=True, out=f, firstOut=32)["N"] == 16
    assert _bind(f, out=g, firstOut=68)["N"] == 32
    for bad in (None, 3, _arr(64, 3, "points")):
        with pytest.raises(TypeError):
            _bind(bad)
    for kw in (dict(r=None), dict(r=1.5), dict(r=True), dict(low=1), dict(out=7), dict(out=_arr(64, 3, "points"))):
        with pytest.raises(TypeError):
            _bind(f, **kw)
    for kw in (dict(r=Q), dict(r=-1), dict(count=0), dict(count=True), dict(count=3),       # 64 is not 3 tables
               dict(nVars=0), dict(nVars=32), dict(nVars=7), dict(nVars=True), dict(nVars=6, first=1), dict(first=-1),
               dict(first=64), dict(first=1), dict(firstOut=1), dict(nVars=31, count=2),      # count 2^v >= 2^32
               dict(nVars=3, count=9), dict(out=g, firstOut=69), dict(out=g, firstOut=-1),
               dict(out=f, firstOut=32),                    # the high half
               dict(out=f, firstOut=1), dict(nVars=4, first=16, out=f, firstOut=9),           # partial overlaps
               dict(nVars=4, first=16, out=f, firstOut=31), dict(nVars=4, first=16, out=f, firstOut=24),
               dict(low=True, out=f), dict(low=True, nVars=4, first=16, out=f, firstOut=16),  # low binding in place
               dict(count=2, out=f), dict(count=2, nVars=4, out=f, firstOut=16)):             # several tables in place
        with pytest.raises(ValueError):
            _bind(f, **kw)
    with pytest.raises(ValueError):
        _bind(_arr(48))            # not a power of two
    with pytest.raises(ValueError):
        _bind(_arr(1))             # a constant has no variable to bind
    same = _arr(64, 1)             # another object for the same handle overlaps all the same
    with pytest.raises(ValueError):
        _bind(f, out=same, firstOut=3)


def _round(tables, terms, nVars=None, low=False):
    from msm_zprize_amd.parallel import sumcheck_round_args
    return sumcheck_round_args(tables, terms, nVars, low, Q)


def test_sumcheck_round_args():
    f, g = _arr(64, 1), _arr(100, 2)
    a = _round([f, (g, 36)], [(None, 0b11), (Q - 1, 0b10)])
    assert a["nVars"] == 6 and a["degree"] == 2 and a["flags"] == 0
    assert a["tables"] == [(f, 0), (g, 36)] and a["terms"] == [(None, 3), ((Q - 1).to_bytes(32, "little"), 2)]
    assert _round([f, f], [(1, 3)], low=True)["flags"] == 1                       # the same table twice: a square
    assert _round([f] * 6, [(None, 0b111100)] * 8, 3)["degree"] == 4
    assert _round([(g, 4)], [(0, 1)], 5)["nVars"] == 5
    for tables, terms in ((None, [(1, 1)]), ([f], None), ([7], [(1, 1)]), ([_arr(64, 3, "points")], [(1, 1)]),
                          ([(f, 0, 0)], [(1, 1)]), ([f], [1]), ([f], [(1, 1, 1)]), ([f], [(1.5, 1)]), ([f], [(True, 1)]),
                          ([f], [(1, None)]), ([f], [(1, 1.0)]), ([f], [(b"\x01", 1)])):
        with pytest.raises(TypeError):
            _round(tables, terms)
    with pytest.raises(TypeError):
        _round([f], [(1, 1)], low=0)
    for tables, terms, nv in (([], [(1, 1)], None), ([f] * 7, [(1, 1)], None), ([f], [], None), ([f], [(1, 1)] * 9, None),
                              ([f], [(1, 0)], None), ([f], [(1, 2)], None), ([f, f], [(1, 4)], None), ([f], [(1, -1)], None),
                              ([f] * 5, [(1, 0b11111)], None),              # five factors
                              ([f], [(Q, 1)], None), ([f], [(-1, 1)], None),
                              ([f], [(1, 1)], 0), ([f], [(1, 1)], 32), ([f], [(1, 1)], 7), ([f], [(1, 1)], True),
                              ([g], [(1, 1)], None),                          # 100 entries: nVars is needed
                              ([f, (g, 37)], [(1, 3)], None), ([(f, 1)], [(1, 1)], 6), ([(f, -1)], [(1, 1)], 2),
                              ([(f, 64)], [(1, 1)], 1)):
        with pytest.raises(ValueError):
            _round(tables, terms, nv)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


NAMES = ("msmz_scalars_eq_table", "msmz_scalars_mle_eval", "msmz_scalars_mle_bind", "msmz_scalars_sumcheck_round",
         "msmz_test_mle_geometry")


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in NAMES:
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    assert C.sizeof(_native.MsmzMleBind) == 40 and C.sizeof(_native.MsmzSumcheck) == 32
    assert C.sizeof(_native.MsmzSumcheckTable) == 16 and C.sizeof(_native.MsmzSumcheckTerm) == 16
    assert (_native.MSMZ_SUMCHECK_MAX_TABLES, _native.MSMZ_SUMCHECK_MAX_DEGREE, _native.MSMZ_SUMCHECK_MAX_TERMS) == (6, 4, 8)
    header = open(os.path.join(ROOT, "include", "msmz.h")).read()
    assert "MSMZ_SUMCHECK_MAX_TABLES = 6, MSMZ_SUMCHECK_MAX_DEGREE = 4, MSMZ_SUMCHECK_MAX_TERMS = 8" in header


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof and the offsets of every field of the three descriptors, C side == ctypes side"""
    from msm_zprize_amd import _native as N
    src = tmp_path / "layout.c"
    fields = [("msmz_mle_bind", N.MsmzMleBind), ("msmz_sumcheck_table", N.MsmzSumcheckTable),
              ("msmz_sumcheck_term", N.MsmzSumcheckTerm), ("msmz_sumcheck", N.MsmzSumcheck)]
    prints, want = [], []
    for cname, T in fields:
        prints.append(f'printf("%zu ", sizeof({cname}));')
        want.append(C.sizeof(T))
        for fname, _ in T._fields_:
            prints.append(f'printf("%zu ", offsetof({cname}, {fname}));')
            want.append(getattr(T, fname).offset)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msmz.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()] == want


def test_geometry_accessor(lib, driver):
    """msmz_test_mle_geometry == the constants the host driver was compiled with; needs no context"""
    r, e, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lib.msmz_test_mle_geometry(C.byref(r), C.byref(e), C.byref(p))
    assert [r.value, e.value, p.value] == _geometry()[:3]
    assert e.value % r.value == 0 and e.value & (e.value - 1) == 0 and p.value & (p.value - 1) == 0
    lib.msmz_test_mle_geometry(None, None, None)


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG and the outputs untouched, for all four entry points"""
    from msm_zprize_amd import _native as N
    one = (1).to_bytes(32, "little")
    h = C.c_uint64(0)
    assert lib.msmz_scalars_eq_table(None, one, 1, None, C.byref(h)) == 1 and h.value == 0
    out = C.create_string_buffer(b"\xaa" * 32, 32)
    assert lib.msmz_scalars_mle_eval(None, 1, 0, 1, one, out) == 1 and out.raw == b"\xaa" * 32
    b = N.MsmzMleBind(1, 0, 1, 1, 0, one)
    h = C.c_uint64(77)
    assert lib.msmz_scalars_mle_bind(None, C.byref(b), 0, C.byref(h)) == 1 and h.value == 77
    tabs = (N.MsmzSumcheckTable * 1)(N.MsmzSumcheckTable(1, 0))
    terms = (N.MsmzSumcheckTerm * 1)(N.MsmzSumcheckTerm(None, 1))
    s = N.MsmzSumcheck(tabs, 1, 1, terms, 1, 0)
    d = C.c_uint32(9)
    ev = C.create_string_buffer(b"\xaa" * 160, 160)
    assert lib.msmz_scalars_sumcheck_round(None, C.byref(s), C.byref(d), ev) == 1
    assert d.value == 9 and ev.raw == b"\xaa" * 160
