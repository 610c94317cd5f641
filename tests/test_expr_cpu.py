"""Gate expressions without a GPU: the host/device half of csrc/expr_kernels.h compiled for the CPU
(tests/native/expr_test.cpp, the same templates the kernels instantiate) against Python integers (tests/expr_util.py)
-- the body of one entry in both of its forms, the index function up to n = 2^32 - 1, the compile step with its
deduplication, limits and refusals, and the overlap rule as a table; then the descriptor layouts, the exports, null
arguments, the Python argument checks and the behaviour without a device.  The driver is also built with the address
and undefined-behaviour sanitizers as a stand-alone program and run over the same requests.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import expr_util as E
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "expr_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "expr_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "expr_kernels.h", "mle_kernels.h", "scalar_kernels.h", "ranges.h", "fp.h",
                                                "constants_gen.h")]
OK, ERR_ARG, ERR_RANGE = 0, 1, 6


def _build(exe, extra=()):
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, "-o", exe, SRC])


def _ask(exe, lines):
    """request lines -> the answer lines, as lists of words"""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(lines)
    return [line.split() for line in out[:len(lines)]]


@pytest.fixture(scope="module")
def driver():
    _build(EXE)
    return lambda lines: _ask(EXE, lines)


@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def _hex(values):
    return " ".join(f"{v:x}" for v in values)


def _desc(n, n_columns, terms, flags=0, cols="ok", trms="ok", n_terms=None, reserved=None, factors=None, n_factors=None):
    """DESC of the driver.  reserved / factors / n_factors: {term index: value} overrides of what the terms give"""
    words = [n, n_columns, flags, cols, trms, len(terms) if n_terms is None else n_terms]
    for k, (c, fs) in enumerate(terms[:words[-1]]):
        fs = [E.factor(f) for f in fs]
        nf = (n_factors or {}).get(k, len(fs))
        ptr = (factors or {}).get(k, "ok")
        words += ["-" if c is None else f"{c:x}", (reserved or {}).get(k, 0), nf, ptr]
        if ptr == "ok":
            assert nf == len(fs)
            words += [w for f in fs for w in f]
    return " ".join(str(w) for w in words)


# ------------------------------------------------------------------------------------------------ the body of one entry
def _eval_lines(label, slots, n, n_columns, terms, columns):
    return f"{label} eval {slots} {_desc(n, n_columns, terms)} {_hex(v for col in columns for v in col[:n])}"


def _parse_eval(words, n):
    assert len(words) == n + 1, words[:3]
    return [int(w, 16) for w in words[:n]], int(words[n])


@pytest.mark.parametrize("label", S.ALL)
def test_entry_body_gives_the_model(driver, label):
    """every term set of expr_util (coefficients None, 0, 1, q - 1 and random, degrees 0 .. 8, a^8, the same column at
    three rotations, mixed degrees, 1 to 32 operands) over columns of {0, 1, q - 1, random} at n = 1, 2, 3, 5 and 33"""
    q = S.order(label)
    cases = []
    for n in (1, 2, 3, 5, 33):
        rng = random.Random(n + 10 * S.ALL.index(label))
        for name, (nc, terms) in E.term_sets(q, n, seed=n).items():
            cases.append((name, n, nc, terms, E.edge_columns(nc, n, q, rng)))
    got = driver([_eval_lines(label, 0, n, nc, terms, cols) for _, n, nc, terms, cols in cases])
    for (name, n, nc, terms, cols), words in zip(cases, got):
        assert _parse_eval(words, n) == (E.model(cols, terms, n, q), 0), (name, n)
    assert any(name == "operands_32" for name, *_ in cases)


@pytest.mark.parametrize("label", S.ALL)
def test_register_resident_body_gives_the_same_values(driver, label):
    """fr_expr_entry_slots<2 | 4 | 8> on every term set that fits its slots == fr_expr_entry == the model; a set with
    one operand too many is refused by the driver, so the slot counts tested are the real edges"""
    q = S.order(label)
    n = 7
    rng = random.Random(99 + S.ALL.index(label))
    sets = E.term_sets(q, n, seed=3)
    ran = {2: 0, 4: 0, 8: 0}
    for name, (nc, terms) in sets.items():
        cols = E.edge_columns(nc, n, q, rng)
        n_ops = len(E.operands(terms, n))
        want = (E.model(cols, terms, n, q), 0)
        for slots, words in zip((2, 4, 8), driver([_eval_lines(label, s, n, nc, terms, cols) for s in (2, 4, 8)])):
            if n_ops <= slots:
                assert _parse_eval(words, n) == want, (name, slots)
                ran[slots] += 1
            else:
                assert words == ["status", "-1"], (name, slots)
    assert len(E.operands(sets["operands_8"][1], n)) == 8 and len(E.operands(sets["operands_9"][1], n)) == 9
    assert len(E.operands(sets["operands_4"][1], n)) == 4 and len(E.operands(sets["operands_5"][1], n)) == 5
    assert ran[2] >= 5 and ran[4] > ran[2] and ran[8] > ran[4]


@pytest.mark.parametrize("label", S.ALL)
def test_records_not_below_q_are_flagged_only_where_read(driver, label):
    """q and 2^256 - 1 in a named column raise the flag in both bodies; in a column no factor names they do not"""
    q = S.order(label)
    terms = [(3, [0, (0, 1)]), (None, [])]
    lines, want = [], []
    for bad in (q, (1 << 256) - 1):
        for slots in (0, 2):
            lines += [_eval_lines(label, slots, 3, 2, terms, [[5, bad, 7], [1, 2, 3]]),
                      _eval_lines(label, slots, 3, 2, terms, [[5, 6, 7], [1, bad, 3]])]
            want += [1, 0]
    got = driver(lines)
    assert [int(w[-1]) for w in got] == want
    assert _parse_eval(got[1], 3)[0] == E.model([[5, 6, 7]], terms, 3, q)


# ------------------------------------------------------------------------------------------------ the index function
def test_index_function_up_to_2_32_minus_1(driver):
    """n in {1, 2, 3, 64, 2^31, 2^32 - 1} x rot in {0, +-1, n - 1, n, -n, n + 1, 2^31 - 1, -2^31} x i in {0, 1, n - 2,
    n - 1}: (i + rot) mod n as Python computes it, with rot reduced from any int32"""
    cases = []
    for n in (1, 2, 3, 64, 1 << 31, (1 << 32) - 1):
        rots = {0, 1, -1, n - 1, n, -n, n + 1, E.INT32_MAX, E.INT32_MIN}
        for rot in sorted(r for r in rots if E.INT32_MIN <= r <= E.INT32_MAX):
            for i in sorted(i for i in {0, 1, n - 2, n - 1} if 0 <= i < n):
                cases.append((i, rot, n))
    got = driver([f"index {i} {rot} {n}" for i, rot, n in cases])
    for (i, rot, n), words in zip(cases, got):
        assert int(words[0]) == E.index(i, rot, n), (i, rot, n)
    assert len(cases) > 100 and any(i + rot % n >= 1 << 32 for i, rot, n in cases)   # a 32-bit sum would have wrapped


# ------------------------------------------------------------------------------------------------ the compile step
def _compile(driver, label, *descs):
    return driver([f"{label} compile {d}" for d in descs])


def test_compile_deduplicates_operands(driver):
    """(col, rot) and (col, rot + n) and (col, rot - n) are one operand; operands are numbered in first-use order; a
    term keeps one index per factor, a repeated factor as often as it occurs; named[] tells unread, unrotated, rotated"""
    n = 5
    terms = [(2, [(0, 1), (0, 6), (0, -4), 1]), (None, [1, (1, 5), (2, 0)]), (7, []), (1, [(0, 1)] * 8)]
    words = _compile(driver, "pallas", _desc(n, 4, terms))[0]
    assert words[:4] == ["0", "0", "3", "1"]
    assert words[4:7] == ["0:1", "1:0", "2:0"]
    assert words[7:11] == ["0,0,0,1", "1,1,2", "-", "0,0,0,0,0,0,0,0"]
    assert words[11:15] == ["3", "1", "1", "0"]
    assert [tuple(int(x) for x in w.split(":")) for w in words[4:7]] == E.operands(terms, n)
    unrot = _compile(driver, "pallas", _desc(n, 2, [(None, [(0, 5), (1, -10)])]))[0]
    assert unrot[:4] == ["0", "0", "2", "0"] and unrot[-3:-1] == ["1", "1"]


@pytest.mark.parametrize("label", S.ALL)
def test_compile_prepares_the_coefficients(driver, label):
    """coefficient k comes out as c 2^(256 f) mod q, f the factors of the term; NULL is 1"""
    q = S.order(label)
    rng = random.Random(8)
    terms = [(c, [0] * f) for f, c in enumerate([None, 0, 1, q - 1] + [rng.randrange(q) for _ in range(5)])]
    words = _compile(driver, label, _desc(4, 1, terms))[0]
    got = [int(w, 16) for w in words[-len(terms):]]
    assert got == [(1 if c is None else c) * pow(2, 256 * len(fs), q) % q for c, fs in terms]


def test_compile_accepts_32_operands_and_refuses_33(driver):
    n = 64
    pairs = [(k % 2, k // 2) for k in range(33)]
    t32 = [(None, pairs[8 * t:8 * t + 8]) for t in range(4)]
    ok, again, bad, wrapped = _compile(driver, "bls12-377", _desc(n, 2, t32), _desc(n, 2, t32 + [(None, pairs[:8])]),
                                       _desc(n, 2, t32 + [(None, [pairs[32]])]), _desc(n, 2, t32 + [(None, [(0, 16 - n)])]))
    assert ok[:3] == ["0", "0", "32"] and again[:3] == ["0", "0", "32"]
    assert bad == ["1", "-"]
    assert wrapped == ["1", "-"]   # (0, 16 - n) is (0, 16): the 33rd pair all the same


def test_compile_refuses_in_the_documented_order(driver):
    """every MSMZ_ERR_ARG of the compile step, each alone and then together with a coefficient >= q, which must lose:
    MSMZ_ERR_RANGE is reported only once nothing else is wrong"""
    q = S.order("bls12-377")
    good = [(5, [0, (1, 1)]), (None, [1])]
    big = [(q, [0, (1, 1)]), (None, [1])]
    nine = [0] * 9
    many = [(None, [0])] * 33

    def cases(terms):
        return [
            _desc(8, 2, terms, cols="null"), _desc(8, 2, terms, trms="null"),
            _desc(8, 0, terms), _desc(8, 17, terms), _desc(8, 2, terms, n_terms=0), _desc(8, 2, many),
            _desc(0, 2, terms), _desc(1 << 32, 2, terms), _desc(8, 2, terms, flags=1), _desc(8, 2, terms, flags=1 << 31),
            _desc(8, 2, terms, reserved={1: 1}), _desc(8, 2, terms + [(None, nine)]),
            _desc(8, 2, terms, factors={1: "null"}), _desc(8, 2, terms + [(None, [2])]), _desc(8, 2, terms + [(None, [(1 << 32) - 1])]),
        ]
    for words in _compile(driver, "bls12-377", *cases(good), *cases(big)):
        assert words == [str(ERR_ARG), "-"]
    accepted = _compile(driver, "bls12-377", _desc(8, 2, good), _desc((1 << 32) - 1, 16, good), _desc(8, 2, good + [(None, [0] * 8)]),
                        _desc(8, 2, [(None, [])], factors={0: "null"}, n_factors={0: 0}), _desc(8, 2, [(None, [0])] * 32))
    assert [w[:2] for w in accepted] == [["0", "0"]] * 5
    for bad in (q, q + 1, (1 << 256) - 1):
        assert _compile(driver, "bls12-377", _desc(8, 2, [(1, [0]), (bad, [])]))[0] == ["0", str(ERR_RANGE)]
    assert _compile(driver, "bls12-377", _desc(8, 2, [(q - 1, [0])]))[0][:2] == ["0", "0"]


# ------------------------------------------------------------------------------------------------ the overlap rule
def test_overlap_rule_as_a_table(driver):
    """(how the column is read, column first, destination first, n) -> allowed?  unrotated: the exact range or apart;
    rotated: apart; unnamed: anything"""
    n = 8
    table = []
    for first_out in (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 100):
        d = abs(first_out - 16)
        table += [((0, 16, first_out, n), True), ((1, 16, first_out, n), d == 0 or d >= n), ((3, 16, first_out, n), d >= n)]
    table += [((1, 0, 0, 1), True), ((3, 0, 0, 1), False), ((1, 0, 1, 1), True), ((3, 0, 1, 1), True), ((3, 1, 0, 1), True),
              ((1, (1 << 64) - 9, (1 << 64) - 8, n), False), ((3, (1 << 64) - 8, 0, n), True), ((1, 5, 5, (1 << 32) - 1), True),
              ((1, 5, 6, (1 << 32) - 1), False), ((3, 5, 5 + (1 << 32) - 1, (1 << 32) - 1), True), ((3, 5, 4 + (1 << 32) - 1, (1 << 32) - 1), False)]
    got = driver(["overlap " + " ".join(str(v) for v in args) for args, _ in table])
    assert [w[0] for w in got] == ["1" if ok else "0" for _, ok in table]
    assert {ok for (named, *_), ok in table if named == 1} == {True, False}


def test_sanitized_driver_runs_clean():
    """expr_test.cpp as a stand-alone program with -fsanitize=address,undefined over requests of every kind, the
    refusals included: exit 0, nothing on stderr, the same answers"""
    _build(EXE)
    exe = EXE + "_asan"
    _build(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    label, q = "bls12-377", S.order("bls12-377")
    rng = random.Random(4)
    lines = ["geometry", f"index {(1 << 32) - 2} {E.INT32_MIN} {(1 << 32) - 1}", f"index 0 -1 {1 << 31}", "index 0 5 1",
             "overlap 3 16 9 8", "overlap 1 16 16 8",
             f"{label} compile {_desc(8, 2, [(q, [0])])}", f"{label} compile {_desc(8, 2, [(1, [2])])}",
             f"{label} compile {_desc(8, 2, [(1, [0])], cols='null')}", f"{label} compile {_desc(8, 2, [(1, [0])], factors={0: 'null'})}",
             f"{label} compile {_desc(64, 2, [(None, [(k % 2, k // 2) for k in range(8 * t, 8 * t + 8)]) for t in range(4)] + [(None, [(0, 40)])])}"]
    for n in (1, 3, 33):
        for name, (nc, terms) in E.term_sets(q, n, seed=n).items():
            cols = E.edge_columns(nc, n, q, rng)
            lines.append(_eval_lines(label, 0, n, nc, terms, cols))
            lines.append(_eval_lines(label, 8, n, nc, terms, cols))
    lines.append(_eval_lines(label, 0, 3, 1, [(None, [0])], [[5, q, (1 << 256) - 1]]))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=64, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


def _args(columns, terms, N=None, out=None, firstOut=0, label="bls12-377"):
    from msm_zprize_amd.parallel import expr_args
    return expr_args(columns, terms, N, out, firstOut, S.order(label))


def test_expr_args():
    q = S.order("bls12-377")
    a, b, o = _arr(64, 1), _arr(64, 2), _arr(100, 3)
    t = _args([a, (b, 0)], [(5, [0, (1, -1)]), (None, []), (q - 1, [1] * 8)])
    assert t["N"] == 64 and t["columns"] == [(a, 0), (b, 0)]
    assert t["terms"] == [((5).to_bytes(32, "little"), [(0, 0), (1, -1)]), (None, []), ((q - 1).to_bytes(32, "little"), [(1, 0)] * 8)]
    assert _args([(a, 4), (b, 4)], [(None, [0])])["N"] == 60                      # the same number of entries from `first`
    assert _args([(a, 4), (o, 40)], [(None, [0])])["N"] == 60
    assert _args([a, o], [(None, [0])], N=10, out=o, firstOut=90)["N"] == 10
    assert _args([a], [(None, [(0, E.INT32_MAX), (0, E.INT32_MIN)])])["N"] == 64
    for cols, terms, kw in (
            (a, [(None, [0])], {}), ([a], (None, [0]), {}), ([7], [(None, [0])], {}), ([_arr(64, 4, "points")], [(None, [0])], {}),
            ([(a, 0, 0)], [(None, [0])], {}), ([a], [None], {}), ([a], [(None,)], {}), ([a], [(None, 0)], {}), ([a], [(1.0, [0])], {}),
            ([a], [(True, [0])], {}), ([a], [(None, [0.0])], {}), ([a], [(None, [(0, 1.0)])], {}), ([a], [(None, [True])], {}),
            ([a], [(None, [0])], dict(out=7)), ([a], [(None, [0])], dict(out=_arr(64, 4, "points")))):
        with pytest.raises(TypeError):
            _args(cols, terms, **kw)
    same = _arr(64, 1)   # another object for the same handle overlaps all the same
    for cols, terms, kw in (
            ([], [(None, [])], dict(N=4)), ([a] * 17, [(None, [0])], {}), ([a], [], {}), ([a], [(None, [0])] * 33, {}),
            ([a], [(q, [0])], {}), ([a], [(-1, [0])], {}), ([a], [(None, [1])], {}), ([a], [(None, [-1])], {}),
            ([a], [(None, [(0, 1 << 31)])], {}), ([a], [(None, [(0, -(1 << 31) - 1)])], {}), ([a], [(None, [0] * 9)], {}),
            ([a, o], [(None, [0])], {}),                                              # different lengths and no N
            ([(a, 1), b], [(None, [0])], {}), ([a], [(None, [0])], dict(N=0)), ([a], [(None, [0])], dict(N=65)),
            ([a], [(None, [0])], dict(N=True)), ([a], [(None, [0])], dict(N=1 << 32)), ([(a, 64)], [(None, [0])], dict(N=1)),
            ([(a, -1)], [(None, [0])], dict(N=1)), ([(a, 60)], [(None, [0])], dict(N=5)), ([a], [(None, [0])], dict(firstOut=1)),
            ([a], [(None, [0])], dict(out=o, firstOut=37)), ([a], [(None, [0])], dict(out=o, firstOut=-1)),
            ([a, a], [(None, [(k % 2, k // 2) for k in range(8 * t, 8 * t + 8)]) for t in range(4)] + [(None, [(0, 16)])], {}),
            ([(a, 8)], [(None, [0])], dict(N=8, out=same, firstOut=9)), ([(a, 8)], [(None, [0])], dict(N=8, out=a, firstOut=1)),
            ([(a, 8)], [(None, [0])], dict(N=8, out=a, firstOut=15)),                   # unrotated: every partial overlap
            ([(a, 8)], [(None, [(0, 1)])], dict(N=8, out=a, firstOut=8)),              # rotated: the exact range too
            ([(a, 8)], [(None, [0, (0, 8), (0, -3)])], dict(N=8, out=same, firstOut=15)),
            ([(a, 8)], [(None, [(0, 1)])], dict(N=8, out=a, firstOut=1))):
        with pytest.raises(ValueError):
            _args(cols, terms, **kw)
    assert _args([(a, 8)], [(3, [0, (0, 8), (0, -16)])], N=8, out=same, firstOut=8)["N"] == 8    # rot = 0 mod N: in place
    assert _args([(a, 8)], [(None, [(0, 1)])], N=8, out=a, firstOut=16)["N"] == 8                 # rotated and adjacent
    assert _args([(a, 8)], [(None, [(0, 1)])], N=8, out=a, firstOut=0)["N"] == 8
    assert _args([(b, 8), (a, 12)], [(None, [(0, 1)])], N=8, out=a, firstOut=13)["N"] == 8       # an unnamed column overlaps anything
    assert _args([(a, 8)], [(7, [])], N=8, out=a, firstOut=11)["N"] == 8                          # constants only: nothing is read
    assert _args([a, a], [(None, [(k % 2, k // 2) for k in range(8 * t, 8 * t + 8)]) for t in range(4)] + [(None, [(0, 64)])])["N"] == 64


# ------------------------------------------------------------------------------------------------ the library
NAMES = ("msmz_scalars_expr", "msmz_test_expr_geometry")


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in NAMES:
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    assert (_native.MSMZ_EXPR_MAX_COLUMNS, _native.MSMZ_EXPR_MAX_TERMS, _native.MSMZ_EXPR_MAX_DEGREE,
            _native.MSMZ_EXPR_MAX_OPERANDS) == (E.MAX_COLUMNS, E.MAX_TERMS, E.MAX_DEGREE, E.MAX_OPERANDS)
    from msm_zprize_amd.parallel import _Parallel
    assert callable(_Parallel.evaluateExpression)


def test_geometry(driver, lib):
    """msmz_test_expr_geometry == the constants the driver was compiled with; needs no context.  The slot count is 0 (the
    register-resident kernel is not built) or one of its instances; the program fits a kernel argument"""
    w, s = C.c_uint32(99), C.c_uint32(99)
    lib.msmz_test_expr_geometry(C.byref(w), C.byref(s))
    threads, slots, slots_max, program = (int(v) for v in driver(["geometry"])[0])
    assert (w.value, s.value) == (threads, slots)
    assert w.value % 64 == 0 and w.value >= 64 and s.value in (0, 2, 4, 8) and slots_max == 8 and program <= 2048
    lib.msmz_test_expr_geometry(None, None)


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof and the offsets of every field of the four descriptors, C side == ctypes side; the limits too"""
    from msm_zprize_amd import _native as N
    src = tmp_path / "layout.c"
    prints, want = [], []
    for cname, T in (("msmz_expr_column", N.MsmzExprColumn), ("msmz_expr_factor", N.MsmzExprFactor), ("msmz_expr_term", N.MsmzExprTerm),
                     ("msmz_expr", N.MsmzExpr)):
        prints.append(f'printf("%zu ", sizeof({cname}));')
        want.append(C.sizeof(T))
        for fname, _ in T._fields_:
            prints.append(f'printf("%zu ", offsetof({cname}, {fname}));')
            want.append(getattr(T, fname).offset)
    prints.append('printf("%d %d %d %d", MSMZ_EXPR_MAX_COLUMNS, MSMZ_EXPR_MAX_TERMS, MSMZ_EXPR_MAX_DEGREE, MSMZ_EXPR_MAX_OPERANDS);')
    want += [16, 32, 8, 32]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msmz.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()] == want
    assert (C.sizeof(N.MsmzExprColumn), C.sizeof(N.MsmzExprFactor), C.sizeof(N.MsmzExprTerm), C.sizeof(N.MsmzExpr)) == (16, 8, 24, 40)


def test_null_arguments_are_bad_arguments(lib):
    """no context, no device -> MSMZ_ERR_ARG and the output handle untouched"""
    from msm_zprize_amd import _native as N
    cols = (N.MsmzExprColumn * 1)(N.MsmzExprColumn(1, 0))
    facs = (N.MsmzExprFactor * 1)(N.MsmzExprFactor(0, 0))
    trms = (N.MsmzExprTerm * 1)(N.MsmzExprTerm(None, facs, 1, 0))
    e = N.MsmzExpr(cols, 1, 1, trms, 4, 0)
    h = C.c_uint64(77)
    assert lib.msmz_scalars_expr(None, C.byref(e), 0, C.byref(h)) == ERR_ARG
    assert lib.msmz_scalars_expr(None, None, 0, C.byref(h)) == ERR_ARG
    assert lib.msmz_scalars_expr(None, C.byref(e), 0, None) == ERR_ARG
    assert h.value == 77


def test_without_a_device_the_method_raises_after_the_argument_checks():
    """evaluateExpression checks its arguments before it reaches for the library: a bad argument raises its own error
    with no context behind the arrays, and there is no fall-back that would compute the expression on the host"""
    from msm_zprize_amd.parallel import _Parallel

    class NoDevice:
        params = {"order": S.order("pallas")}
        _ctx = None
    par = _Parallel(NoDevice())
    a = _arr(8, 1)
    with pytest.raises(ValueError):
        par.evaluateExpression([a], [(None, [1])])
    with pytest.raises(TypeError):
        par.evaluateExpression([a], [(None, 0)])
    import inspect
    from msm_zprize_amd import parallel
    body = inspect.getsource(parallel._Parallel.evaluateExpression)
    assert "msmz_scalars_expr" in body and "expr_args" in body
