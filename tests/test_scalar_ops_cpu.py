"""Scalar-set arithmetic without a GPU: the F_q functions of csrc/fr.h and the body of the powers kernel compiled for
the host (tests/native/scalar_ops_test.cpp, the same templates the kernels instantiate) against Python integers; the
generated constants; the Python argument checks of combineScalars; the exports and the behaviour without a device.
CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "scalar_ops_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "scalar_ops_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


@pytest.fixture(scope="module")
def driver():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "scalar_kernels.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])

    def run(lines):
        """request lines -> one list of ints per answer line"""
        out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) >= len(lines)
        return [[int(v, 16) for v in line.split()] for line in out[:len(lines)]]

    return run


@pytest.mark.parametrize("label", S.ALL)
def test_field_functions_match_python_integers(driver, label):
    """fr_add, fr_sub, fr_mont_mul and the canonical product over ALL pairs of: 0, 1, 2, q - 1, q - 2, the halves,
    2^32 - 1, 2^32, 2^64 - 1, 2^128, 2^224, the largest value below q with seven full low words, and 64 random values;
    then pairs with x + y == q and x + y == q - 1 exactly"""
    q = S.order(label)
    ops = S.operands(label)
    assert len(ops) == 13 + 64 and all(0 <= v < q for v in ops)
    low = S.low_words_full(q)
    assert low < q and low + (1 << 224) >= q and low & ((1 << 224) - 1) == (1 << 224) - 1
    pairs = [(a, b) for a in ops for b in ops]
    rng = random.Random(5)
    for x in ops[:13] + [rng.randrange(q) for _ in range(32)]:
        pairs.append((x, (q - x) % q if x else 0))        # x + y == q (or both 0)
        pairs.append((x, (q - 1 - x) % q))                # x + y == q - 1
    assert any(a + b == q for a, b in pairs) and any(a + b == q - 1 for a, b in pairs)
    got = driver([f"{label} ops {a:x} {b:x}" for a, b in pairs])
    rinv = pow(2, -256, q)
    bad = [(hex(a), hex(b), g) for (a, b), g in zip(pairs, got)
           if g != [(a + b) % q, (a - b) % q, a * b * rinv % q, a * b % q]]
    assert not bad, bad[:3]


@pytest.mark.parametrize("label", S.ALL)
def test_generated_constants(driver, label):
    """R2 and ONE of the *Fr structs (tools/gen_constants.py)"""
    q = S.order(label)
    assert driver([f"{label} const"]) == [[pow(2, 512, q), pow(2, 256, q)]]


@pytest.mark.parametrize("label", S.ALL)
def test_powers_table_and_run(driver, label):
    """the table of ratio^(2^k) and one thread's run of the powers kernel (fr_pow_run): base ratio^(g + j) for ratio in
    {0, 1, q - 1, random} at g in {0, 1, 31, 32, 33, 2^16 - 1, 2^16, 2^32 - 1} (every table entry is used by the last),
    stepping through a whole run where the index allows"""
    q = S.order(label)
    rng = random.Random(S.ALL.index(label) + 9)
    run = int(subprocess.run([EXE], input="geometry\n", capture_output=True, text=True, check=True).stdout.split()[2])
    assert run == 8
    lines, want = [], []
    for ratio in (0, 1, q - 1, rng.randrange(2, q)):
        for base in (1, 0, rng.randrange(2, q)):
            for g in (0, 1, 31, 32, 33, (1 << 16) - 1, 1 << 16, (1 << 32) - 1):
                count = min(run, (1 << 32) - g)
                lines.append(f"{label} pow {base:x} {ratio:x} {g} {count}")
                want.append([base * pow(ratio, g + j, q) % q for j in range(count)])
    assert want[0][:2] == [1, 0]   # 0^0 = 1, 0^1 = 0
    got = driver(lines)
    bad = [(line, g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]


def test_planted_vectors_hold_what_the_issue_asks():
    """the vectors of the GPU tests: 0, 1, q - 1, the carry-chain values and the pairs that sum to q and to 0 in the
    first 64 entries, planted rows again in the last (partial) wave"""
    for label in S.ALL:
        q = S.order(label)
        rows = S.planted_pairs(q, random.Random(0))
        for n in (63, 65, 257, 1000):
            xs, ys = S.build_vectors(label, n, 3)
            assert len(xs) == len(ys) == n and all(0 <= v < q for v in xs + ys)
            head = list(zip(xs[:64], ys[:64]))
            assert {0, 1, q - 1, S.low_words_full(q)} <= set(xs[:64])
            assert any(x + y == q for x, y in head) and any(x == 0 and y == 0 for x, y in head)
            assert set(S.edge_values(q)) <= set(xs[:64])
            last = list(zip(xs, ys))[(n - 1) // 64 * 64:]
            planted = set(S.planted_pairs(q, random.Random(3))) | set(rows)
            assert any((x + y) % q == 0 or x in S.edge_values(q) for x, y in last) or any(r in planted for r in last)


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=100, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


def _args(a, x, b=None, y=None, N=None, firstX=0, firstY=0, out=None, firstOut=0, firstA=0, firstB=0, q=1009):
    from msm_zprize_amd.parallel import combine_scalars_args
    return combine_scalars_args(a, x, b, y, N, firstX, firstY, out, firstOut, firstA, firstB, q)


def test_combine_scalars_args_accepts():
    x, y, c = _arr(100, 1), _arr(80, 2), _arr(60, 3)
    a = _args(5, x)
    assert a["N"] == 100 and a["firstOut"] == 0 and a["terms"] == [(x, 0, None, 0, (5).to_bytes(32, "little"))]
    assert _args(1, x)["terms"] == [(x, 0, None, 0, None)]                 # the coefficient 1: no product
    assert _args(0, x)["terms"][0][4] == bytes(32)
    assert _args(1008, x)["N"] == 100
    a = _args(c, x, 7, y, None, 10, 30, None, 0, 20, 0)                     # vector and broadcast coefficients
    assert a["N"] == 40 and a["terms"] == [(x, 10, c, 20, None), (y, 30, None, 0, (7).to_bytes(32, "little"))]
    a = _args(c, x, c, y)                                                   # Hadamard products
    assert a["N"] == 60 and a["terms"][1] == (y, 0, c, 0, None)
    a = _args(1, x, 9, x, 50, 0, 50, x, 0)                                  # the fold in place: destination == x range
    assert a["N"] == 50 and a["firstOut"] == 0
    assert _args(1, x, 9, x, 50, 0, 50, x, 50)["firstOut"] == 50            # destination == y range
    assert _args(1, x, 9, x, 10, 0, 50, x, 80)["N"] == 10                   # disjoint inside the same handle
    assert _args(1, x, None, None, None, 0, 0, y)["N"] == 80                # another array as the destination
    assert _args(x, x, None, None, 50, 0, 0, x, 0, 0)["N"] == 50            # squares in place


def test_combine_scalars_args_refuses():
    x, y = _arr(100, 1), _arr(80, 2)
    for bad in (_arr(100, 4, "points"), _arr(100, 4, "precomputed"), b"x" * 32, None, 7):
        with pytest.raises(TypeError):
            _args(1, bad)
        with pytest.raises(TypeError):
            _args(1, x, 1, bad)
        if bad is not None:
            with pytest.raises(TypeError):
                _args(1, x, None, None, None, 0, 0, bad)
    for bad in (_arr(100, 4, "points"), b"\x01" * 32, None, True, 1.5):
        with pytest.raises(TypeError):
            _args(bad, x)
        with pytest.raises(TypeError):
            _args(1, x, bad, y)
    with pytest.raises(TypeError):
        _args(1, x, 1, None)          # b without y
    with pytest.raises(TypeError):
        _args(1, x, None, y)          # y without b
    for coeff in (1009, -1, 1 << 256):
        with pytest.raises(ValueError):
            _args(coeff, x)
        with pytest.raises(ValueError):
            _args(1, x, coeff, y)
    for name in ("N", "firstX", "firstY", "firstOut", "firstA", "firstB"):
        for bad in (-1, True, 1.0, 2.5, "1"):
            kw = {name: bad}
            with pytest.raises(ValueError):
                _args(x, x, x, x, **{"N": 10, "out": x, **kw})
    for kw in (dict(N=0), dict(N=101), dict(N=1 << 32), dict(N=51, firstX=50), dict(N=1, firstX=100),
               dict(N=10, firstY=71), dict(N=10, firstA=91), dict(N=10, firstB=75), dict(N=10, out=y, firstOut=71)):
        with pytest.raises(ValueError):
            _args(x, x, y, y, **kw)
    with pytest.raises(ValueError):
        _args(3, x, None, None, 10, firstA=2)          # firstA without a coefficient array
    with pytest.raises(ValueError):
        _args(3, x, None, None, 10, firstY=2)          # firstY without y
    with pytest.raises(ValueError):
        _args(3, x, None, None, 10, firstOut=5)        # firstOut without out
    for first_out in (1, 25, 49, 51):                  # partial overlap of the destination with x [0, 50) or y [50, 100)
        with pytest.raises(ValueError):
            _args(1, x, 9, x, 49, 0, 50, x, first_out)
    with pytest.raises(ValueError):
        _args(x, y, None, None, 50, 0, 0, x, 10, 0)    # partial overlap with the coefficient range
    same = _arr(100, 1)                                  # another object for the same handle overlaps all the same
    with pytest.raises(ValueError):
        _args(1, x, None, None, 50, 0, 0, same, 25)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in ("msmz_scalars_combine", "msmz_scalars_dot", "msmz_scalars_powers", "msmz_test_scalar_dot_geometry"):
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    assert C.sizeof(_native.MsmzScalarTerm) == 40


def test_dot_geometry_accessor(lib):
    """msmz_test_scalar_dot_geometry == the constants the host driver was compiled with; needs no context"""
    t, p = C.c_uint32(0), C.c_uint32(0)
    lib.msmz_test_scalar_dot_geometry(C.byref(t), C.byref(p))
    out = subprocess.run([EXE], input="geometry\n", capture_output=True, text=True, check=True).stdout.split()
    assert [t.value, p.value] == [int(out[0]), int(out[1])] and t.value % 256 == 0 and p.value >= 64
    lib.msmz_test_scalar_dot_geometry(None, None)


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG and the outputs untouched, for all three entry points"""
    from msm_zprize_amd import _native
    one = (1).to_bytes(32, "little")
    term = _native.MsmzScalarTerm(1, 0, 0, 0, one)
    h = C.c_uint64(0)
    assert lib.msmz_scalars_combine(None, C.byref(term), None, 1, 0, C.byref(h)) == 1
    assert h.value == 0
    h = C.c_uint64(77)
    assert lib.msmz_scalars_combine(None, C.byref(term), C.byref(term), 1, 0, C.byref(h)) == 1
    assert h.value == 77
    out = C.create_string_buffer(b"\xaa" * 32, 32)
    assert lib.msmz_scalars_dot(None, 1, 0, 0, 0, 1, out) == 1
    assert out.raw == b"\xaa" * 32
    h = C.c_uint64(0)
    assert lib.msmz_scalars_powers(None, one, one, 1, C.byref(h)) == 1
    assert h.value == 0
