"""msmz_points_mul without a GPU: the chain [s]P and the final addition of csrc/mul_kernels.h compiled for the host
(tests/native/points_mul_test.cpp, the same templates the kernels instantiate) against the oracle; the Python argument
checks of mulPoints; the export; the behaviour without a device.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import check_points_util as U
import points_mul_util as M
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "points_mul_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "points_mul_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


@pytest.fixture(scope="module")
def driver():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mul_kernels.h", "curve.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])

    def run(label, cases):
        """cases: (s, P, Q or None) -> the driver's points, and its trailing `products` line"""
        lines = []
        for s, p, q in cases:
            z = q if q is not None else U.pt(0, 0)
            lines.append(f"{label} {s:x} {p['x']:x} {p['y']:x} {int(p['isZero'])} {int(q is not None)} "
                         f"{z['x']:x} {z['y']:x} {int(z['isZero'])}")
        out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) >= len(cases) + 1 and out[len(cases)].startswith("products")
        pts = []
        for line in out[:len(cases)]:
            x, y, inf = line.split()
            pts.append(U.pt(int(x, 16), int(y, 16), inf == "1"))
        return pts, [int(v) for v in out[len(cases)].split()[1:]]

    return run


def scalars_of(params, rng):
    q = params["order"]
    return [0, 1, 2, 3, q - 1] + [1 << k for k in (31, 32, 63, 64, 127, 128, 224)] + [rng.randrange(q) for _ in range(16)]


@pytest.mark.parametrize("label", M.ALL)
def test_host_chain_matches_the_oracle(driver, label):
    """[s]P (+ Q) from the MSMZ_HD functions == the oracle: s over 0, 1, 2, 3, q - 1, the powers of two at the word
    boundaries of the bit walk and 16 random scalars; P over G, [k]G, infinity / (0, 1) and every on-curve named point;
    Q over none, infinity, [s]P (the addition is a doubling), -[s]P and a random point"""
    params = P.CURVES[label]
    q = params["order"]
    rng = random.Random(M.ALL.index(label) + 77)
    g = U.generator(params)
    points = [g, U.scale(params, rng.randrange(1, q), g), M.neutral(params)] + M.on_curve_named(label)
    rq = U.scale(params, rng.randrange(1, q), g)
    cases, want = [], []
    for s in scalars_of(params, rng):
        for p in points:
            sp = U.scale(params, s, p)
            for addend in (None, M.neutral(params), sp, M.negate(params, sp), rq):
                cases.append((s, p, addend))
                want.append(M.canon(params, sp if addend is None else U.add(params, sp, addend)))
    got, _ = driver(label, cases)
    bad = [(hex(c[0]), c[1], c[2], g_, w) for c, g_, w in zip(cases, got, want) if g_ != w]
    assert not bad, bad[:3]
    # the vectors do cover what they are meant to: identities and finite results, and small orders on the cofactor curves
    assert M.neutral(params) in want and any(w != M.neutral(params) for w in want)
    assert (len(points) > 3) == (params["cofactor"] != 1)


def test_cost_model_counts(driver):
    """points_mul_products (the report tool's product count, with an addend): chain + addend + normalisation"""
    _, products = driver("pallas", [(1, U.generator(P.PALLAS), None)])
    want = []
    for label in M.ALL:
        bits = P.CURVES[label]["order"].bit_length()
        te = P.CURVES[label]["kind"] != "weierstrass"
        want.append(bits * 9 + (bits // 2) * 7 + 7 + 18 if te else bits * 9 + (bits // 2) * 10 + 10 + 19)
    assert products == want


def test_planted_sets_hold_what_the_issue_asks():
    """the sets of the GPU tests: every planted row in the first 64 lanes, one in the last (partial) wave"""
    for label in M.ALL:
        params = P.CURVES[label]
        q = params["order"]
        for n in (63, 65, 257):
            rows = M.build_set(label, n, 3)
            assert len(rows) == n
            head = rows[:64]
            assert any(s == 0 for s, _, _ in head) and any(s == 1 for s, _, _ in head) and any(s == q - 1 for s, _, _ in head)
            assert any(p == M.neutral(params) for _, p, _ in head) and any(a == M.neutral(params) for _, _, a in head)
            sums = [M.expected(params, s, p, a) for s, p, a in head[:9]]
            assert M.neutral(params) in sums                                       # Q = -[s]P
            assert any(M.expected(params, s, p) == M.canon(params, a) for s, p, a in head[:9])   # Q = [s]P
            planted = M.planted_rows(label, random.Random(0))
            assert len(planted) == (7 if params["cofactor"] == 1 else 9)
            last = rows[(n - 1) // 64 * 64:]
            assert any(s in (0, 1, q - 1) or p == M.neutral(params) or a == M.neutral(params) or
                       M.expected(params, s, p, a) == M.neutral(params) or M.expected(params, s, p) == M.canon(params, a) or
                       U.verdict(params, p) == U.OFF_SUBGROUP for s, p, a in last)


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(kind="points", n=100):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, 1, n, kind)


def test_mul_points_args():
    from msm_zprize_amd.parallel import mul_points_args
    q = 1009
    a = mul_points_args(_arr("scalars"), _arr(), None, None, 0, 0, 0, q)
    assert a == {"N": 100, "firstPoint": 0, "firstScalar": 0, "firstAddend": 0, "scalar": None}
    a = mul_points_args(_arr("scalars", 80), _arr(), None, _arr(n=60), 10, 30, 20, q)
    assert (a["N"], a["firstPoint"], a["firstScalar"], a["firstAddend"]) == (40, 10, 30, 20)
    a = mul_points_args(5, _arr(), 50, _arr(), 50, 0, 0, q)   # the fold: one array as both operands
    assert a["N"] == 50 and a["scalar"] == (5).to_bytes(32, "little")
    assert mul_points_args(0, _arr(), 1, None, 99, 0, 0, q)["scalar"] == bytes(32)
    assert mul_points_args(q - 1, _arr(), None, None, 0, 0, 0, q)["N"] == 100
    for s in (q, -1, 1 << 256):
        with pytest.raises(ValueError):
            mul_points_args(s, _arr(), None, None, 0, 0, 0, q)
    for N, fp, fs, fa in [(0, 0, 0, 0), (-1, 0, 0, 0), (101, 0, 0, 0), (51, 50, 0, 0), (1, 100, 0, 0), (1, -1, 0, 0),
                          (10, 0, 91, 0), (True, 0, 0, 0), (1.0, 0, 0, 0), (1, 0, 1.0, 0), (1, True, 0, 0), (1, 0, 0, 7)]:
        with pytest.raises(ValueError):
            mul_points_args(_arr("scalars"), _arr(), N, None, fp, fs, fa, q)
    with pytest.raises(ValueError):
        mul_points_args(3, _arr(), 1, None, 0, 2, 0, q)        # firstScalar without a scalar array
    with pytest.raises(ValueError):
        mul_points_args(_arr("scalars"), _arr(), 10, _arr(n=20), 0, 0, 11, q)
    for bad in (_arr("scalars"), _arr("precomputed"), b"points", None):
        with pytest.raises(TypeError):
            mul_points_args(1, bad, None, None, 0, 0, 0, q)
    for bad in (_arr("scalars"), _arr("precomputed"), b"x"):
        with pytest.raises(TypeError):
            mul_points_args(1, _arr(), None, bad, 0, 0, 0, q)
    for bad in (_arr("points"), b"\x01" * 32, None, True, 1.5):
        with pytest.raises(TypeError):
            mul_points_args(bad, _arr(), None, None, 0, 0, 0, q)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_point_is_exported(lib):
    from msm_zprize_amd import _native
    assert "msmz_points_mul" in _native.EXPORTS
    assert lib.msmz_points_mul is not None
    assert C.sizeof(_native.MsmzMul) == 56


def test_null_context_is_a_bad_argument(lib):
    """as tests/test_cabi_cpu.py expects of the other entry points: no context, no device -> MSMZ_ERR_ARG, nothing runs"""
    from msm_zprize_amd import _native
    m = _native.MsmzMul(1, 0, 0, 0, bytes(32), 0, 0)
    h = C.c_uint64(0)
    assert lib.msmz_points_mul(None, C.byref(m), 1, C.byref(h)) == 1
    assert h.value == 0
