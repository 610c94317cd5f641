"""msmz_check_points without a GPU: the chain [q]P and the curve equations of csrc/check_kernels.h compiled for the host
(tests/native/check_points_test.cpp, the same templates the kernels instantiate) against the oracle's verdicts; the
Python argument checks of checkPoints / check=; the export; the behaviour without a device.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import check_points_util as U
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "check_points_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "check_points_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


@pytest.fixture(scope="module")
def driver():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("check_kernels.h", "curve.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])

    def run(label, pts):
        lines = [f"{label} {q['x']:x} {q['y']:x} {int(q['isZero'])}" for q in pts]
        out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) >= len(pts) + 1 and out[len(pts)].startswith("weights")
        return [int(v) for v in out[:len(pts)]], [int(w) for w in out[len(pts)].split()[1:]]

    return run


@pytest.mark.parametrize("label", U.ALL)
def test_host_chain_matches_the_oracle(driver, label):
    """the generator, k G, the identity / a flagged infinity with junk coordinates, every named point of the curve, 32 raw
    points from random x and the same 32 times the cofactor: the verdict of the kernels' code == the oracle's"""
    params = P.CURVES[label]
    p = params["modulus"]
    rng = random.Random(U.ALL.index(label) + 41)
    g = U.generator(params)
    pts = [g] + [U.scale(params, k, g) for k in (2, 3, 5, 0xFFFF, params["order"] - 1, rng.randrange(params["order"]))]
    if params["kind"] == "weierstrass":
        pts += [U.pt(rng.randrange(p), rng.randrange(p), True), U.pt(0, 0, True)]
        pts.append(U.pt(0, 0))   # unflagged: zero is stored as a non-zero multiple of p, so this is no infinity record
    else:
        pts.append(U.pt(0, 1))
    named = U.table_points(label)
    pts += [q for _, q in named]
    raw, cleared = U.helper_points(label, rng, 32)
    pts += raw + cleared
    pts += [U.pt(g["x"], (g["y"] + 1) % p), U.pt(rng.randrange(p), rng.randrange(p))]
    want = [U.verdict(params, q) for q in pts]
    got, _ = driver(label, pts)
    assert got == want
    # the vectors do cover what they are meant to: both verdicts on the cofactor curves, good points everywhere
    assert 0 in want and U.OFF_CURVE in want
    assert (U.OFF_SUBGROUP in want) == (params["cofactor"] != 1)
    assert all(U.verdict(params, q) == 0 for q in cleared)


def test_named_points_are_what_the_issue_says():
    """the table of bad points, by the oracle: on / off the curve, inside / outside the subgroup"""
    want = {"bls12-377": [2, 2, 2, 2, 1], "bls12-381": [2, 2, 1, 1], "ed-on-bls12-377": [2, 2, 0], "pallas": [1, 1]}
    for label in U.ALL:
        assert [U.verdict(P.CURVES[label], q) for _, q in U.table_points(label)] == want[label], label


def test_chain_weight_is_the_hamming_weight_of_q(driver):
    """order_weight<Fr>() (the additions of one chain, the report tool's product count) == popcount(q)"""
    _, weights = driver("pallas", [U.generator(P.PALLAS)])
    assert weights == [bin(P.CURVES[l]["order"]).count("1") for l in U.ALL]


@pytest.mark.parametrize("label", U.ALL)
def test_square_roots_square_back(label):
    params = P.CURVES[label]
    p = params["modulus"]
    rng = random.Random(3)
    roots = 0
    for a in [0, 1, 4, p - 1] + [rng.randrange(p) for _ in range(60)]:
        r = U.sqrt_mod(a, p)
        if r is None:
            assert pow(a, (p - 1) // 2, p) == p - 1
        else:
            roots += 1
            assert r * r % p == a % p
    assert roots > 20
    for _ in range(8):
        q = U.raw_point(params, rng)
        assert U.verdict(params, q) != U.OFF_CURVE


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(kind="points", n=100):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, 1, n, kind)


def test_check_points_args():
    from msm_zprize_amd.parallel import check_points_args
    assert check_points_args(_arr(), None, True, 0) == (0, 100, 3)
    assert check_points_args(_arr(), None, False, 40) == (40, 60, 1)
    assert check_points_args(_arr(), 1, True, 99) == (99, 1, 3)
    for first, n in [(-1, 1), (100, 1), (0, 0), (0, 101), (50, 51), (0, -3), (True, 1), (0, True), (1.0, 1), (0, 2.0)]:
        with pytest.raises(ValueError):
            check_points_args(_arr(), n, True, first)
    for bad in (_arr("scalars"), _arr("precomputed"), b"points", None):
        with pytest.raises(TypeError):
            check_points_args(bad, None, True, 0)


def test_check_spellings():
    from msm_zprize_amd.parallel import check_arg
    assert check_arg(None, "t") == 0 and check_arg("curve", "t") == 1 and check_arg("subgroup", "t") == 3
    for bad in ("Curve", "group", "", True, 1, "both"):
        with pytest.raises(ValueError):
            check_arg(bad, "t")


def test_result_object():
    from msm_zprize_amd.parallel import CheckResult
    r = CheckResult(False, 1, 2, 7, b"\x00\x01")
    assert (r.ok, r.offCurve, r.offSubgroup, r.firstBad, r.verdicts) == (False, 1, 2, 7, b"\x00\x01")
    assert "firstBad=7" in repr(r)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_point_is_exported(lib):
    from msm_zprize_amd import _native
    assert "msmz_check_points" in _native.EXPORTS
    assert lib.msmz_check_points is not None
    assert C.sizeof(_native.MsmzCheckResult) == 24


def test_null_context_is_a_bad_argument(lib):
    """as tests/test_cabi_cpu.py expects of the other entry points: no context, no device -> MSMZ_ERR_ARG, nothing runs"""
    from msm_zprize_amd import _native
    res = _native.MsmzCheckResult()
    assert lib.msmz_check_points(None, 1, 0, 1, 3, C.byref(res), None) == 1
    assert lib.msmz_strerror(1) == b"bad argument"
