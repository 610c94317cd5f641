"""msmz_points_mul_opts without a GPU: the bounded plain chain and the GLV chain of csrc/mul_kernels.h compiled for the
host (tests/native/points_mul_opts_test.cpp, the same templates the kernels instantiate) against the oracle; the chain
choice and the cost models, pinned; the Python argument checks of mulPoints' options; the export; the behaviour without
a device.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import check_points_util as U
import points_mul_opts_util as O
import points_mul_util as M
from oracle import bigint_ref as B
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "points_mul_opts_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "points_mul_opts_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


@pytest.fixture(scope="module")
def driver():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mul_kernels.h", "curve.h", "scalar.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])

    def run(label, cases):
        """cases: (mode, bits, s, P, Q or None) -> ([(point, neg0, neg1, inverted)], the trailing lines)"""
        lines = []
        for mode, bits, s, p, q in cases:
            z = q if q is not None else U.pt(0, 0)
            lines.append(f"{label} {mode} {bits} {s:x} {p['x']:x} {p['y']:x} {int(p['isZero'])} {int(q is not None)} "
                         f"{z['x']:x} {z['y']:x} {int(z['isZero'])}")
        out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) > len(cases) and out[len(cases)].startswith("chain")
        got = []
        for line in out[:len(cases)]:
            x, y, inf, n0, n1, inverted = line.split()
            got.append((U.pt(int(x, 16), int(y, 16), inf == "1"), int(n0), int(n1), int(inverted)))
        return got, [line.split() for line in out[len(cases):] if line]

    return run


def _cases(params, mode, bits, scalars, points, rq):
    cases, want = [], []
    for s in scalars:
        for p in points:
            sp = U.scale(params, s, p)
            for addend in (None, M.neutral(params), sp, M.negate(params, sp), rq):
                cases.append((mode, bits, s, p, addend))
                want.append(M.canon(params, sp if addend is None else U.add(params, sp, addend)))
    return cases, want


@pytest.mark.parametrize("label", O.WEIER)
def test_glv_chain_matches_the_oracle(driver, label):
    """glv_decompose + glv_table_begin / _finish + group_times_glv (+ Q) == the oracle's [s]P (+ Q): s over 0, 1, 2, 3,
    q - 1, lambda, lambda +- 1, q - lambda, powers of two at the word boundaries and 16 random; P over G, [k]G and
    infinity; Q over none, infinity, +-[s]P and a random point.  Both branches of the table ran: equal signs (T for
    free, nothing inverted) and unequal signs (the affine addition, with an inverse)."""
    params = P.CURVES[label]
    q = params["order"]
    rng = random.Random(O.ALL.index(label) + 177)
    g = U.generator(params)
    points = [g, U.scale(params, rng.randrange(1, q), g), M.neutral(params)]
    rq = U.scale(params, rng.randrange(1, q), g)
    cases, want = _cases(params, "glv", 0, O.glv_scalars(label, rng), points, rq)
    got, _ = driver(label, cases)
    bad = [(hex(c[2]), c[3], c[4], g_[0], w) for c, g_, w in zip(cases, got, want) if g_[0] != w]
    assert not bad, bad[:3]
    finite = [(n0, n1, inv) for (c, (_, n0, n1, inv)) in zip(cases, got) if not c[3]["isZero"]]
    assert any(n0 == n1 for n0, n1, _ in finite) and any(n0 != n1 for n0, n1, _ in finite)
    assert all(inv == (1 if n0 != n1 else 0) for n0, n1, inv in finite)
    assert all(inv == 0 for c, (_, _, _, inv) in zip(cases, got) if c[3]["isZero"])   # P at infinity feeds a 1
    assert M.neutral(params) in want and any(w != M.neutral(params) for w in want)


@pytest.mark.parametrize("label", [label for label in O.WEIER if P.CURVES[label]["cofactor"] != 1])
def test_glv_chain_is_safe_outside_the_subgroup(driver, label):
    """what the vouch does NOT cover: a named small-order point (x = 0 among them: phi P = P, T = O with unequal signs)
    gives infinity or a point of the curve, whatever the scalar"""
    params = P.CURVES[label]
    rng = random.Random(3)
    aw = B.AffineWeierstrass(params)
    cases = [("glv", 0, s, p, None) for p in M.on_curve_named(label) for s in O.glv_scalars(label, rng)]
    got, _ = driver(label, cases)
    assert all(r["isZero"] or aw.is_on_curve((r["x"], r["y"], False)) for r, _, _, _ in got)
    zero_x = [(n0, n1, inv) for c, (_, n0, n1, inv) in zip(cases, got) if c[3]["x"] == 0]
    assert zero_x and any(n0 != n1 for n0, n1, _ in zero_x) and all(inv == 0 for _, _, inv in zero_x)


@pytest.mark.parametrize("label", O.ALL)
def test_bounded_chain_matches_the_oracle(driver, label):
    """group_times_scalar over b bits, b in 1, 31, 32, 33, 64, 128, 129, 200 and the bit length of q, with scalars up to
    min(2^b, q) - 1: every word boundary of the shift register's skip"""
    params = P.CURVES[label]
    q = params["order"]
    rng = random.Random(O.ALL.index(label) + 277)
    g = U.generator(params)
    points = [g, U.scale(params, rng.randrange(1, q), g), M.neutral(params)]
    rq = U.scale(params, rng.randrange(1, q), g)
    cases, want = [], []
    for b in O.BOUNDS + [O.order_bits(label)]:
        scalars = O.bounded_scalars(label, b, rng)
        assert min(1 << b, q) - 1 in scalars
        c, w = _cases(params, "plain", b, scalars, points, rq)
        cases += c
        want += w
    got, _ = driver(label, cases)
    bad = [(c[1], hex(c[2]), c[3], c[4], g_[0], w) for c, g_, w in zip(cases, got, want) if g_[0] != w]
    assert not bad, bad[:3]


def test_chain_choice_is_pinned(driver):
    """points_mul_chain for every curve, with and without the vouch, at b = 0, 64, GLV_PROVEN_BITS, GLV_PROVEN_BITS + 1, 256"""
    _, tail = driver("pallas", [])
    got = {(t[1], int(t[2]), int(t[3])): (int(t[4]), int(t[5])) for t in tail if t[0] == "chain"}
    want = {}
    for label, bits, h in (("bls12-377", 253, 126), ("pallas", 255, 128), ("bls12-381", 255, 128)):
        for b, plain, vouched in ((0, (0, bits), (1, h)), (64, (0, 64), (0, 64)), (h, (0, h), (0, h)),
                                  (h + 1, (0, h + 1), (1, h)), (256, (0, bits), (1, h))):
            want[(label, 0, b)] = plain
            want[(label, 1, b)] = vouched
    for flag in (0, 1):   # no endomorphism: the vouch changes nothing
        want.update({("ed-on-bls12-377", flag, 0): (0, 251), ("ed-on-bls12-377", flag, 64): (0, 64),
                     ("ed-on-bls12-377", flag, 1): (0, 1), ("ed-on-bls12-377", flag, 256): (0, 251)})
    assert got == want
    for (label, flag, b), v in want.items():   # and the tests' own statement of the rules agrees
        assert O.chain(label, bool(flag), b) == v


def test_cost_models_are_pinned(driver):
    """points_mul_products_glv = h 9 + (3h / 4) 10 + 1 + 14 + 3 (+ 10) + 19; points_mul_products_bounded = the plain
    model over b bits"""
    _, tail = driver("pallas", [])
    glv = [int(v) for t in tail if t[0] == "products_glv" for v in t[1:]]
    bounded = [int(v) for t in tail if t[0] == "products_bounded" for v in t[1:]]
    assert glv == [2121, 2159, 2159, 2111, 2149, 2149]
    assert bounded == [128 * 9 + 64 * 10 + 10 + 19, 128 * 9 + 64 * 10 + 10 + 19, 64 * 9 + 32 * 10 + 10 + 19,
                       128 * 9 + 64 * 7 + 7 + 18]


# ------------------------------------------------------------------------------------------------ Python arguments
def test_mul_points_opts_args():
    from msm_zprize_amd import _native
    from msm_zprize_amd.parallel import DeviceArray, mul_points_opts
    arr = DeviceArray(None, 1, 100, "scalars")
    o = mul_points_opts(arr, 0, False)
    assert (o.flags, o.scalar_bits, list(o.reserved)) == (0, 0, [0, 0])
    o = mul_points_opts(arr, 128, True)
    assert (o.flags, o.scalar_bits, list(o.reserved)) == (_native.MSMZ_MUL_SUBGROUP, 128, [0, 0])
    assert mul_points_opts((1 << 128) - 1, 128, False).scalar_bits == 128
    assert mul_points_opts(5, 256, True).scalar_bits == 256
    assert mul_points_opts(1 << 200, 0, False).scalar_bits == 0
    for bits in (-1, 257, 1.0, True, "8"):
        with pytest.raises(ValueError):
            mul_points_opts(arr, bits, False)
    for s, bits in ((1 << 128, 128), (2, 1), (1 << 64, 64)):   # the broadcast scalar breaks the bound
        with pytest.raises(ValueError):
            mul_points_opts(s, bits, False)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError):
            mul_points_opts(arr, 0, bad)
    assert C.sizeof(_native.MsmzMulOpts) == 16


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_point_is_exported(lib):
    from msm_zprize_amd import _native
    assert "msmz_points_mul_opts" in _native.EXPORTS
    assert lib.msmz_points_mul_opts is not None
    with open(os.path.join(ROOT, "include", "msmz.h")) as f:
        header = f.read()
    assert "int msmz_points_mul_opts(" in header and "MSMZ_MUL_SUBGROUP = 1" in header


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG, nothing runs: with options and without"""
    from msm_zprize_amd import _native
    m = _native.MsmzMul(1, 0, 0, 0, bytes(32), 0, 0)
    o = _native.MsmzMulOpts(_native.MSMZ_MUL_SUBGROUP, 128)
    h = C.c_uint64(0)
    assert lib.msmz_points_mul_opts(None, C.byref(m), 1, C.byref(o), C.byref(h)) == 1
    assert lib.msmz_points_mul_opts(None, C.byref(m), 1, None, C.byref(h)) == 1
    assert h.value == 0
