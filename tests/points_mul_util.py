"""Shared by the msmz_points_mul tests (tests/test_points_mul_cpu.py, tests/test_points_mul_gpu.py,
tests/test_js_points_mul.py, tests/golden/make_points_mul_fixture.py): what [s]P (+ Q) is, by the oracle
(oracle/bigint_ref.py through check_points_util.scale / add), the rows the issue plants into every set, and the byte
encodings of the C ABI."""
import random

import check_points_util as U
from oracle import params as P

ALL = U.ALL


def neutral(params):
    """the point at infinity as download_points reports it / the twisted-Edwards identity"""
    return U.pt(0, 0, True) if params["kind"] == "weierstrass" else U.pt(0, 1)


def negate(params, q):
    p = params["modulus"]
    if params["kind"] == "weierstrass":
        return U.pt(q["x"], (p - q["y"]) % p, q["isZero"])
    return U.pt((p - q["x"]) % p, q["y"])


def canon(params, q):
    """a result as msmz_download_points gives it: an infinite Weierstrass point is the all-zero record"""
    if params["kind"] == "weierstrass" and q["isZero"]:
        return U.pt(0, 0, True)
    return U.pt(q["x"], q["y"], False)


def expected(params, s, point, addend=None):
    """[s]point (+ addend) by the oracle"""
    r = U.scale(params, s, point)
    if addend is not None:
        r = U.add(params, r, addend)
    return canon(params, r)


def on_curve_named(label):
    params = P.CURVES[label]
    return [q for _, q in U.table_points(label) if U.verdict(params, q) != U.OFF_CURVE]


def small_order_rows(label):
    """(point, s a multiple of its order, s not a multiple) for one named small-order point of a cofactor curve"""
    params = P.CURVES[label]
    if params["cofactor"] == 1:
        return []
    name, q = U.table_points(label)[0]
    order = int(name.split("order ")[1])
    return [(q, 6 * order * 1000003, 6 * order * 1000003 + 1)]


def planted_rows(label, rng):
    """The rows of the issue: (s, P, Q or None for 'Q = infinity').  Q is used only by the addend mode."""
    params = P.CURVES[label]
    q = params["order"]
    g = U.generator(params)
    pk = U.scale(params, rng.randrange(1, q), g)
    rq = U.scale(params, rng.randrange(1, q), g)
    s = rng.randrange(1, q)
    sp = U.scale(params, s, pk)
    rows = [(0, pk, rq), (1, pk, rq), (q - 1, pk, rq), (rng.randrange(q), neutral(params), rq),
            (rng.randrange(q), pk, neutral(params)), (s, pk, sp), (s, pk, negate(params, sp))]
    for pt, mult, other in small_order_rows(label):
        rows += [(mult, pt, rq), (other, pt, rq)]
    return rows


def build_set(label, n, seed):
    """n rows (s, P, Q): the planted rows in the first lanes AND ending at the last index (the partial wave), random
    multiples of G elsewhere"""
    params = P.CURVES[label]
    q = params["order"]
    rng = random.Random(seed)
    g = U.generator(params)
    pool = [U.scale(params, rng.randrange(1, q), g) for _ in range(6)]
    rows = [(rng.randrange(q), pool[rng.randrange(6)], pool[rng.randrange(6)]) for _ in range(n)]
    planted = planted_rows(label, rng)
    for k, row in enumerate(planted):
        if k < n:
            rows[k] = row
    for k in range(len(planted)):   # (rotated by n: the one-lane last waves of n = 65 and 257 get different rows)
        if n - 1 - k >= min(len(planted), n):
            rows[n - 1 - k] = planted[(k + n) % len(planted)]
    return rows


def encode_scalars(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def same(params, got, want):
    """downloaded point == oracle point (a Weierstrass infinity: flag and all-zero record)"""
    return canon(params, got) == canon(params, want)
