"""Shared by the compressed-point tests (tests/test_compressed_cpu.py, tests/test_compressed_gpu.py,
tests/golden/make_compressed_fixture.py): compressed records built from Python integers, and the points a test set is
made of.  The wire coordinate is x on the Weierstrass curves and y on the twisted Edwards curve; bit 7 of the last byte
is the sign of the other coordinate: "largest" = its canonical value is above (p - 1) / 2, "parity" = it is odd."""
import random

import check_points_util as U
from oracle import params as P

SIGNS = ("largest", "parity")


def two_adicity(p):
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    return s, t


def sign_of(value, p, sign):
    return value & 1 if sign == "parity" else int(value > (p - 1) // 2)


def wire_other(params, q):
    return (q["x"], q["y"]) if params["kind"] == "weierstrass" else (q["y"], q["x"])


def record(params, q, sign, flip=False):
    """the compressed record of the affine point q (bytes); flip: with the sign bit inverted"""
    p, fb = params["modulus"], params["fe_bytes"]
    wire, other = wire_other(params, q)
    bit = sign_of(other, p, sign) ^ int(flip)
    return (wire | (bit << (8 * fb - 1))).to_bytes(fb, "little")


def negated(params, q):
    """the point with the same wire coordinate and the other root"""
    p = params["modulus"]
    if params["kind"] == "weierstrass":
        return U.pt(q["x"], (p - q["y"]) % p)
    return U.pt((p - q["x"]) % p, q["y"])


def decompress(params, wire, bit, sign):
    """Python reference: -> the point, or None if the record is no point"""
    p = params["modulus"]
    if params["kind"] == "weierstrass":
        root = U.sqrt_mod(wire ** 3 + params["b"], p)
    else:
        root = U.sqrt_mod((wire * wire - 1) * pow(params["d"] * wire * wire + 1, -1, p), p)
    if root is None or (root == 0 and bit):
        return None
    if sign_of(root, p, sign) != bit:
        root = p - root
    return U.pt(wire, root) if params["kind"] == "weierstrass" else U.pt(root, wire)


def on_curve_named(label):
    """the named points of check_points_util.table_points that lie on the curve (zero roots and small orders among them)"""
    params = P.CURVES[label]
    return [q for _, q in U.table_points(label) if U.verdict(params, q) != U.OFF_CURVE]


def non_residue_wire(params, rng):
    """a wire coordinate below p whose right-hand side has no square root"""
    p = params["modulus"]
    while True:
        w = rng.randrange(p)
        if decompress(params, w, 0, "largest") is None:
            return w


def zero_root_wires(params):
    """wire coordinates whose recovered coordinate is 0 (a sign bit on them is refused), if the curve has any"""
    p = params["modulus"]
    if params["kind"] == "twisted-edwards":
        return [1, p - 1]                      # (0, 1) and (0, -1)
    if params["label"] == "bls12-377":
        return [p - 1]                         # (-1, 0): b = 1
    return []                                  # y = 0 needs a cube root of -b: none on Pallas (b = 5) / BLS12-381 (b = 4)


def round_trip_points(label, n, seed=11):
    """(n points of the curve, n flag bytes) for a round trip: the named points, raw points from random x (any
    subgroup), multiples of G.  Indices i % 7 == 3 are flagged: their records carry junk and are not decompressed; the
    point there is infinity, on the twisted Edwards curve (which has none) the identity (0, 1)."""
    params = P.CURVES[label]
    rng = random.Random(seed)
    g = U.generator(params)
    pts = on_curve_named(label) + [U.raw_point(params, rng) for _ in range(12)]
    acc = g
    while len(pts) < n:
        pts.append(acc)
        acc = U.add(params, acc, g)
    pts = pts[:n]
    flags = bytes(1 if i % 7 == 3 else 0 for i in range(n))
    for i in range(n):
        if flags[i]:
            pts[i] = U.pt(0, 0, True) if params["kind"] == "weierstrass" else U.pt(0, 1)
    return pts, flags


def records(params, pts, flags, sign, rng):
    """packed compressed records of pts; flagged entries get junk bytes"""
    fb = params["fe_bytes"]
    return b"".join(bytes(rng.randrange(256) for _ in range(fb)) if f else record(params, q, sign) for q, f in zip(pts, flags))


def want_compressed(params, pts, sign):
    """what msmz_download_points_compressed owes these points: (records, flags); infinity is the all-zero record"""
    fb = params["fe_bytes"]
    recs = b"".join(bytes(fb) if q["isZero"] else record(params, q, sign) for q in pts)
    return recs, bytes(1 if q["isZero"] else 0 for q in pts)
