"""Shared by the msmz_check_points tests (tests/test_check_points_cpu.py, tests/test_check_points_gpu.py,
tests/test_js_check_points.py): points on and off the four curves, inside and outside their prime-order subgroups, and
the verdict the oracle gives each of them.  No verdict is assumed: `verdict` asks the oracle (oracle/bigint_ref.py) for
every point -- is_on_curve, then ProjectiveWeierstrass.scale(q, .) with Z = 0, or TwistedEdwards.scale(q, .) with
is_zero.  (AffineWeierstrass.is_in_subgroup is not usable: it divides by zero as soon as a multiple has order 2.)
`verdict_fast` asks the C oracle's scale instead; the GPU tests use it for the thousands of generated points of a set."""
import random

from oracle import bigint_ref as B
from oracle import c_oracle
from oracle import params as P

ALL = ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"]
OFF_CURVE, OFF_SUBGROUP = 1, 2
NO_INDEX = (1 << 64) - 1


def sqrt_mod(a, p):
    """Tonelli-Shanks: a square root of a mod the odd prime p, or None.  (Of the four base fields only BLS12-381's has
    p = 3 mod 4; the others have 2-adicity 46, 32 and 47.)"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    c, x, b, m = pow(z, t, p), pow(a, (t + 1) // 2, p), pow(a, t, p), s
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2, i = b2 * b2 % p, i + 1
        e = pow(c, 1 << (m - i - 1), p)
        x, c = x * e % p, e * e % p
        b, m = b * c % p, i
    return x


def pt(x, y, inf=False):
    return {"x": x, "y": y, "isZero": inf}


def raw_point(params, rng):
    """a point of the curve from a random x: the raw solution, whatever subgroup it falls in"""
    p = params["modulus"]
    while True:
        x = rng.randrange(p)
        if params["kind"] == "weierstrass":
            y = sqrt_mod(x * x * x + params["b"], p)
        else:   # -x^2 + y^2 = 1 + d x^2 y^2  ->  y^2 = (1 + x^2) / (1 - d x^2)
            den = (1 - params["d"] * x * x) % p
            y = sqrt_mod((1 + x * x) * pow(den, -1, p), p) if den else None
        if y is not None:
            return pt(x, y if rng.randrange(2) else (p - y) % p)


def scale(params, s, point):
    """[s]point by the oracle, as an affine dict"""
    if params["kind"] == "weierstrass":
        pw = B.ProjectiveWeierstrass(params)
        x, y, z = pw.to_affine(pw.scale(s, pw.from_affine((point["x"], point["y"], point["isZero"]))))
        return pt(x, y, z)
    te = B.TwistedEdwards(params)
    x, y = te.to_affine(te.scale(s, te.from_affine((point["x"], point["y"]))))
    return pt(x, y)


def add(params, a, b):
    if params["kind"] == "weierstrass":
        pw = B.ProjectiveWeierstrass(params)
        f = lambda q: pw.from_affine((q["x"], q["y"], q["isZero"]))
        x, y, z = pw.to_affine(pw.add(f(a), f(b)))
        return pt(x, y, z)
    te = B.TwistedEdwards(params)
    f = lambda q: te.from_affine((q["x"], q["y"]))
    x, y = te.to_affine(te.add(f(a), f(b)))
    return pt(x, y)


def generator(params):
    return pt(params["generator"]["x"], params["generator"]["y"])


def verdict(params, point):
    """the verdict byte msmz_check_points owes this point, from the oracle"""
    p, q = params["modulus"], params["order"]
    if params["kind"] == "weierstrass":
        if point["isZero"]:
            return 0   # a flagged record: on the curve and in the subgroup whatever its coordinates
        if not B.AffineWeierstrass(params).is_on_curve((point["x"], point["y"], False)):
            return OFF_CURVE
        pw = B.ProjectiveWeierstrass(params)
        return 0 if pw.scale(q, (point["x"], point["y"], 1))[2] % p == 0 else OFF_SUBGROUP
    te = B.TwistedEdwards(params)
    e = te.from_affine((point["x"], point["y"]))
    if not te.is_on_curve(e):
        return OFF_CURVE
    return 0 if te.is_zero(te.scale(q, e)) else OFF_SUBGROUP


def verdict_fast(params, point):
    """as `verdict`, the scalar multiplication by the C oracle (oracle/msm_oracle.c)"""
    p = params["modulus"]
    if params["kind"] == "weierstrass":
        if point["isZero"]:
            return 0
        if not B.AffineWeierstrass(params).is_on_curve((point["x"], point["y"], False)):
            return OFF_CURVE
        return 0 if c_oracle.scale(params, params["order"], point)["isZero"] else OFF_SUBGROUP
    te = B.TwistedEdwards(params)
    if not te.is_on_curve(te.from_affine((point["x"], point["y"]))):
        return OFF_CURVE
    r = c_oracle.scale(params, params["order"], point)
    return 0 if (r["x"] % p, r["y"] % p) == (0, 1) else OFF_SUBGROUP


def table_points(label):
    """the named points of the feature's issue, (name, point); what they are is the oracle's to say"""
    params = P.CURVES[label]
    p = params["modulus"]
    g = generator(params)
    if label == "bls12-377":
        return [("(0,1) order 3", pt(0, 1)), ("(-1,0) order 2", pt(p - 1, 0)), ("(2,3)", pt(2, 3)),
                ("G+(0,1)", add(params, g, pt(0, 1))), ("(0,2) off", pt(0, 2))]
    if label == "bls12-381":
        return [("(0,2) order 3", pt(0, 2)), ("G+(0,2)", add(params, g, pt(0, 2))), ("(0,1) off", pt(0, 1)),
                ("(2,3) off", pt(2, 3))]
    if label == "ed-on-bls12-377":
        return [("(0,-1) order 2", pt(0, p - 1)), ("(i,0) order 4", pt(sqrt_mod(p - 1, p), 0)), ("(0,1) identity", pt(0, 1))]
    return [("(1,1) off", pt(1, 1)), ("(0,2) off", pt(0, 2))]   # Pallas (b = 5, cofactor 1): nothing on the curve is outside


def helper_points(label, rng, n):
    """n raw points from random x and the same points times the cofactor"""
    params = P.CURVES[label]
    raw = [raw_point(params, rng) for _ in range(n)]
    return raw, [scale(params, params["cofactor"], r) for r in raw]


def bad_points(label, rng, n_raw=8):
    """points to plant in a good set: the table, raw helper points, off-curve neighbours of good points"""
    params = P.CURVES[label]
    p = params["modulus"]
    raw, cleared = helper_points(label, rng, n_raw)
    g = generator(params)
    off = [pt(g["x"], (g["y"] + 1) % p), pt((raw[0]["x"] + 1) % p, raw[0]["y"]), pt(rng.randrange(p), rng.randrange(p))]
    if params["kind"] == "weierstrass":
        off.append(pt(0, 0))   # UNFLAGGED (0, 0): not the infinity record, off the curve like any other such pair
    return [q for _, q in table_points(label)] + raw + cleared[:2] + off


def planted_set(label, good, seed=5):
    """`good` (downloaded points of a generated set) with about 40 indices overwritten: bad points at 0, the last
    index, both sides of 255/256 and of a wave boundary (63/64), two adjacent ones, and random places; on the
    Weierstrass curves also records flagged as infinity that carry junk coordinates below p.
    -> (points, planted indices)"""
    params = P.CURVES[label]
    p = params["modulus"]
    rng = random.Random(seed)
    n = len(good)
    pts = [dict(q) for q in good]
    bad = bad_points(label, rng)
    where = [0, n - 1, 255, 256, 63, 64, 1000, 1001, n // 2, n - 2]
    while len(where) < 40:
        i = rng.randrange(n)
        if i not in where:
            where.append(i)
    for k, i in enumerate(where):
        pts[i] = dict(bad[k % len(bad)])
    if params["kind"] == "weierstrass":
        for i in (where[10], where[11], where[12]):   # three of the random places
            pts[i] = pt(rng.randrange(p), rng.randrange(p), True)
    return pts, sorted(where)


def encode(params, pts, montgomery=False):
    """-> (x || y bytes, infinity flags or None)"""
    p, fb = params["modulus"], params["fe_bytes"]
    r = (1 << (8 * fb)) if montgomery else 1
    data = b"".join((q["x"] * r % p).to_bytes(fb, "little") + (q["y"] * r % p).to_bytes(fb, "little") for q in pts)
    inf = bytes(1 if q["isZero"] else 0 for q in pts)
    return data, (inf if any(inf) else None)


def summary(verdicts, first=0):
    """(off_curve, off_subgroup, first_bad) of a list of verdict bytes that starts at set index `first`"""
    bad = [i for i, v in enumerate(verdicts) if v]
    return (sum(1 for v in verdicts if v & OFF_CURVE), sum(1 for v in verdicts if v & OFF_SUBGROUP),
            first + bad[0] if bad else NO_INDEX)
