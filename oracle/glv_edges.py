"""Integer model of the device's GLV split (msm_zprize_amd/csrc/scalar.h glv_decompose) and the scalars at which that
routine can go wrong, for tests/test_glv_edges_cpu.py and tests/test_glv_edges_gpu.py.  Python integers and fractions
only.

The device computes, with the constants of tools/gen_constants.py glv_device_constants (one definition: imported),
    x_j = sgn(M_j) round(|M_j| s / 2^256)   (round half up: bits 256.. of the product plus bit 255),
    s0 = s + v00 x0 + v01 x1,   s1 = v10 x0 + v11 x1,
M_0 = trunc(2^256 (-v11) / det), M_1 = trunc(2^256 v10 / det), |det| = q.  `model` is that formula; it is NOT
oracle.bigint_ref.glv_decompose, which restates the reference's variant (s truncated before the product) and gives
other halves.

Where the halves can be long.  |M_j| = 2^256 |nu_j| / q - delta_j with nu = (-v11, v10) and delta_j in [0, 1) the
truncation; round(y) = y + rho with rho in (-1/2, 1/2].  So
    x_j = sgn_j (s |nu_j| / q - s delta_j / 2^256 + rho_j),
and sgn_j s |nu_j| / q is the real solution of V x = (-s, 0), which the lattice basis takes to (0, 0).  What is left is
    s0 = sum_j v0j sgn_j (rho_j - s delta_j / 2^256),   s1 = sum_j v1j sgn_j (rho_j - s delta_j / 2^256):
each half is linear in (rho_0, rho_1, s) over the box [-1/2, 1/2]^2 x [0, q], so its absolute value is largest at a
vertex.  `supremum` is that vertex maximum, in exact rationals.  It is an upper bound for every scalar below q and, for
a half whose dominant x_j has a full-length M_j, scalars come within 0.01 % of it (a threshold of that x_j next to
s = q); a tighter bound than glv_proven_bits' (|v| + |v|)(1/2 + q / 2^256), which ignores the signs of the deltas.

Edge scalars.  A THRESHOLD of x_j is thr = ceil((2k + 1) 2^255 / |M_j|): |x_j| is k at thr - 1 and k + 1 at thr.  At
a threshold the rounding bit decides the half; where k ends in 32, 64 or 96 one-bits the carry of the rounding ripples
through that many words of x_j.
"""
import importlib.util
import os
import random
import re
from fractions import Fraction

from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = ["bls12-377", "pallas", "bls12-381"]
TAGS = {"bls12-377": "Bls377", "pallas": "Pallas", "bls12-381": "Bls381"}
# |M_j| of a few bits (v11 or v10 is +-1): x_j has only a handful of thresholds, all of them are taken
FEW_THRESHOLDS = 64
SMALL_MAGNITUDES = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, (1 << 96) - 1, 1 << 96, 1 << 120]

_gen = None
_consts = {}


def _generator():
    global _gen
    if _gen is None:
        spec = importlib.util.spec_from_file_location("msmz_gen_constants", os.path.join(ROOT, "tools", "gen_constants.py"))
        _gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_gen)
    return _gen


def header_constants(label):
    """the GLV words, GLV_NEG and GLV_PROVEN_BITS of the curve's scalar field as msm_zprize_amd/csrc/constants_gen.h has
    them: {name: integer}, GLV_NEG as a tuple"""
    with open(os.path.join(ROOT, "msm_zprize_amd", "csrc", "constants_gen.h")) as f:
        text = f.read()
    body = re.search(r"struct %sFr \{(.*?)\n\};" % TAGS[label], text, re.S).group(1)
    out = {}
    for name, words in re.findall(r"uint32_t (GLV_[VM]\d+|GLV_NEG)\[\d+\] = \{([^}]*)\}", body):
        vals = [int(w.strip().rstrip("u"), 16 if "x" in w else 10) for w in words.split(",")]
        out[name] = tuple(vals) if name == "GLV_NEG" else sum(v << (32 * i) for i, v in enumerate(vals))
    out["GLV_PROVEN_BITS"] = int(re.search(r"int GLV_PROVEN_BITS = (\d+);", body).group(1))
    return out


def constants(label):
    """q, lambda and glv_device_constants of the curve; asserts once that the header holds the same words"""
    if label not in _consts:
        c = P.CURVES[label]
        q, lam = c["order"], c["endomorphism"]["lambda_"]
        g = _generator().glv_device_constants(q, lam)
        h = header_constants(label)
        v00, v01, v10, v11 = g["v"]
        want = dict(GLV_V00=abs(v00), GLV_V01=abs(v01), GLV_V10=abs(v10), GLV_V11=abs(v11), GLV_M0=abs(g["m"][0]),
                    GLV_M1=abs(g["m"][1]), GLV_NEG=tuple(1 if s < 0 else 0 for s in g["sgn"]))
        for name, v in want.items():
            assert h[name] == v, f"{label}: {name} of constants_gen.h is not the generator's"
        _consts[label] = dict(q=q, lam=lam, g=g, proven_bits=h["GLV_PROVEN_BITS"])
    return _consts[label]


def model(label, s):
    """(s0, s1), signed: the device formula on the integer s < q"""
    k = constants(label)
    return _generator().glv_decompose_model(s, k["q"], k["lam"], k["g"])


def x_magnitudes(label, s):
    """(|x_0|, |x_1|) of the device formula"""
    m0, m1 = constants(label)["g"]["m"]
    rnd = lambda x: (x >> 256) + ((x >> 255) & 1)
    return rnd(abs(m0) * s), rnd(abs(m1) * s)


def supremum(label):
    """(sup |s0|, sup |s1|) over the box of the module docstring, as Fractions"""
    k = constants(label)
    q = k["q"]
    v00, v01, v10, v11 = k["g"]["v"]
    m = k["g"]["m"]
    nu = (-v11, v10)
    sgn = [1 if x >= 0 else -1 for x in m]
    delta = [Fraction((1 << 256) * abs(nu[j]), q) - abs(m[j]) for j in range(2)]
    assert all(0 <= d < 1 for d in delta)
    out = []
    for row in ((v00, v01), (v10, v11)):
        best = Fraction(0)
        for r0 in (Fraction(-1, 2), Fraction(1, 2)):
            for r1 in (Fraction(-1, 2), Fraction(1, 2)):
                for s in (0, q):
                    e = [sgn[j] * (r - Fraction(s, 1 << 256) * delta[j]) for j, r in enumerate((r0, r1))]
                    best = max(best, abs(row[0] * e[0] + row[1] * e[1]))
        out.append(best)
    return tuple(out)


def k_max(label, j):
    """|x_j| of the largest scalar, q - 1: the thresholds below q are those of k < k_max"""
    return x_magnitudes(label, constants(label)["q"] - 1)[j]


def threshold(label, j, k):
    """the smallest s with |x_j| = k + 1"""
    m = abs(constants(label)["g"]["m"][j])
    return -(-((2 * k + 1) << 255) // m)


def _unique(values):
    return list(dict.fromkeys(values))


def threshold_ks(label, j, rng):
    """the k of the issue: the word boundaries, the last one, eight (r << w) - 1 per w and 20 random; every k where
    there are only a few"""
    top = k_max(label, j)
    if top <= FEW_THRESHOLDS:
        return list(range(top))
    ks = [0, 1, (1 << 32) - 1, (1 << 64) - 1, (1 << 96) - 1, top - 1]
    for w in (32, 64, 96):
        ks += [(rng.randrange(1, top >> w) << w) - 1 for _ in range(8)]
    ks += [rng.randrange(top) for _ in range(20)]
    assert all(0 <= k < top for k in ks)
    return _unique(ks)


def small_pairs(label):
    """(a, b, a + b lambda mod q) for a, b over +-SMALL_MAGNITUDES: 17 x 17 = 289 rows"""
    k = constants(label)
    signed = _unique([v for mag in SMALL_MAGNITUDES for v in (mag, -mag)])
    return [(a, b, (a + b * k["lam"]) % k["q"]) for a in signed for b in signed]


def corner_scalars(label):
    """the named scalars of tests/test_fp_host.py::test_glv_decompose and tests/test_stages_gpu.py::test_glv_decomposition"""
    k = constants(label)
    q, lam = k["q"], k["lam"]
    return _unique([0, 1, 2, q - 1, q - 2, lam, lam + 1, q - lam, q // 2, (1 << 128) - 1, 1 << 128, (lam + 1) % q, q // 3] +
                   [1 << b for b in range(0, 250, 13)])


def longest_ratio(label, s):
    """the larger of |s0| / sup |s0| and |s1| / sup |s1|, as a Fraction"""
    sup = supremum(label)
    s0, s1 = model(label, s)
    return max(Fraction(abs(s0)) / sup[0], Fraction(abs(s1)) / sup[1])


def threshold_cases(label, seed=1):
    """[(j, k, thr)]: the thresholds of edge_scalars, thr = threshold(label, j, k)"""
    rng = random.Random(2 * seed)
    return [(j, k, threshold(label, j, k)) for j in (0, 1) for k in threshold_ks(label, j, rng)]


def edge_scalars(label, seed=1):
    """{"thresholds", "ripple", "small", "longest", "corners"}: lists of scalars below q, each without repeats.
      thresholds  thr - 1 and thr for every row of threshold_cases
      ripple      the thresholds thr whose k + 1 ends in 32 or more zero bits (a subset of `thresholds`): the rounding
                  carry crosses a word of x_j there
      small       the scalars of small_pairs
      longest     of 20000 random threshold pairs (40000 scalars), the 64 whose larger half is the greatest fraction of
                  its supremum
      corners     corner_scalars"""
    k = constants(label)
    q = k["q"]
    rng = random.Random(2 * seed + 1)
    thresholds, ripple = [], []
    for j, kk, thr in threshold_cases(label, seed):
        assert 0 < thr < q
        thresholds += [thr - 1, thr]
        if (kk + 1) % (1 << 32) == 0:
            ripple.append(thr)
    # plain integers in the loop: the ratio to the supremum as a 64-bit fixed-point number
    v00, v01, v10, v11 = k["g"]["v"]
    m = [abs(x) for x in k["g"]["m"]]
    sg = [1 if x >= 0 else -1 for x in k["g"]["m"]]
    tops = [k_max(label, 0), k_max(label, 1)]
    sup = [int(x) + 1 for x in supremum(label)]
    scored = []
    for _ in range(20000):
        j = rng.randrange(2)
        thr = -(-((2 * rng.randrange(tops[j]) + 1) << 255) // m[j])
        for s in (thr - 1, thr):
            p0, p1 = m[0] * s, m[1] * s
            x0 = sg[0] * ((p0 >> 256) + ((p0 >> 255) & 1))
            x1 = sg[1] * ((p1 >> 256) + ((p1 >> 255) & 1))
            scored.append((max((abs(s + v00 * x0 + v01 * x1) << 64) // sup[0], (abs(v10 * x0 + v11 * x1) << 64) // sup[1]), s))
    scored.sort(reverse=True)
    longest = _unique(s for _, s in scored)[:64]
    out = dict(thresholds=_unique(thresholds), ripple=_unique(ripple), small=_unique(s for _, _, s in small_pairs(label)),
               longest=longest, corners=corner_scalars(label))
    for name, vals in out.items():
        assert all(0 <= s < q for s in vals), name
    return out


def edge_set(label, seed=1):
    """every edge scalar once, in the order thresholds, small, longest, corners"""
    e = edge_scalars(label, seed)
    return _unique(e["thresholds"] + e["small"] + e["longest"] + e["corners"])
