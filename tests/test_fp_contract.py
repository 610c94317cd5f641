"""The lazy-limb contract of csrc/fp.h, checked on every call: tests/native/fp_contract_test.cpp compiles fp.h and
curve.h for the host with traced field types, so each fe_mul / fe_sqr / fe_reduce_small / fe_store / fe_store_mulout /
fe_is_zero inside the curve formulas checks its operands against the documented bounds (value, and the limb-product
condition N*A*B + N*2^(2W) < 2^63) and its output against the range it claims.  The formulas run on adversarial
operands -- memory residues lifted anywhere in [0, 3p), accumulators rescaled by random lambda, both operands of P + P and
P + (-P) in different representations, long chains that feed every output back in -- and the results are compared with
oracle/bigint_ref.py.  The driver is built twice, with MSMZ_FE_ILP = 0 and 1.  Each run prints the worst value/p, limb
magnitude and product margin seen at every call site next to the bound (run pytest with -s to see the table).

Worst cases observed (formulas = the curve formulas on the operands below and the 10^4-step chains; edges = the raw
limb cases of oracle/lazy_limbs.py; both builds):
  routine               documented bound                          formulas                         edges
  mul / sqr input       |v| < 32p (8p for the 255-bit fields)     5.9p (6.7p), limbs <= 2^W          32p - 1 (8p - 1)
  mul / sqr limbs       N*A*B + N*2^(2W) < 2^63                   2^60.8 (2^62.2)                    2^63 - 2^33
  mul / sqr output      (-1.5p, 0.5p)                             [-1.02p, 0.23p]                    [-1.18p, 0.32p]
  reduce_small / store  |v| < 16p -> [0, 3p)                      3.9p -> [p, 2p]                    16p - 1 -> [p, 2p]
  store_mulout          (-1.5p, 0.5p) -> [0, 3p)                  --                                 both ends -> (0.5p, 2.5p)
  is_zero               |v| < 16p                                 3.9p                               15p, limbs to 2^31
The 255-bit fields' xyzz_mdbl squared 2y uncarried (limbs to 2^(W+1), 9 * 2^60 > 2^63); it now carries like xyzz_dbl.

Mutation record (each applied alone to curve.h / fp.h; "old" = tests/test_fp_host.py, the CPU suite before this file):
  caught here          xyzz_madd / xyzz_add carry of X3; xyzz_dbl carries of U, t and xyzz_carry; xyzz_mdbl carries
                       of U, M, t; te_add / te_madd carry of G; fe_reduce_small quotient "- 0" (old too) and "- 2";
                       fe_is_zero filter 15u -> 14u / 16u and 30u -> 29u; fe_store_mulout without P2 (old too);
                       xyzz_dbl carry of M (old too)
  equivalent           every other carry of xyzz_madd (P, R, t, r.Y), xyzz_add (t, r.Y), xyzz_mdbl (xyzz_carry),
                       te_add and te_madd: with the carry removed, every call the harness checks stays in contract --
                       worst N*A*B + N*2^(2W) = 2^60.81 (377/381-bit) / 2^62.75 (255-bit), limbs <= 2^(W+1),
                       |v| <= 6.72p -- because each operand it leaves uncarried is the sum or difference of two
                       normalized values; fe_is_zero 30u -> 31u only sends one more residue class to the full
                       reduction, which answers it exactly
CPU only."""
import os
import random
import subprocess

import pytest

from oracle import bigint_ref as B
from oracle import lazy_limbs as LZ
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fp_contract_test.cpp")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("fp.h", "curve.h", "test_ops.h", "constants_gen.h")]
CURVES = ["bls12-377", "bls12-381", "pallas", "ed-on-bls12-377"]
CHAIN_STEPS = 10000


def build_driver(ilp):
    exe = os.path.join(ROOT, "tests", "native", f"fp_contract_test{'_ilp' if ilp else ''}")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", f"-DMSMZ_FE_ILP={ilp}", "-o", exe, SRC])
    return exe


def run_driver(exe, lines):
    """one output line per command; a broken bound makes the driver exit 1 with the violations on stderr"""
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-6000:]
    out = r.stdout.split("\n")[:len(lines)]
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module", params=[0, 1], ids=["single_chain", "ilp"])
def driver(request):
    exe = build_driver(request.param)
    return lambda lines: run_driver(exe, lines)


# ------------------------------------------------------------------------------------------------ operand builders
class Field:
    def __init__(self, label):
        self.label = label
        self.name = LZ.DRIVER_NAME[label]
        self.p, self.n, self.w = LZ.FIELDS[label]
        self.R = 1 << (self.n * self.w)
        self.top = 3 * self.p   # memory residues as the kernels write them: [0, 3p) (fp.h)

    def mont(self, x):
        return x * self.R % self.p

    def lift(self, x, rng):
        """a memory-format residue of the class x: x + k p anywhere in [0, top)"""
        v = x % self.p + self.p * rng.randrange(0, (self.top - x % self.p - 1) // self.p + 1)
        assert v < self.top
        return f"{v:x}"

    def mem(self, x, rng):
        return self.lift(self.mont(x), rng)


def _curve(label):
    params = P.CURVES[label]
    return B.TwistedEdwards(params) if params["kind"] == "twisted-edwards" else B.AffineWeierstrass(params)


def _points(label, rng, k):
    c = _curve(label)
    pts = []
    for _ in range(k):
        q = c.scale(rng.randrange(1, c.q), c.one)
        pts.append(c.to_affine(q) if isinstance(c, B.TwistedEdwards) else q)
    return c, pts


def xyzz(f, pt, rng, lam=None):
    """XYZZ accumulator of an affine point (x, y, inf): X = x l^2, Y = y l^3, ZZ = l^2, ZZZ = l^3, lifted"""
    lam = lam or rng.randrange(1, f.p)
    if pt[2]:
        return [f.mem(rng.randrange(f.p), rng), f.mem(rng.randrange(f.p), rng), f.lift(0, rng), f.lift(0, rng)]
    l2, l3 = lam * lam % f.p, lam ** 3 % f.p
    return [f.mem(pt[0] * l2, rng), f.mem(pt[1] * l3, rng), f.mem(l2, rng), f.mem(l3, rng)]


def te_ext(f, pt, rng, lam=None):
    """extended twisted-Edwards point of affine (x, y): (x l, y l, l, x y l), lifted"""
    lam = lam or rng.randrange(1, f.p)
    x, y = pt
    return [f.mem(x * lam, rng), f.mem(y * lam, rng), f.mem(lam, rng), f.mem(x * y * lam, rng)]


def niels(f, c, pt, rng):
    x, y = pt
    return [f.mem(y - x, rng), f.mem(y + x, rng), f.mem(c.k * x * y, rng)]


def parse_w(s, c):
    if s == "INF":
        return c.zero
    x, y = s.split(":")
    return (int(x, 16), int(y, 16), False)


def parse_te(s):
    x, y = s.split(":")
    return (int(x, 16), int(y, 16))


def te_affine(c, P1, P2):
    return c.to_affine(c.add(c.from_affine(P1), c.from_affine(P2)))


def te_neg(c, pt):
    return ((-pt[0]) % c.p, pt[1])


# ------------------------------------------------------------------------------------------------ formulas
@pytest.mark.parametrize("label", CURVES[:3])
def test_xyzz_formulas_adversarial(driver, label):
    """xyzz_add / xyzz_dbl / xyzz_madd / xyzz_mdbl on lifted, rescaled operands; P + P and P + (-P) with a different
    lambda on each side; infinity on either side; madd with the negated record"""
    f = Field(label)
    rng = random.Random(LZ.DRIVER_NAME[label])
    c, pts = _points(label, rng, 12)
    lines, want = [], []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        for q in (b, a, c.negate(a), c.zero):   # P + Q, P + P, P + (-P), P + 0
            lines.append(f"{f.name} wadd {' '.join(xyzz(f, a, rng) + xyzz(f, q, rng))}"); want.append(c.add(a, q))
            lines.append(f"{f.name} wadd {' '.join(xyzz(f, q, rng) + xyzz(f, a, rng))}"); want.append(c.add(q, a))
        lines.append(f"{f.name} wadd {' '.join(xyzz(f, c.zero, rng) * 2)}"); want.append(c.zero)
        lines.append(f"{f.name} wdbl {' '.join(xyzz(f, a, rng))}"); want.append(c.double(a))
        lines.append(f"{f.name} wdbl {' '.join(xyzz(f, c.zero, rng))}"); want.append(c.zero)
        for neg in (0, 1):
            for q in (b, a, c.negate(a)):
                # the record holds q (or -q with neg = 1, negated in registers as load_affine does)
                rec = q if not neg else c.negate(q)
                lines.append(f"{f.name} wmadd {' '.join(xyzz(f, a, rng))} {f.mem(rec[0], rng)} {f.mem(rec[1], rng)} "
                             f"{neg} 0")
                want.append(c.add(a, q))
            lines.append(f"{f.name} wmadd {' '.join(xyzz(f, c.zero, rng))} {f.mem(b[0], rng)} {f.mem(b[1], rng)} 0 0")
            want.append(b)
            lines.append(f"{f.name} wmadd {' '.join(xyzz(f, a, rng))} 0 0 {neg} 1")
            want.append(a)
            rec = a if not neg else c.negate(a)
            lines.append(f"{f.name} wmdbl {f.mem(rec[0], rng)} {f.mem(rec[1], rng)} {neg}")
            want.append(c.double(a))
    # regression: a y whose low limbs are all 2^W - 1, so 2y has every low limb at 2^(W+1) - 2 (xyzz_mdbl once
    # squared it uncarried, beyond the limb-product bound of the 255-bit fields)
    low = (1 << (f.w * (f.n - 1))) - 1
    for ymem in (low, low + (f.top - 1 - low) // (low + 1) * (low + 1)):
        y = ymem * pow(f.R, -1, f.p) % f.p
        x = pts[0][0]
        lines.append(f"{f.name} wmdbl {f.mem(x, rng)} {ymem:x} 0"); want.append(c.double((x, y, False)))
    got = driver(lines)
    for l, g, w in zip(lines, got, want):
        assert parse_w(g, c) == w, l


def test_te_formulas_adversarial(driver):
    """te_add / te_madd (neg 0 and 1) on lifted extended points with Z != 1; P + P and P + (-P) with a different
    lambda on each side; the identity on either side"""
    label = "ed-on-bls12-377"
    f = Field(label)
    rng = random.Random(5)
    c, pts = _points(label, rng, 12)
    ident = (0, 1)
    lines, want = [], []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        for q in (b, a, te_neg(c, a), ident):
            lines.append(f"{f.name} tadd {' '.join(te_ext(f, a, rng) + te_ext(f, q, rng))}"); want.append(te_affine(c, a, q))
            lines.append(f"{f.name} tadd {' '.join(te_ext(f, q, rng) + te_ext(f, a, rng))}"); want.append(te_affine(c, q, a))
            for neg in (0, 1):
                rec = q if not neg else te_neg(c, q)
                lines.append(f"{f.name} tmadd {' '.join(te_ext(f, a, rng) + niels(f, c, rec, rng))} {neg}")
                want.append(te_affine(c, a, q))
        lines.append(f"{f.name} tmadd {' '.join(te_ext(f, ident, rng) + niels(f, c, b, rng))} 0"); want.append(b)
    got = driver(lines)
    for l, g, w in zip(lines, got, want):
        assert parse_te(g) == w, l


def _chain_ops(rng, steps, every):
    ops = []
    for i in range(1, steps + 1):
        ops.append(rng.choices("mnabdes", weights=[35, 15, 10, 5, 20, 3, 7])[0])
        if i % every == 0:
            ops.append("p")
    return "".join(ops)


@pytest.mark.parametrize("label", CURVES)
def test_long_chains(driver, label):
    """CHAIN_STEPS madd / add / dbl steps in registers, each output fed back in, with occasional trips through memory:
    the output ranges of the formulas must be a fixed point of the chain (checked at every call by the driver)"""
    f = Field(label)
    rng = random.Random(100 + CURVES.index(label))
    c, pts = _points(label, rng, 8)
    A, Bacc = pts[0], pts[1]
    base = pts[2:]
    ops = _chain_ops(rng, CHAIN_STEPS, 500)
    te = isinstance(c, B.TwistedEdwards)
    if te:
        args = te_ext(f, A, rng) + te_ext(f, Bacc, rng) + [str(len(base))] + sum((niels(f, c, q, rng) for q in base), [])
        add, neg = (lambda u, v: te_affine(c, u, v)), (lambda u: te_neg(c, u))
    else:
        args = xyzz(f, A, rng) + xyzz(f, Bacc, rng) + [str(len(base))] + sum(([f.mem(q[0], rng), f.mem(q[1], rng)] for q in base), [])
        add, neg = c.add, c.negate
    line = f"{f.name} {'tchain' if te else 'wchain'} {ops} {' '.join(args)}"
    want, j = [], 0
    for o in ops:
        if o in "mn":
            q = base[j % len(base)]
            A = add(A, q if o == "m" else neg(q))
            j += 1
        elif o == "a":
            A = add(A, Bacc)
        elif o == "b":
            Bacc = add(Bacc, A)
        elif o in "de":
            A = add(A, A)
        elif o == "p":
            want.append(A)
    got = driver([line])[0].split()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (parse_te(g) if te else parse_w(g, c)) == w, f"checkpoint {i}"


@pytest.mark.parametrize("label", CURVES)
def test_inverse_lazy_inputs(driver, label):
    """fe_inverse of lazy inputs anywhere in |v| < 16p (it canonicalizes through fe_store first)"""
    f = Field(label)
    rng = random.Random(9)
    lines, want = [], []
    for name, limbs in LZ.reduce_cases(label)[::5]:
        v = LZ.value(limbs, f.w)
        lines.append(f"{f.name} inv L{','.join(map(str, limbs))}")
        want.append("ZERO" if v % f.p == 0 else f.R * f.R * pow(v, -1, f.p) % f.p)
    for _ in range(20):
        x = rng.randrange(1, f.p)
        lines.append(f"{f.name} inv {f.lift(x, rng)}"); want.append(f.R * f.R * pow(x, -1, f.p) % f.p)
    got = driver(lines)
    for l, g, w in zip(lines, got, want):
        assert (g if g == "ZERO" else int(g, 16)) == w, l


# ------------------------------------------------------------------------------------------------ field routines on raw limbs
def field_limb_lines(label):
    """driver commands for the shared edge cases of oracle/lazy_limbs.py (the device test feeds the same limbs)"""
    cases = LZ.field_limb_cases(label)
    name = LZ.DRIVER_NAME[label]
    return [f"{name} fl {op} L{','.join(map(str, a))} L{','.join(map(str, b))}" for op, a, b in cases], cases


@pytest.mark.parametrize("label", CURVES)
def test_field_routines_on_raw_limbs(driver, label):
    """fe_mul / fe_sqr at +-(bound p - 1) with limbs at the product limit; fe_reduce_small / fe_store at k p - 1, k p,
    k p + 1 for k in [-16, 15] in three limb forms; fe_is_zero at k p, |k| <= 15, and its near misses; fe_store_mulout
    across (-1.5p, 0.5p); fe_carry / fe_normalize; fe_inverse -- the same cases tests/test_lazy_contract_gpu.py runs
    on the device"""
    lines, cases = field_limb_lines(label)
    got = driver(lines)
    for l, g, (op, a, b) in zip(lines, got, cases):
        raw, canon = g.split()
        raw = [int(x) for x in raw.split(",")]
        try:
            LZ.check_field_limb_result(label, op, a, b, raw, int(canon, 16))
        except AssertionError as e:
            raise AssertionError(f"{l} -> {g}") from e
