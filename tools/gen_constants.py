#!/usr/bin/env python3
"""Generate msm_zprize_amd/csrc/constants_gen.h from msm_zprize_amd/curves.py.

This is the build-time analogue of the reference's module init:
`montgomeryParams` (bigint/field-util.ts:18-41), the constants `createMsmField` writes into
wasm memory (field-msm.ts:165-177: p, R, R^2, ...) and the GLV lattice basis `glvGeneral` bakes
into the scalar module (wasm/glv.ts:45-63, glv/glv.ts:21-50).  Limbs are 32-bit words of the
64-bit-limb little-endian layout (6x64 for 377/381-bit fields, 4x64 for 255-bit fields).

Run:  python tools/gen_constants.py   (output is committed; the build does not need Python)
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("curves", os.path.join(ROOT, "msm_zprize_amd", "curves.py"))
curves = importlib.util.module_from_spec(spec)
spec.loader.exec_module(curves)


def limbs(x, n):
    assert 0 <= x < (1 << (32 * n)), (hex(x), n)
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def arr(name, vals):
    body = ", ".join("0x%08xu" % v for v in vals)
    return "  static constexpr uint32_t %s[%d] = {%s};" % (name, len(vals), body)


def egcd_stop_early(l, p):
    """Truncated EGCD lattice basis (same construction as glv/glv.ts:21-50)."""
    r0, r1, t0, t1 = p, l, 0, 1
    while r1 * r1 > p:
        qt = r0 // r1
        r0, r1 = r1, r0 - qt * r1
        t0, t1 = t1, t0 - qt * t1
    qt = r0 // r1
    r2, t2 = r0 - qt * r1, t0 - qt * t1
    v00, v10 = r1, -t1
    if max(r0, abs(t0)) <= max(r2, abs(t2)):
        v01, v11 = r0, -t0
    else:
        v01, v11 = r2, -t2
    return (v00, v01), (v10, v11)


def tdiv(a, b):
    qt = abs(a) // abs(b)
    return qt if (a >= 0) == (b >= 0) else -qt


def glv_device_constants(q, lam):
    """Constants for the device decomposition:
         x_j = sign(m_j) * round(|m_j| * s / 2^256),  m0 = 2^256 * (-v11) / det, m1 = 2^256 * v10 / det
         s0 = s + v00*x0 + v01*x1,   s1 = v10*x0 + v11*x1
    """
    (v00, v01), (v10, v11) = egcd_stop_early(lam, q)
    det = v00 * v11 - v10 * v01
    assert abs(det) == q
    assert (v00 + lam * v10) % q == 0 and (v01 + lam * v11) % q == 0
    m0 = tdiv((1 << 256) * -v11, det)
    m1 = tdiv((1 << 256) * v10, det)
    sg = lambda x: 1 if x >= 0 else -1
    for v in (v00, v01, v10, v11):
        assert abs(v) < (1 << 128)
    assert abs(m0) < (1 << 160) and abs(m1) < (1 << 160)
    return dict(v=(v00, v01, v10, v11), m=(m0, m1),
                # sign of the product v_ij * x_j
                sgn=(sg(v00) * sg(m0), sg(v01) * sg(m1), sg(v10) * sg(m0), sg(v11) * sg(m1)))


def glv_proven_bits(q, c):
    """Analytic bound on the halves, the counterpart of maxS0 / maxS1 of the reference (src/wasm/glv.ts:216-226), in
    exact rational arithmetic.  The real solution of  V x = (-s, 0)  is x*_0 = -s v11 / det, x*_1 = s v10 / det.  The
    device computes x_j = round(|m_j| s / 2^256) with m_j = trunc(2^256 (-v11 | v10) / det): the truncation moves
    m_j by less than 1, hence x_j by less than s / 2^256 < q / 2^256, and the rounding by at most 1/2, so
        |x_j - x*_j| < E = 1/2 + q / 2^256,
        |s0| = |v00 e0 + v01 e1| < (|v00| + |v01|) E,   |s1| < (|v10| + |v11|) E.
    Returns the bit length that bound implies (so |s_j| < 2^bits for EVERY scalar < q)."""
    from fractions import Fraction
    import math
    v00, v01, v10, v11 = c["v"]
    E = Fraction(1, 2) + Fraction(q, 1 << 256)
    bound = max((abs(v00) + abs(v01)) * E, (abs(v10) + abs(v11)) * E)
    return int(math.ceil(bound)).bit_length()


def glv_decompose_model(s, q, lam, c):
    """Integer model of the device kernel (used to bound |s_i| and as a self-check)."""
    v00, v01, v10, v11 = c["v"]
    m0, m1 = c["m"]
    sg = lambda x: 1 if x >= 0 else -1
    rnd = lambda x: (x >> 256) + ((x >> 255) & 1)
    x0 = sg(m0) * rnd(abs(m0) * s)
    x1 = sg(m1) * rnd(abs(m1) * s)
    return s + v00 * x0 + v01 * x1, v10 * x0 + v11 * x1


def limbs_w(x, n, w):
    assert 0 <= x < (1 << (w * n)), (hex(x), n, w)
    return [(x >> (w * i)) & ((1 << w) - 1) for i in range(n)]


def iarr(name, vals):
    body = ", ".join(str(v) for v in vals)
    return "  static constexpr int32_t %s[%d] = {%s};" % (name, len(vals), body)


def iarr2(name, rows):
    body = ",\n".join("    {%s}" % ", ".join(str(v) for v in r) for r in rows)
    return "  static constexpr int32_t %s[%d][%d] = {\n%s};" % (name, len(rows), len(rows[0]), body)


SQRT_WINDOW = 4   # bits per digit of the discrete logarithm (sqrt.h); fields with a smaller 2-adicity use that


def sliding_schedule(e, w=3):
    """e > 0 as a left-to-right sliding-window schedule over the odd powers 1, 3, .. 2^w - 1: entries (squarings, index)
    = "square that many times, then multiply by x^(2 index + 1)"; index 2^(w-1) = no product (trailing zero bits).  The
    first entry starts the accumulator at its power."""
    bits = bin(e)[2:]
    out, pend, i = [], 0, 0
    while i < len(bits):
        if bits[i] == "0":
            pend, i = pend + 1, i + 1
            continue
        j = min(i + w, len(bits))
        while bits[j - 1] == "0":
            j -= 1
        out.append((pend + (j - i), (int(bits[i:j], 2) - 1) // 2))
        pend, i = 0, j
    if pend:
        out.append((pend, 1 << (w - 1)))
    return out


def run_schedule(sched, x, p, w=3):
    acc = None
    for sq, idx in sched:
        if acc is None:
            acc = pow(x, 2 * idx + 1, p)
            continue
        acc = pow(acc, 1 << sq, p)
        if idx < (1 << (w - 1)):
            acc = acc * pow(x, 2 * idx + 1, p) % p
    return acc


def sqrt_constants(p):
    """The tables of fe_sqrt (sqrt.h): Tonelli-Shanks with the discrete logarithm in the 2^S-th roots of unity taken by
    C-bit digits.  p - 1 = 2^S t, w = g^t for a non-residue g, NWIN = ceil(S / C) digits.  The logarithm e is handled as
    E = e << DELTA, DELTA = C NWIN - S, so that every digit of E is C bits wide and the short one is at the bottom (its
    low DELTA bits are zero).  INV[k][d] = w^-((d << C (NWIN-1-k)) >> DELTA); KEY[d] identifies zeta^d, zeta = w^(2^(S-C))
    the primitive 2^C-th root, by the low word of its canonical Montgomery residue."""
    S = ((p - 1) & -(p - 1)).bit_length() - 1
    t = (p - 1) >> S
    C = min(SQRT_WINDOW, S)
    NWIN = -(-S // C)
    DELTA = C * NWIN - S
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    assert pow(g, (p - 1) // 2, p) == p - 1, "the non-residue used is one"
    w = pow(g, t, p)
    assert pow(w, 1 << (S - 1), p) == p - 1, "w has order exactly 2^S"
    winv = pow(w, -1, p)
    inv = [[pow(winv, (d << (C * (NWIN - 1 - k))) >> DELTA, p) for d in range(1 << C)] for k in range(NWIN)]
    for k in range(NWIN):
        for d in range(1 << C):
            assert inv[k][d] * pow(w, (d << (C * (NWIN - 1 - k))) >> DELTA, p) % p == 1, "every entry is what its index says"
    zeta = pow(w, 1 << (S - C), p)
    roots = [pow(zeta, d, p) for d in range(1 << C)]
    assert roots[1 << (C - 1)] == p - 1 and len(set(roots)) == 1 << C
    assert all(inv[0][d] * roots[d] % p == 1 for d in range(1 << C))
    e = (t - 1) // 2
    sched = sliding_schedule(e)
    assert all(sq < 256 for sq, _ in sched) and sched[0][1] < 4
    return dict(S=S, t=t, C=C, NWIN=NWIN, DELTA=DELTA, g=g, w=w, inv=inv, roots=roots, e=e, sched=sched)


def sqrt_model(a, p, k):
    """Integer model of fe_sqrt, step for step (self-check of the tables and of the window arithmetic)."""
    C, NWIN, DELTA = k["C"], k["NWIN"], k["DELTA"]
    u = run_schedule(k["sched"], a, p) if a % p else 0
    r = u * a % p
    v = u * r % p
    if a % p == 0:
        return 0
    E = 0
    for lo, hi in ((0, NWIN // 2), (NWIN // 2, NWIN)):
        xs = {}
        y = pow(v, 1 << (C * (NWIN - hi)), p) if hi > lo else v
        for i in range(hi - 1, lo - 1, -1):
            xs[i] = y
            y = pow(y, 1 << C, p)
        for i in range(lo, hi):
            y = xs[i]
            for j in range(i):
                y = y * k["inv"][i - j][(E >> (C * j)) & ((1 << C) - 1)] % p
            E |= k["roots"].index(y) << (C * i)
    if (E >> DELTA) & 1:
        return None
    H = E >> 1
    for j in range(NWIN):
        r = r * k["inv"][NWIN - 1 - j][(H >> (C * j)) & ((1 << C) - 1)] % p
    return r


def sqrt_products(k):
    """field products of one fe_sqrt, squarings counted as products, from the loop bounds of sqrt.h"""
    C, NWIN = k["C"], k["NWIN"]
    power = 4 + sum(sq for sq, _ in k["sched"][1:]) + sum(1 for _, i in k["sched"][1:] if i < 4)
    chain = 0
    for lo, hi in ((0, NWIN // 2), (NWIN // 2, NWIN)):
        if hi > lo:
            chain += C * (NWIN - hi) + C * (hi - 1 - lo)
    return power + 2 + chain + NWIN * (NWIN - 1) // 2 + NWIN


def field_struct(name, p, nwords, N, W, extra=(), rng=None):
    """Base-field constants.  Arithmetic radix is 2^W with N signed lazy limbs (R = 2^(N*W));
    the memory format is `nwords` saturated 32-bit words (= nwords/2 64-bit limbs, little endian)."""
    R = 1 << (N * W)
    assert R > (1 << 6) * p, "need headroom for lazy values"
    assert 3 * p < (1 << (32 * nwords)), "memory format must hold lazy values < 3p"
    pinv = pow(p, -1, 1 << W)
    PL = limbs_w(p, N, W)
    out = ["struct %s {" % name,
           "  static constexpr int N = %d;    // limbs in registers" % N,
           "  static constexpr int W = %d;    // bits per limb" % W,
           "  static constexpr int NW = %d;   // 32-bit words in memory (%d x 64-bit limbs)" % (nwords, nwords // 2),
           "  static constexpr int BITS = %d;" % p.bit_length(),
           iarr("PL", PL),
           iarr("NPL", [-v for v in PL]),
           "  static constexpr uint32_t PINV = 0x%08xu;  // p^-1 mod 2^W" % pinv,
           arr("PW", limbs(p, nwords)),
           iarr("ONE", limbs_w(R % p, N, W)),          # Montgomery form of 1
           iarr("R2", limbs_w(R * R % p, N, W)),       # to-Montgomery factor
           iarr("R3", limbs_w(R * R * R % p, N, W)),   # fixes up a plain inverse of a Montgomery value
           iarr("P2", limbs_w(2 * p, N, W)),
           iarr("P4", limbs_w(4 * p, N, W)),
           # imported 64-bit-limb Montgomery coordinates v * R_std, R_std = 2^(32 nwords): one product with
           # R^2 / R_std takes them to v * R, as R2 takes canonical ones
           iarr("R2STD", limbs_w(R * R * pow(1 << (32 * nwords), -1, p) % p, N, W)),
           # ... and the way out (export_kernels.h): one product of a resident v * R with R_std leaves v * R_std
           iarr("RSTD", limbs_w((1 << (32 * nwords)) % p, N, W))]
    for nm, val in extra:
        out.append(iarr(nm, limbs_w(val * R % p, N, W)))
    # square roots (sqrt.h) and the sign of a compressed coordinate
    k = sqrt_constants(p)
    for a in [0, 1, 4, p - 1, k["g"]] + [rng.randrange(p) for _ in range(200)] + \
            [pow(k["w"], (1 << (k["S"] - j)) % (1 << k["S"]), p) * pow(rng.randrange(1, p), 1 << (k["S"] + 1), p) % p for j in range(k["S"] + 1)]:
        r = sqrt_model(a, p, k)
        assert (r is None) == (a % p != 0 and pow(a, (p - 1) // 2, p) == p - 1), hex(a)
        assert r is None or r * r % p == a % p, hex(a)
    keys = [(v * R % p) & 0xFFFFFFFF for v in k["roots"]]
    assert len(set(keys)) == len(keys) and 0 not in keys, "the low word tells the 2^C-th roots apart (and from zero)"
    out += ["  static constexpr int SQRT_S = %d;      // p - 1 = 2^SQRT_S * t, t odd" % k["S"],
            "  static constexpr int SQRT_C = %d;      // bits per digit of the discrete logarithm" % k["C"],
            "  static constexpr int SQRT_N = %d;      // digits: ceil(SQRT_S / SQRT_C)" % k["NWIN"],
            "  static constexpr int SQRT_DELTA = %d;  // SQRT_C * SQRT_N - SQRT_S: the logarithm is kept shifted left by this" % k["DELTA"],
            "  static constexpr int SQRT_PRODUCTS = %d;  // field products of one fe_sqrt (squarings included), from its loop bounds" % sqrt_products(k),
            "  static constexpr int SQRT_SCHED_LEN = %d;  // sliding-window schedule of a^((t - 1) / 2): (squarings, odd-power index; 4 = none)" % len(k["sched"]),
            "  static constexpr uint8_t SQRT_SCHED[%d] = {%s};" % (2 * len(k["sched"]), ", ".join("%d, %d" % e for e in k["sched"])),
            "  // SQRT_INV[k * 2^C + d] = w^-((d << C (N-1-k)) >> DELTA), w = %d^t of order 2^S; Montgomery limbs" % k["g"],
            iarr2("SQRT_INV", [limbs_w(v * R % p, N, W) for row in k["inv"] for v in row]),
            "  // low word of the canonical Montgomery residue of zeta^d, zeta = w^(2^(S-C)): distinct, non-zero (asserted)",
            arr("SQRT_KEY", keys),
            arr("PHALF1", limbs((p + 1) // 2, nwords)) + "  // (p + 1) / 2: a canonical value >= this is the 'larger' root"]
    out.append("};")
    return "\n".join(out)


# multiplicative generators of the scalar fields as arkworks (bls12-377, ed-on-bls12-377), pasta_curves and bls12_381 use
NTT_GENERATOR = {"bls12-377": 22, "pallas": 5, "bls12-381": 7, "ed-on-bls12-377": 5}


def main():
    import random
    rng = random.Random(1234)
    L = ["// GENERATED by tools/gen_constants.py -- do not edit.",
         "// Field / curve / GLV constants for the MSM kernels (32-bit words of 64-bit-limb LE layout).",
         "#pragma once", "#include <cstdint>", "", "namespace msmz {", ""]
    for c in curves.ALL_CURVES:
        p, q = c["modulus"], c["order"]
        n = c["fe_bytes"] // 4
        tag = {"bls12-377": "Bls377", "pallas": "Pallas", "bls12-381": "Bls381", "ed-on-bls12-377": "Ed377"}[c["label"]]
        R = 1 << (32 * n)
        extra = [("GX", c["generator"]["x"]), ("GY", c["generator"]["y"])]
        if c["kind"] == "weierstrass":
            extra += [("B", c["b"]), ("B3", 3 * c["b"] % p), ("BETA", c["endomorphism"]["beta"])]
        else:
            extra += [("D", c["d"]), ("K2D", 2 * c["d"] % p)]
            # decompression divides by d y^2 + 1 (TeGroup::decompress): never zero, as -1/d is a non-residue
            assert pow(c["d"], (p - 1) // 2, p) == p - 1, "d must be a quadratic non-residue"
            assert pow(p - 1, (p - 1) // 2, p) == 1, "-1 must be a quadratic residue"
        L.append("// %s base field: p = 0x%x" % (c["label"], p))
        N, W = {12: (14, 28), 8: (9, 29)}[n]
        L.append(field_struct(tag + "Fp", p, n, N, W, extra, rng))
        L.append("")
        # scalar field
        L.append("struct %sFr {" % tag)
        L.append("  static constexpr int BITS = %d;" % q.bit_length())
        L.append(arr("Q", limbs(q, 8)))
        L.append("  static constexpr uint32_t QINV32 = 0x%08xu;  // -q^-1 mod 2^32 (fr_from_mont, scalar.h)" % ((-pow(q, -1, 1 << 32)) % (1 << 32)))
        L.append(arr("R2", limbs(pow(2, 512, q), 8)) + "   // 2^512 mod q: fr_mont_mul by it multiplies by 2^256 (fr.h)")
        L.append(arr("ONE", limbs(pow(2, 256, q), 8)) + "  // 2^256 mod q: the Montgomery form of 1")
        # 2-adic roots of unity (ntt_kernels.h): S = the 2-adicity of q - 1, W = G^((q - 1) / 2^S) for the multiplicative
        # generator G the common libraries use; W has order exactly 2^S iff G is a quadratic non-residue
        G = NTT_GENERATOR[c["label"]]
        S = ((q - 1) & -(q - 1)).bit_length() - 1
        assert pow(G, (q - 1) // 2, q) == q - 1, "the NTT generator must be a quadratic non-residue"
        W = pow(G, (q - 1) >> S, q)
        assert pow(W, 1 << (S - 1), q) == q - 1
        L.append("  static constexpr int TWO_ADICITY = %d;  // q - 1 = 2^TWO_ADICITY * odd: the longest transform is 2^TWO_ADICITY (ntt_kernels.h)" % S)
        L.append(arr("ROOT_MAX", limbs(W, 8)) + "  // %d^((q - 1) / 2^TWO_ADICITY): a primitive 2^TWO_ADICITY-th root of unity, canonical" % G)
        L.append("  static constexpr bool PRIME_ORDER = %s;  // true iff the cofactor is 1, i.e. the whole curve is the subgroup (check_kernels.h)" % ("true" if c["cofactor"] == 1 else "false"))
        if c["kind"] == "weierstrass":
            lam = c["endomorphism"]["lambda_"]
            g = glv_device_constants(q, lam)
            mx = 0
            samples = [0, 1, 2, q - 1, q - 2, q // 2, q // 3, lam, lam + 1, q - lam] + [rng.randrange(q) for _ in range(20000)]
            for s in samples:
                s0, s1 = glv_decompose_model(s, q, lam, g)
                assert (s0 + s1 * lam - s) % q == 0
                mx = max(mx, abs(s0), abs(s1))
            assert mx < (1 << 127), mx.bit_length()
            proven = glv_proven_bits(q, g)
            assert mx.bit_length() <= proven <= 128, (mx.bit_length(), proven)   # 4-word halves can never truncate
            L.append("  static constexpr bool HAS_GLV = true;")
            L.append("  static constexpr int GLV_BITS = 128;  // windows cover GLV_BITS bits: halves below 2^127 (observed: %d bits) never overflow them" % mx.bit_length())
            L.append("  static constexpr int GLV_PROVEN_BITS = %d;  // analytic bound (tools/gen_constants.py glv_proven_bits; cf. src/wasm/glv.ts:216-226): |s0|, |s1| < 2^%d for every scalar" % (proven, proven))
            L.append("  static constexpr int GLV_TYP_BITS = %d;  // bit length of the largest half seen in 20000 samples (bucket-balance heuristic only)" % mx.bit_length())
            v00, v01, v10, v11 = g["v"]
            L.append(arr("GLV_V00", limbs(abs(v00), 4)))
            L.append(arr("GLV_V01", limbs(abs(v01), 4)))
            L.append(arr("GLV_V10", limbs(abs(v10), 4)))
            L.append(arr("GLV_V11", limbs(abs(v11), 4)))
            L.append(arr("GLV_M0", limbs(abs(g["m"][0]), 5)))
            L.append(arr("GLV_M1", limbs(abs(g["m"][1]), 5)))
            L.append("  // sign (+1 -> 0, -1 -> 1) of the products v00*x0, v01*x1, v10*x0, v11*x1")
            L.append("  static constexpr uint32_t GLV_NEG[4] = {%s};" % ", ".join("1u" if s < 0 else "0u" for s in g["sgn"]))
            L.append(arr("LAMBDA", limbs(lam, 8)))
        else:
            L.append("  static constexpr bool HAS_GLV = false;")
            L.append("  static constexpr int GLV_BITS = 0;")
            L.append("  static constexpr int GLV_PROVEN_BITS = 0;")
            L.append("  static constexpr int GLV_TYP_BITS = 0;")
        L.append("};")
        L.append("")
    L.append("}  // namespace msmz")
    path = os.path.join(ROOT, "msm_zprize_amd", "csrc", "constants_gen.h")
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
