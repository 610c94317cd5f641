"""The yardstick of the multilinear tests (tests/test_mle_cpu.py, tests/test_mle_gpu.py, tests/test_js_mle.py,
tests/golden/make_mle_fixture.py): Python integers mod q over lists.  A polynomial in v variables is the list of its 2^v
values on the Boolean cube, entry i = f(b_0, .., b_(v-1)) with i = sum b_j 2^j -- variable 0 is the lowest index bit
(include/msmz.h)."""


def eq(point, q, scale=1):
    """the table of scale * eq(r, i), i < 2^len(point):  eq(r, i) = prod_j (b_j r_j + (1 - b_j)(1 - r_j))"""
    table = [scale % q]
    for r in point:   # variable j doubles the table: the new index bit is the highest so far
        table = [t * (1 - r) % q for t in table] + [t * r % q for t in table]
    return table


def eq_at(point, i, q):
    """one entry of the table, without the table (for a point of 31 variables)"""
    acc = 1
    for j, r in enumerate(point):
        acc = acc * (r if (i >> j) & 1 else 1 - r) % q
    return acc


def mle_eval(f, point, q):
    """f(r) = sum_i f_i eq(r, i)"""
    assert len(f) == 1 << len(point)
    return sum(a * b for a, b in zip(f, eq(point, q))) % q


def pairs(f, low):
    """the (lo, hi) pairs of one table: (f_i, f_(i+h)) for the high variable, (f_(2i), f_(2i+1)) for variable 0"""
    h = len(f) // 2
    assert h >= 1 and 2 * h == len(f)
    return [(f[2 * i], f[2 * i + 1]) for i in range(h)] if low else [(f[i], f[i + h]) for i in range(h)]


def bind(f, r, q, low=False):
    """one variable bound to r: out_i = lo + r (hi - lo)"""
    return [(lo + r * (hi - lo)) % q for lo, hi in pairs(f, low)]


def round_poly(tables, terms, q, low=False):
    """g(t) = sum_i sum_T c_T prod_(j in T) ((1 - t) lo_j + t hi_j), t = 0 .. d, for terms [(c or None, mask)] over equally
    long tables; d = the largest popcount of a mask"""
    d = max(bin(mask).count("1") for _, mask in terms)
    split = [pairs(f, low) for f in tables]
    out = []
    for t in range(d + 1):
        total = 0
        for i in range(len(split[0])):
            vals = [(lo + t * (hi - lo)) % q for lo, hi in (s[i] for s in split)]
            for c, mask in terms:
                p = 1 if c is None else c
                for j, v in enumerate(vals):
                    if (mask >> j) & 1:
                        p = p * v % q
                total += p
        out.append(total % q)
    return out


def mask_sets(nt, max_degree=4):
    """the mask sets of the issue for `nt` tables: {1}, {all}, {0b0011, 0b0100} (mixed degree), {0b1111, 0b0001} --
    each where it fits.  A term has at most max_degree factors, so with more tables "all" is the TOP max_degree tables,
    and every set is run again shifted to the top tables: each table of each count is a factor somewhere."""
    shift = max(0, nt - max_degree)
    sets = [[1], [((1 << min(nt, max_degree)) - 1) << shift]]
    if nt >= 3:
        sets.append([0b0011, 0b0100])
    if nt >= 4:
        sets.append([0b1111, 0b0001])
    if shift:
        sets += [[m << shift for m in s] for s in sets[2:]] + [[1 << (nt - 1)]]
    return sets


def interpolate(evals, x, q):
    """the polynomial of degree < len(evals) through (t, evals[t]), t = 0 .., at x (Lagrange)"""
    total = 0
    for t, y in enumerate(evals):
        num = den = 1
        for u in range(len(evals)):
            if u != t:
                num = num * (x - u) % q
                den = den * (t - u) % q
        total += y * num * pow(den, -1, q)
    return total % q
