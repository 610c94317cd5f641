"""Shared by the recurrence / inversion tests (tests/test_scalar_scan_cpu.py, tests/test_scalar_scan_gpu.py,
tests/test_js_scalar_scan.py, tests/golden/make_scalar_scan_fixture.py): the plain sequential recurrence and the
inverse on Python integers, the five modes, and operand vectors.  Expected values are Python integers mod
oracle.params.CURVES[label]["order"]."""
import random

import scalar_ops_util as S

ALL = S.ALL
# (name, multiplier: None / "broadcast" / "resident", addend present)
MODES = [("sums", None, True), ("geometric", "broadcast", False), ("horner", "broadcast", True),
         ("products", "resident", False), ("general", "resident", True)]
MODE = {m[0]: m for m in MODES}


def recurrence(q, n, a, b, init=None, reverse=False, exclusive=False):
    """y_i = a_i y_(i-1) + b_i (reverse: y_(i+1)) -> (the n output entries, the final y).  a: None (1), an int (one
    multiplier) or a list; b: None or a list; init None: 0 with an addend, 1 without."""
    y = (0 if b is not None else 1) if init is None else init
    out = [None] * n
    for p in range(n):
        i = n - 1 - p if reverse else p
        ai = 1 if a is None else (a if isinstance(a, int) else a[i])
        before = y
        y = (ai * y + (0 if b is None else b[i])) % q
        out[i] = before if exclusive else y
    return out, y


def inverse(q, xs):
    """-> (x^-1 or 0, the number of zeros)"""
    return [pow(x, -1, q) if x else 0 for x in xs], sum(1 for x in xs if x == 0)


def mode_operands(label, mode, n, seed):
    """(a, b) of a mode over n entries as the recurrence() arguments: edge values first, random values after"""
    q = S.order(label)
    rng = random.Random(seed * 7919 + n)
    _, mult, addend = MODE[mode]
    xs, ys = S.build_vectors(label, n, seed)
    a = None if mult is None else (rng.randrange(2, q) if mult == "broadcast" else xs)
    return a, (ys if addend else None)


def synthetic_division(q, p, z):
    """(p(X) - p(z)) / (X - z): the quotient's n coefficients (the top one 0) and p(z)"""
    n = len(p)
    w = [0] * n
    acc = 0
    for i in range(n - 1, -1, -1):
        w[i] = acc
        acc = (acc * z + p[i]) % q
    return w, acc
