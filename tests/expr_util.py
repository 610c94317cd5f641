"""The Python-integer model of msmz_scalars_expr / evaluateExpression: columns are lists of ints below q, a rotation is
cyclic inside the column,
    out_i = sum_T c_T prod_(f in T) columns[f.column][(i + f.rot) mod n]   mod q,
and the term sets the CPU, GPU and JavaScript tests share.  A term is (c or None, [column or (column, rot), ...])."""
import random

MAX_COLUMNS, MAX_TERMS, MAX_DEGREE, MAX_OPERANDS = 16, 32, 8, 32
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)


def factor(f):
    """a factor as (column, rot)"""
    return f if isinstance(f, tuple) else (f, 0)


def index(i, rot, n):
    """the entry a factor at rotation `rot` reads for output i"""
    return (i + rot) % n


def model(columns, terms, n, q):
    """columns: lists of at least n ints (the first n are the column) -> the n output values"""
    out = []
    for i in range(n):
        acc = 0
        for c, factors in terms:
            p = 1 if c is None else c
            for f in factors:
                col, rot = factor(f)
                p = p * columns[col][index(i, rot, n)] % q
            acc = (acc + p) % q
        out.append(acc)
    return out


def operands(terms, n):
    """the distinct (column, rot mod n) pairs in first-use order: the operand table of the compile step"""
    seen = []
    for _, factors in terms:
        for f in factors:
            col, rot = factor(f)
            if (col, rot % n) not in seen:
                seen.append((col, rot % n))
    return seen


def rotations(n):
    """the rotations every size class is tested at"""
    return [0, 1, -1, n - 1, n, -n, n + 1, INT32_MAX, INT32_MIN]


# -- the gates of the report (tools/expr_report.py) and of the protocol tests ---------------------------------------
def plonk_gate(qL=0, qR=1, qO=2, qM=3, qC=4, a=5, b=6, c=7):
    """q_L a + q_R b + q_M a b + q_O c + q_C over 8 columns: 5 terms, degree 3"""
    return [(None, [qL, a]), (None, [qR, b]), (None, [qM, a, b]), (None, [qO, c]), (None, [qC])]


def permutation_wire(beta, gamma, q, z=0, w=1, sigma=2, ident=3):
    """one wire of the permutation step, Z(wX) (w + beta sigma + gamma) - Z(X) (w + beta id + gamma), expanded into a
    sum of products: 6 terms, one rotated operand"""
    return [(None, [(z, 1), w]), (beta, [(z, 1), sigma]), (gamma, [(z, 1)]),
            (q - 1, [z, w]), (q - beta, [z, ident]), (q - gamma, [z])]


def sbox_gate(c, q, a=0, b=1):
    """a^5 + c b - a[+1]: a repeated factor"""
    return [(None, [a] * 5), (c, [b]), (q - 1, [(a, 1)])]


def stress_gate(q, rng):
    """32 terms of degree 8 over 16 columns, unrotated: 16 operands"""
    return [(rng.randrange(q), [rng.randrange(MAX_COLUMNS) for _ in range(MAX_DEGREE)]) for _ in range(MAX_TERMS)]


# -- the term sets of the tests -------------------------------------------------------------------------------------
def term_sets(q, n, seed=0):
    """name -> (number of columns, terms): every shape the compile step and the kernels tell apart.  The coefficients
    cover None, 0, 1, q - 1 and random values; degrees 0 .. 8; a^8; the same column at three rotations in one term;
    mixed degrees; operand counts 1, 2, 3, 4, 5, 8, 9 and 32 (the edges of every register-resident instance)."""
    rng = random.Random(1000 + seed)
    r = lambda: rng.randrange(q)   # noqa: E731
    sets = {
        "constant": (1, [(r(), [])]),
        "constants_only": (2, [(r(), []), (None, []), (0, []), (q - 1, [])]),
        "copy": (1, [(None, [0])]),
        "zero_coeff": (2, [(0, [0, 1]), (1, [1])]),
        "linear": (2, [(r(), [0]), (r(), [1])]),
        "product": (2, [(None, [0, 1])]),
        "a8": (1, [(q - 1, [0] * 8)]),
        "degrees_0_to_8": (3, [(r(), [k % 3 for k in range(d)]) for d in range(MAX_DEGREE + 1)]),
        "three_rotations": (2, [(r(), [(0, 1), (0, -1), (0, 2), 1]), (None, [(0, -1), (0, 1)])]),
        "plonk": (8, plonk_gate()),
        "permutation": (4, permutation_wire(r(), r(), q)),
        "sbox": (2, sbox_gate(r(), q)),
        "operands_4": (2, [(r(), [(0, 0), (0, 1), (1, 0), (1, -1)]), (None, [(1, -1), (1, -1)])]),
        "operands_5": (3, [(r(), [(0, 0), (0, 1), (1, 0), (1, -1), (2, 3)])]),
        "operands_8": (4, [(r(), [(k % 4, k // 4) for k in range(8)]), (r(), [(3, 1)] * 3)]),
        "operands_9": (3, [(r(), [(k % 3, k // 3) for k in range(8)]), (None, [(2, 2), (0, 0)])]),
        "columns_16": (16, [(r(), [k, (k + 1) % 16]) for k in range(16)]),
        "terms_32": (4, [(r(), [(k % 4, k % 3 - 1)] * (1 + k % 3)) for k in range(MAX_TERMS)]),
        "stress": (16, stress_gate(q, rng)),
    }
    if n >= MAX_OPERANDS // 2:   # 32 distinct pairs need 16 distinct rotations of two columns
        sets["operands_32"] = (2, [(r(), [(k % 2, k // 2) for k in range(8 * t, 8 * t + 8)]) for t in range(4)])
    return sets


def edge_columns(n_columns, n, q, rng):
    """columns of n values over {0, 1, q - 1, random}, every column with each of them somewhere when n allows"""
    pick = [0, 1, q - 1]
    return [[pick[(i + c) % 4] if (i + c) % 4 < 3 else rng.randrange(q) for i in range(n)] for c in range(n_columns)]
