"""The yardstick of the batched inner-product tests (tests/test_dot_many_cpu.py, tests/test_dot_many_gpu.py,
tests/test_js_dot_many.py, tests/golden/make_dot_many_fixture.py): Python integers mod q over lists, and the case
builders.  result[r][c] = sum_i rows[r][i] cols[c][i] mod q (include/msmz.h, msmz_scalars_dot_many)."""
import random

import scalar_ops_util as S

MAX_ROWS, MAX_COLS = 128, 8
SCRATCH_MAX = 16 << 20
STRIDE = 7      # entries between the starts of two vectors of a pool: they overlap as soon as n > 7


def products(rows, cols, q):
    """every inner product of the lists `rows` with the lists `cols`, row-major as a list of lists"""
    return [[sum(a * b for a, b in zip(r, c)) % q for c in cols] for r in rows]


def horner(coeffs, z, q):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % q
    return acc


def pool(label, n, seed):
    """the values of ONE scalar set that holds MAX_ROWS + MAX_COLS + 4 overlapping vectors of n entries, vector k from entry
    first(k): the planted rows of the scalar-set tests at its head and ending at its last index, random values between"""
    xs, ys = S.build_vectors(label, first(MAX_ROWS + MAX_COLS + 4) + n, seed)
    return [x if k % 3 else y for k, (x, y) in enumerate(zip(xs, ys))]


def first(k):
    return 5 + STRIDE * k


def vector(values, k, n):
    return values[first(k):first(k) + n]


def plan(n, n_rows, n_cols, rows_per_block, tile, max_groups):
    """the planner of csrc/dot_kernels.h in Python integers -> (rg, tiles, groups, row_groups, scratch bytes)"""
    rg = rows_per_block[n_cols - 1]
    tiles = -(-n // tile)
    results = n_rows * n_cols
    room = (SCRATCH_MAX - 64) // (32 * results) - 1
    groups = min(tiles, max_groups, room)
    return rg, tiles, groups, -(-n_rows // rg), 64 + 32 * results * (1 + groups)


def fixture_values(label, n_rows, n_cols, n, seed):
    """rows and columns of the JavaScript fixture: the operands of the scalar-set tests, 0 and q - 1 among them"""
    q = S.order(label)
    rng = random.Random(seed)
    ops = S.operands(label, seed)
    draw = lambda: [ops[rng.randrange(len(ops))] if rng.random() < 0.5 else rng.randrange(q) for _ in range(n)]   # noqa: E731
    rows, cols = [draw() for _ in range(n_rows)], [draw() for _ in range(n_cols)]
    rows[0][0], rows[0][1], cols[0][0], cols[0][1] = 0, q - 1, q - 1, q - 1
    return rows, cols
