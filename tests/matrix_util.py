"""Shared by the sparse-matrix tests (tests/test_matrix_cpu.py, tests/test_matrix_gpu.py, tests/test_js_matvec.py,
tests/golden/make_matvec_fixture.py): the product in Python integers, and the row structures that decide where the
segments of a product fall against the runs and tiles of csrc/matrix_kernels.h.  T is a tile, E a run, both from
msmz_test_matrix_geometry (or the CPU driver's `geometry`), never copies of the constants."""
import random

from oracle.prng import splitmix64

import scalar_ops_util as S


def matvec(rows, cols, vals, x, n_rows, q, transpose=False):
    """out_i = sum over {k: rows[k] == i} of vals[k] x[cols[k]] mod q (vals None: every value is 1); transpose swaps
    the roles of rows and cols, and n_rows is then the column count"""
    if transpose:
        rows, cols = cols, rows
    out = [0] * n_rows
    for k, (i, j) in enumerate(zip(rows, cols)):
        out[i] += x[j] if vals is None else vals[k] * x[j]
    return [v % q for v in out]


def sorted_form(keys, others):
    """what mat_sort_form must leave: (seg, gidx, perm), a STABLE sort of the triples by key"""
    perm = sorted(range(len(keys)), key=lambda k: keys[k])
    return [keys[k] for k in perm], [others[k] for k in perm], perm


def sizes(T, E):
    """the non-zero counts of the issue"""
    return [1, E - 1, E, E + 1, 64 * E - 1, 64 * E, T - 1, T, T + 1, 2 * T + 5, 3 * T]


def _from_lengths(lengths, nnz, first_row=0, gaps=None):
    """rows (sorted) from consecutive row lengths, cut at nnz; gaps: {row position: empty rows before it}"""
    rows, r = [], first_row
    for pos, n in enumerate(lengths):
        r += (gaps or {}).get(pos, 0)
        rows += [r] * min(n, nnz - len(rows))
        r += 1
        if len(rows) >= nnz:
            break
    while len(rows) < nnz:   # the lengths ran out: one non-zero per row from here on
        rows.append(r)
        r += 1
    return rows


def structures(nnz, T, E, seed=0):
    """{name: (rows in sorted order, n_rows)} for one nnz: where the row boundaries fall is the whole test"""
    out = {}
    out["one_row"] = ([0] * nnz, 1)                                  # carries chain across every tile
    out["one_per_row"] = (list(range(nnz)), nnz)
    # a row from the last run of tile 0 to the first run of tile 2 (as far as nnz reaches), one per row around it
    a, b = max(0, T - E + 1), min(nnz, 2 * T + 2)
    rows = list(range(a)) + [a] * max(0, b - a)
    rows = (rows + list(range(a + 1, a + 1 + nnz)))[:nnz]
    out["span_tiles"] = (rows, max(rows) + 1)
    # boundaries exactly on run boundaries (rows of E and 2E) and exactly on the tile boundary (E divides T)
    out["on_boundaries"] = (_from_lengths([E, 2 * E, E] * (nnz // (4 * E) + 1), nnz), None)
    # empty rows first (3), last (4), and a stretch of 5 exactly where the tile boundary falls: the row of non-zero T - 1
    # ends with tile 0 and the next non-empty row begins tile 1
    per = E // 2 + 1
    rows = [3 + k // per if k < T else 3 + (T - 1) // per + 6 + (k - T) // per for k in range(nnz)]
    out["empty_rows"] = (rows, max(rows) + 5)
    # power-law lengths: 2^k with probability 2^-(k+1), k <= 12, from the repository's generator
    def length(i):
        z = splitmix64(seed + 77, i) | (1 << 12)
        return z & -z
    out["power_law"] = (_from_lengths([length(i) for i in range(nnz)], nnz), None)
    fixed = {}
    for name, (rows, n_rows) in out.items():
        assert len(rows) == nnz and rows == sorted(rows), name
        fixed[name] = (rows, max(rows) + 1 if n_rows is None else n_rows)
    return fixed


def values_for(nnz, q, rng):
    """0, 1, q - 1 and random, the constants planted at the start, around the middle and at the end"""
    vals = S.random_below_2_250(nnz, rng)
    for k, v in ((0, q - 1), (1, 0), (2, 1), (nnz // 2, q - 1), (nnz // 2 + 1, 0), (nnz - 2, 1), (nnz - 1, q - 1)):
        if 0 <= k < nnz:
            vals[k] = v
    return vals


def x_for(n, q, rng):
    """random entries with 0, q - 1 and 1 planted"""
    x = S.random_below_2_250(n, rng)
    for k, v in ((0, q - 1), (1, 0), (n // 2, q - 1), (n - 1, 0), (n - 2, 1)):
        if 0 <= k < n:
            x[k] = v
    return x


def columns(nnz, n_cols, rng, duplicates=False):
    """a column per non-zero; duplicates: every third non-zero repeats the column of the one before it (with a sorted
    row list that makes duplicate (row, col) pairs wherever a row is longer than one)"""
    cols = [rng.randrange(n_cols) for _ in range(nnz)]
    if duplicates:
        for k in range(1, nnz, 3):
            cols[k] = cols[k - 1]
    return cols


def shuffled(rows, cols, vals, rng):
    order = list(range(len(rows)))
    rng.shuffle(order)
    return [rows[k] for k in order], [cols[k] for k in order], None if vals is None else [vals[k] for k in order]
