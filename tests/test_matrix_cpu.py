"""Sparse matrices without a GPU: the host-callable part of csrc/matrix_kernels.h compiled for the CPU
(tests/native/matrix_test.cpp, the same templates the kernels instantiate) against Python integers
(tests/matrix_util.py) -- the host sort into both forms against sorted(), and the product emulated tile by tile (the
run walk, the segmented scan, the finish, the carry fold) for every row structure of the GPU test and all four scalar
fields; the descriptor layouts, the exports, null arguments and the Python argument checks.  The driver is also built
with the address and undefined-behaviour sanitizers as a stand-alone program and run over the same requests.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import matrix_util as M
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "matrix_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "matrix_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "matrix_kernels.h", "scalar_kernels.h", "fp.h", "constants_gen.h")]


def _build(exe, extra=()):
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, "-o", exe, SRC])


def _ask(exe, lines):
    """request lines -> the answer lines, as lists of words"""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(lines)
    return [line.split() for line in out[:len(lines)]]


@pytest.fixture(scope="module")
def driver():
    _build(EXE)
    return lambda lines: _ask(EXE, lines)


def _geometry():
    return [int(v) for v in subprocess.run([EXE], input="geometry\n", capture_output=True, text=True, check=True).stdout.split()]


# ------------------------------------------------------------------------------------------------ the host sort
def _sort_line(keys, others, n_keys):
    return f"sort {n_keys} {len(keys)} " + " ".join(f"{k} {o}" for k, o in zip(keys, others))


def _sort_cases():
    rng = random.Random(5)
    cases = [([0], [0], 1), ([4, 4, 4, 4], [3, 2, 1, 0], 5), ([3, 1, 2, 0], [9, 8, 7, 6], 4),
             ([2, 0, 2, 0, 2, 0], [5, 5, 5, 5, 5, 5], 3),                  # duplicates (key, other) kept apart, in order
             ([1, 0, 1], [(1 << 32) - 1, 7, 0], 2)]                        # the largest gathered index
    for nnz, n_keys in ((100, 7), (1000, 1000), (4097, 50), (513, 100000)):
        cases.append(([rng.randrange(n_keys) for _ in range(nnz)], [rng.randrange(1 << 32) for _ in range(nnz)], n_keys))
    return cases


def test_sort_is_the_stable_sort(driver):
    """mat_sort_form == sorted() by key: stable (triples of one key keep the caller's order), duplicates kept, shuffled
    input, empty keys; both forms of one matrix are this sort with the roles of row and col swapped"""
    cases = _sort_cases()
    got = driver([_sort_line(*c) for c in cases])
    for (keys, others, _), words in zip(cases, got):
        seg, gidx, perm = M.sorted_form(keys, others)
        assert [int(w) for w in words] == [v for t in zip(seg, gidx, perm) for v in t]
    rng = random.Random(6)
    rows = [rng.randrange(40) for _ in range(150)]
    cols = [rng.randrange(48) for _ in range(150)]
    by_row, by_col = driver([_sort_line(rows, cols, 40), _sort_line(cols, rows, 48)])
    assert [int(w) for w in by_row[2::3]] == sorted(range(150), key=lambda k: rows[k])
    assert [int(w) for w in by_col[2::3]] == sorted(range(150), key=lambda k: cols[k])
    assert sorted(zip(map(int, by_row[0::3]), map(int, by_row[1::3]))) == sorted(zip(map(int, by_col[1::3]), map(int, by_col[0::3])))


def test_first_bad_index(driver):
    """the triples are looked at in the caller's order; the bound is exclusive"""
    lines = ["badindex 4 5 3 0 0 3 4 1 1", "badindex 4 5 3 0 0 4 0 0 5", "badindex 4 5 3 0 5 4 0 0 0", "badindex 4 5 2 3 4 3 5",
             "badindex 1 1 1 0 0", f"badindex 4 5 2 {(1 << 32) - 1} 0 0 0"]
    assert [int(w[0]) for w in driver(lines)] == [3, 1, 0, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ tiles on the CPU
def _mul_line(label, rows, cols, vals, x, n_rows):
    seg, gidx, perm = M.sorted_form(rows, cols)
    body = " ".join(f"{s} {g}" + ("" if vals is None else f" {vals[p]:x}") for s, g, p in zip(seg, gidx, perm))
    return f"{label} mul {n_rows} {len(x)} {len(rows)} {0 if vals is None else 1} {body} " + " ".join(f"{v:x}" for v in x)


def _cases(label, nnz_list, T, E, seed):
    q = S.order(label)
    rng = random.Random(seed)
    for nnz in nnz_list:
        n_cols = max(1, min(nnz, 61))
        x = M.x_for(n_cols, q, rng)
        for si, (name, (rows, n_rows)) in enumerate(M.structures(nnz, T, E, seed).items()):
            cols = M.columns(nnz, n_cols, rng, duplicates=si % 2 == 0)
            vals = M.values_for(nnz, q, rng)
            if si % 3 == 0:
                rows, cols, vals = M.shuffled(rows, cols, vals, rng)
            for v in (vals, None):
                yield (name, nnz, v is None), _mul_line(label, rows, cols, v, x, n_rows), M.matvec(rows, cols, v, x, n_rows, q)


def _check(driver, cases):
    ids, lines, want = zip(*cases)
    got = driver(list(lines))
    bad = [(i, g[:2], w[:2]) for i, g, w in zip(ids, got, want) if [int(v, 16) for v in g] != w + [0]]
    assert not bad, bad[:3]


@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_tiles_every_size_and_structure(driver, label):
    """every nnz of the GPU test x every row structure (one row; one per row; a row across three tiles; boundaries on
    run and tile edges; empty rows first, last and at a tile edge; power-law lengths), with duplicates, shuffled
    triples, values over {0, 1, q - 1, random} and the value-less form == the Python model"""
    T, E, _ = _geometry()
    _check(driver, list(_cases(label, M.sizes(T, E), T, E, 40 + S.ALL.index(label))))


@pytest.mark.parametrize("label", ["bls12-381", "ed-on-bls12-377"])
def test_tiles_other_fields(driver, label):
    T, E, _ = _geometry()
    _check(driver, list(_cases(label, [E + 1, 2 * T + 5], T, E, 50 + S.ALL.index(label))))


def test_fold_loops_over_passes(driver):
    """more tiles than the fold takes per pass: one row over all of them (the sum crosses the passes), and rows that
    end exactly with the last tile of a pass"""
    T, E, P = _geometry()
    label, q = "pallas", S.order("pallas")
    rng = random.Random(9)
    nnz = (P + 2) * T + 3
    x = M.x_for(17, q, rng)
    cols = M.columns(nnz, 17, rng)
    cases = []
    for name, rows in (("one_row", [0] * nnz), ("ends_with_pass", [0] * (P * T) + [2] * (nnz - P * T)),
                       ("a_row_per_tile", [k // T for k in range(nnz)]),
                       ("tiles_in_pairs", [k // (2 * T) for k in range(nnz)])):
        cases.append(((name, nnz, True), _mul_line(label, rows, cols, None, x, max(rows) + 2), M.matvec(rows, cols, None, x, max(rows) + 2, q)))
    _check(driver, cases)


def test_entry_of_x_not_below_q(driver):
    """an entry >= q raises the error bit if a non-zero reads it and not otherwise"""
    label, q = "bls12-377", S.order("bls12-377")
    rows, cols = [0, 1, 1, 2], [0, 2, 0, 2]
    lines = [_mul_line(label, rows, cols, [1, 2, 3, 4], [5, q, 7], 3), _mul_line(label, rows, cols, [1, 2, 3, 4], [5, 6, q], 3),
             _mul_line(label, rows, cols, None, [(1 << 256) - 1, 6, 7], 3)]
    got = driver(lines)
    assert [int(g[-1]) for g in got] == [0, 1, 1]
    assert [int(v, 16) for v in got[0][:3]] == M.matvec(rows, cols, [1, 2, 3, 4], [5, 0, 7], 3, q)


def test_sanitized_driver_runs_clean(tmp_path):
    """matrix_test.cpp as a stand-alone program with -fsanitize=address,undefined over requests of every kind: exit 0,
    nothing on stderr, the same answers"""
    _build(EXE)
    exe = EXE + "_asan"
    _build(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    T, E, _ = _geometry()
    cases = list(_cases("pallas", [1, E + 1, T + 1, 2 * T + 5], T, E, 3))
    lines = ["geometry", _sort_line([3, 1, 3, 0], [1, 2, 3, 4], 4), "badindex 2 2 2 0 0 2 0"] + [c[1] for c in cases]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=64, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


Q = 1009


def _sparse(rows=(0, 1), cols=(1, 0), values=None, shape=(2, 2), orientations="rows", firstValue=0):
    from msm_zprize_amd.parallel import sparse_matrix_args
    return sparse_matrix_args(rows, cols, values, shape, orientations, firstValue, Q)


def test_sparse_matrix_args():
    import array
    a = _sparse()
    assert (a["nnz"], a["shape"], a["flags"], a["firstValue"], a["upload"]) == (2, (2, 2), 1, 0, None)
    assert list(a["row"]) == [0, 1] and list(a["col"]) == [1, 0]
    assert _sparse(orientations="cols")["flags"] == 2 and _sparse(orientations="both")["flags"] == 3
    assert _sparse(values=[5, Q - 1])["upload"] == (5).to_bytes(32, "little") + (Q - 1).to_bytes(32, "little")
    assert _sparse(values=[(7).to_bytes(32, "little"), 0])["upload"] == (7).to_bytes(32, "little") + bytes(32)
    assert _sparse(values=_arr(10), firstValue=8)["firstValue"] == 8
    assert list(_sparse(rows=array.array("I", [1, 0]), cols=[0, 1])["row"]) == [1, 0]
    assert _sparse(rows=[0] * 5, cols=[0] * 5, shape=(1, 1))["nnz"] == 5
    for kw in (dict(rows=None), dict(rows=7), dict(rows=[0, 1.0]), dict(rows=[0, True]), dict(cols="ab"), dict(shape=None),
               dict(shape=(2,)), dict(shape=(2, 2.0)), dict(values=7), dict(values=_arr(10, 2, "points")), dict(values=[1, 1.5]),
               dict(values=[1, b"\x01"]), dict(rows=array.array("H", [0, 1])), dict(rows=array.array("i", [0, 1]))):
        with pytest.raises(TypeError):
            _sparse(**kw)
    for kw in (dict(rows=[0, 2]), dict(rows=[0, -1]), dict(cols=[2, 0]), dict(cols=[0]), dict(rows=[], cols=[]), dict(shape=(0, 2)),
               dict(shape=(2, 0)), dict(shape=(1 << 32, 2)), dict(orientations="row"), dict(orientations=None), dict(values=[1]),
               dict(values=[1, Q]), dict(values=[1, -1]), dict(values=[1, Q.to_bytes(32, "little")]), dict(firstValue=1),
               dict(values=_arr(10), firstValue=9), dict(values=_arr(10), firstValue=-1), dict(values=_arr(10), firstValue=True),
               dict(values=_arr(1)), dict(rows=array.array("I", [0, 2]))):
        with pytest.raises(ValueError):
            _sparse(**kw)
    with pytest.raises(ValueError, match=r"rows\[1\] = 2 is not in \[0, 2\)"):
        _sparse(rows=[0, 2])


def _matrix(shape=(3, 5), orientations="rows", handle=9):
    from msm_zprize_amd.parallel import SparseMatrix
    return SparseMatrix(None, handle, shape, 4, orientations)


def _matvec(matrix, x, firstX=0, transpose=False, out=None, firstOut=0):
    from msm_zprize_amd.parallel import mat_vec_args
    return mat_vec_args(matrix, x, firstX, transpose, out, firstOut)


def test_mat_vec_args():
    m, both, x, y = _matrix(), _matrix(orientations="both"), _arr(64, 1), _arr(8, 2)
    assert _matvec(m, x) == {"N": 3, "flags": 0}
    assert _matvec(both, x, transpose=True) == {"N": 5, "flags": 1}
    assert _matvec(_matrix(orientations="cols"), y, firstX=5, transpose=True)["N"] == 5
    assert _matvec(m, x, firstX=59)["N"] == 3
    assert _matvec(m, x, out=y, firstOut=5)["N"] == 3
    assert _matvec(m, x, firstX=3, out=x, firstOut=0)["N"] == 3          # ends where x begins
    assert _matvec(m, x, firstX=3, out=x, firstOut=8)["N"] == 3          # begins where x ends
    for args, kw in (((None, x), {}), ((7, x), {}), ((x, x), {}), ((m, None), {}), ((m, _arr(64, 3, "points")), {}),
                     ((m, x), dict(out=7)), ((m, x), dict(out=_arr(64, 3, "points"))), ((m, x), dict(transpose=1))):
        with pytest.raises(TypeError):
            _matvec(*args, **kw)
    same = _arr(64, 1)   # another object for the same handle overlaps all the same
    for args, kw in (((m, x), dict(transpose=True)), ((_matrix(orientations="cols"), x), {}),       # the orientation
                     ((m, x), dict(firstX=60)), ((m, x), dict(firstX=-1)), ((m, x), dict(firstX=True)), ((m, x), dict(firstX=64)),
                     ((both, y), dict(transpose=True, firstX=6)), ((m, x), dict(firstOut=1)), ((m, x), dict(out=y, firstOut=6)),
                     ((m, x), dict(out=y, firstOut=-1)),
                     ((m, x), dict(out=x)), ((m, x), dict(out=same)),                                 # the exact range and
                     ((m, x), dict(firstX=3, out=x, firstOut=1)), ((m, x), dict(firstX=3, out=x, firstOut=7)),   # every partial one
                     ((m, x), dict(firstX=3, out=same, firstOut=5))):
        with pytest.raises(ValueError):
            _matvec(*args, **kw)
    freed = _matrix()
    freed.handle = None
    with pytest.raises(ValueError):
        _matvec(freed, x)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


NAMES = ("msmz_matrix_create", "msmz_matrix_info", "msmz_matrix_mul", "msmz_test_matrix_geometry")


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in NAMES:
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    assert C.sizeof(_native.MsmzSparse) == 56 and C.sizeof(_native.MsmzMatvec) == 32
    assert (_native.MSMZ_MAT_ROWS, _native.MSMZ_MAT_COLS, _native.MSMZ_MATVEC_TRANSPOSE) == (1, 2, 1)
    header = open(os.path.join(ROOT, "include", "msmz.h")).read()
    assert "MSMZ_MAT_ROWS = 1, MSMZ_MAT_COLS = 2" in header and "MSMZ_MATVEC_TRANSPOSE = 1" in header


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof and the offsets of every field of the two descriptors, C side == ctypes side"""
    from msm_zprize_amd import _native as N
    src = tmp_path / "layout.c"
    prints, want = [], []
    for cname, T in (("msmz_sparse", N.MsmzSparse), ("msmz_matvec", N.MsmzMatvec)):
        prints.append(f'printf("%zu ", sizeof({cname}));')
        want.append(C.sizeof(T))
        for fname, _ in T._fields_:
            prints.append(f'printf("%zu ", offsetof({cname}, {fname}));')
            want.append(getattr(T, fname).offset)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msmz.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()] == want
    assert want[0] == 56 and want[len(N.MsmzSparse._fields_) + 1] == 32


def test_geometry_accessor(lib, driver):
    """msmz_test_matrix_geometry == the constants the host driver was compiled with; needs no context"""
    t, r, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lib.msmz_test_matrix_geometry(C.byref(t), C.byref(r), C.byref(p))
    assert [t.value, r.value, p.value] == _geometry()
    assert t.value % r.value == 0 and t.value // r.value == 256 and r.value >= 2 and p.value >= 2
    lib.msmz_test_matrix_geometry(None, None, None)


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG and the outputs untouched, for all three entry points"""
    from msm_zprize_amd import _native as N
    idx = (C.c_uint32 * 1)(0)
    s = N.MsmzSparse(idx, idx, 0, 0, 1, 1, 1, 0)
    h = C.c_uint64(77)
    assert lib.msmz_matrix_create(None, C.byref(s), C.byref(h)) == 1 and h.value == 77
    r, c, n, f = C.c_uint32(5), C.c_uint32(6), C.c_uint64(7), C.c_uint32(8)
    assert lib.msmz_matrix_info(None, 1, C.byref(r), C.byref(c), C.byref(n), C.byref(f)) == 1
    assert (r.value, c.value, n.value, f.value) == (5, 6, 7, 8)
    v = N.MsmzMatvec(1, 1, 0, 0)
    assert lib.msmz_matrix_mul(None, C.byref(v), 0, C.byref(h)) == 1 and h.value == 77
