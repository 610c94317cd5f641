"""The batched inner products without a GPU: the body of k_scalars_dot_many compiled for the CPU
(tests/native/dot_many_test.cpp: fr_dot_many_index, one thread's register block over a run of element indices) against
Python integers (tests/dot_many_util.py) on all four curves, the same program under -fsanitize=address,undefined; the
planner dot_many_plan over every row and column count at the sizes where it changes its answer; the Python argument
checks of innerProducts and the host side of evaluatePolynomials on a library that is a Python model; the export, the
descriptors' layout and the null context.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import dot_many_util as U
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "dot_many_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "dot_many_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


def _build(exe, flags=("-O2",)):
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "dot_kernels.h", "scalar_kernels.h", "sqrt.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", *flags, "-std=c++17", "-o", exe, SRC])


def _ask(exe, lines, base=16):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(lines)
    return [[int(v, base) for v in line.split()] for line in out[:len(lines)]]


def _geometry():
    _build(EXE)
    g = _ask(EXE, ["geometry"], 10)[0]
    return dict(tile=g[0], threads=g[1], per_thread=g[2], groups=g[3], max_rows=g[4], max_cols=g[5], vecs_bytes=g[6], rg=g[7:])


def _requests(label):
    """(request line, wanted answer): every column count with its full block and every shorter row tail, over 1, 2 and 9
    element indices; operands 0, 1, q - 1 in every position of the first block, then S.operands and random values"""
    q = S.order(label)
    rng = random.Random(S.ALL.index(label) + 3200)
    ops = S.operands(label, 5)
    rg = _geometry()["rg"]
    for nc in range(1, 9):
        for live in range(1, rg[nc - 1] + 1):
            for count, source in ((1, "edges"), (2, "edges"), (9, "operands"), (9, "random")):
                cols, rows = [], []
                for i in range(count):
                    pick = {"edges": lambda: (0, 1, q - 1)[rng.randrange(3)], "operands": lambda: ops[rng.randrange(len(ops))],
                            "random": lambda: rng.randrange(q)}[source]
                    cols.append([pick() for _ in range(nc)])
                    rows.append([pick() for _ in range(live)])
                if source == "edges":
                    cols[0][0], rows[0][0] = q - 1, q - 1
                words = " ".join(f"{v:x}" for i in range(count) for v in cols[i] + rows[i])
                want = U.products([[rows[i][j] for i in range(count)] for j in range(live)],
                                  [[cols[i][c] for i in range(count)] for c in range(nc)], q)
                yield f"{label} block {nc} {live} {count} {words}", [v for row in want for v in row]


@pytest.mark.parametrize("label", S.ALL)
def test_register_block(label):
    """fr_dot_many_index over a run of indices == the inner products of Python integers, for every (RG, NC) the planner
    emits and every row tail"""
    _build(EXE)
    lines, want = zip(*_requests(label))
    got = _ask(EXE, lines)
    bad = [(line[:60], g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]
    rg = _geometry()["rg"]
    assert len(lines) == 4 * sum(rg) and any(f" block 8 {rg[7]} 9 " in l for l in lines)


def test_sanitized_driver_runs_clean():
    """dot_many_test.cpp as a stand-alone program with -fsanitize=address,undefined over the requests of the test above on
    two curves, the planner at its largest size and malformed requests: exit 0, nothing on stderr, the same answers"""
    _build(EXE)
    exe = EXE + "_asan"
    _build(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    lines = ["geometry", "nocurve block", "pallas what", "pallas block 9 1 1", "pallas block 1 5 1", "pallas block 1 1 0",
             f"plan {(1 << 32) - 1} 2048", "plan 1 1"]
    lines += [l for label in ("bls12-377", "pallas") for l, _ in _requests(label)]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout


def _covered(n, tiles, groups, g):
    """the element indices the kernel's loops give the threads of workgroups 0 .. groups - 1, in order of appearance"""
    seen = []
    for b in range(groups):
        for tile in range(b, tiles, groups):
            for t in range(g["threads"]):
                for e in range(g["per_thread"]):
                    i = tile * g["tile"] + e * g["threads"] + t
                    if i < n:
                        seen.append(i)
    return seen


@pytest.mark.parametrize("max_groups", (2048, 2))
def test_planner(max_groups):
    """dot_many_plan at every (n_rows, n_cols) x n in {1, tile - 1, tile, tile + 1, 2^20 + 3, 2^32 - 1} == the same rules
    in Python integers; the grid covers every tile, and at the small sizes every index, exactly once; every row is in
    exactly one row group; scratch <= 16 MiB; the pointer tables fit the argument"""
    g = _geometry()
    tile = g["tile"]
    assert g["tile"] == g["threads"] * g["per_thread"] and (g["max_rows"], g["max_cols"]) == (U.MAX_ROWS, U.MAX_COLS)
    assert g["vecs_bytes"] == 8 * (U.MAX_ROWS + U.MAX_COLS) and g["vecs_bytes"] + 64 <= 4096
    assert g["groups"] == 2048 and all(1 <= r <= 8 for r in g["rg"])
    sizes = [1, tile - 1, tile, tile + 1, (1 << 20) + 3, (1 << 32) - 1]
    got = _ask(EXE, [f"plan {n} {max_groups}" for n in sizes], 10)
    largest, strides = 0, {}
    for n, line in zip(sizes, got):
        assert len(line) == 5 * U.MAX_ROWS * U.MAX_COLS
        k = 0
        for n_rows in range(1, U.MAX_ROWS + 1):
            for n_cols in range(1, U.MAX_COLS + 1):
                rg, tiles, groups, row_groups, scratch = line[k:k + 5]
                k += 5
                assert (rg, tiles, groups, row_groups, scratch) == U.plan(n, n_rows, n_cols, g["rg"], tile, max_groups)
                assert tiles == -(-n // tile) and 1 <= groups <= min(tiles, max_groups)
                if (tiles, groups) not in strides:   # workgroup b takes tiles b, b + groups, ..: apart by residue, all of them
                    strides[tiles, groups] = sum(len(range(b, tiles, groups)) for b in range(groups))
                assert strides[tiles, groups] == tiles
                assert (row_groups - 1) * rg < n_rows <= row_groups * rg
                assert scratch == 64 + 32 * n_rows * n_cols * (1 + groups) <= U.SCRATCH_MAX
                largest = max(largest, scratch)
        if n <= tile + 1:
            tiles = -(-n // tile)
            for groups in {1, min(tiles, max_groups)}:
                assert sorted(_covered(n, tiles, groups, g)) == list(range(n))
    assert largest > U.SCRATCH_MAX // 2 or max_groups == 2                                     # the cap is what binds
    n, tiles = 5 * tile + 9, 6
    assert sorted(_covered(n, tiles, 2, g)) == list(range(n)) == sorted(_covered(n, tiles, 6, g))


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=64, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


def _args(rows, cols, N=None, out=None, firstOut=0):
    from msm_zprize_amd.parallel import inner_products_args
    return inner_products_args(rows, cols, N, out, firstOut)


GOOD = [lambda f, g, d: ([f, (g, 36)], [f], None, None, 0), lambda f, g, d: ([f] * 128, [g] * 8, 64, None, 0),
        lambda f, g, d: ([(f, 63)], [(g, 99)], 1, None, 0), lambda f, g, d: ([f], [f], 64, d, 63),
        lambda f, g, d: ([(f, 0), (f, 8)], [(f, 20)], 8, f, 16), lambda f, g, d: ([(f, 0), (f, 8)], [(f, 20)], 8, f, 28),
        lambda f, g, d: ([(f, 0), (f, 8)], [(f, 20)], 8, f, 18), lambda f, g, d: ([f], [(f, 3)], None, None, 0)]
BAD_TYPE = [lambda f, g, d: (f, [f], None, None, 0), lambda f, g, d: ([f], None, None, None, 0), lambda f, g, d: ([7], [f], None, None, 0),
            lambda f, g, d: ([(f, 0, 0)], [f], None, None, 0), lambda f, g, d: ([(f, 1.5)], [f], None, None, 0),
            lambda f, g, d: ([f], [_arr(64, 4, "points")], None, None, 0), lambda f, g, d: ([f], [f], None, 7, 0),
            lambda f, g, d: ([f], [f], 1.5, None, 0), lambda f, g, d: ([f], [f], None, d, None)]
BAD_VALUE = [lambda f, g, d: ([], [f], None, None, 0), lambda f, g, d: ([f], [], None, None, 0),
             lambda f, g, d: ([f] * 129, [f], None, None, 0), lambda f, g, d: ([f], [f] * 9, None, None, 0),
             lambda f, g, d: ([f], [f], 0, None, 0), lambda f, g, d: ([f], [f], 1 << 32, None, 0),
             lambda f, g, d: ([f], [f], None, None, 1), lambda f, g, d: ([f], [f], None, d, -1),
             lambda f, g, d: ([(f, -1)], [f], None, None, 0), lambda f, g, d: ([(f, 65)], [f], None, None, 0),
             lambda f, g, d: ([(f, 64)], [f], None, None, 0), lambda f, g, d: ([(f, 57)], [f], 8, None, 0),
             lambda f, g, d: ([f], [(g, 37)], 64, None, 0), lambda f, g, d: ([f], [f], 64, d, 64),
             lambda f, g, d: ([f, f], [f], 64, d, 63)] + \
            [lambda f, g, d, at=at: ([(f, 0), (f, 8)], [(f, 20)], 8, f, at) for at in (0, 7, 15, 19, 20, 27)]


def test_inner_products_args():
    """the checks of msmz_scalars_dot_many, case for case: a TypeError for a wrong type, a ValueError for each
    MSMZ_ERR_ARG, and their neighbours accepted"""
    f, g, d = _arr(64, 1), _arr(100, 2), _arr(64, 3)
    a = _args(*GOOD[0](f, g, d))
    assert a == {"rows": [(f, 0), (g, 36)], "cols": [(f, 0)], "N": 64, "firstOut": 0}
    assert _args(*GOOD[7](f, g, d))["N"] == 61
    for case in GOOD:
        _args(*case(f, g, d))
    for case in BAD_TYPE:
        with pytest.raises(TypeError):
            _args(*case(f, g, d))
    for k, case in enumerate(BAD_VALUE):
        with pytest.raises(ValueError):
            _args(*case(f, g, d))
            pytest.fail(f"case {k} was accepted")
    same = _arr(64, 1)   # another object for the same handle overlaps all the same
    with pytest.raises(ValueError):
        _args([f], [f], 8, same, 7)
    assert _args([f], [f], 8, same, 8)["firstOut"] == 8


class _ModelLib:
    """stands in for the loaded library: resident scalar sets as Python lists, powers and the batched inner products by
    the integer model; counts its calls"""

    def __init__(self, q):
        self.q, self.sets, self.next, self.calls = q, {}, 1, []

    def add(self, values):
        self.sets[self.next] = list(values)
        self.next += 1
        return self.next - 1

    def msmz_free(self, ctx, h):
        self.calls.append("free")
        del self.sets[h]
        return 0

    def msmz_scalars_powers(self, ctx, base, ratio, n, h):
        self.calls.append("powers")
        b, r = int.from_bytes(base, "little"), int.from_bytes(ratio, "little")
        h._obj.value = self.add([b * pow(r, i, self.q) % self.q for i in range(n)])
        return 0

    def msmz_scalars_dot_many(self, ctx, d, buf, first_out, h):
        d = d._obj
        self.calls.append("dot_many")
        vec = lambda v: self.sets[v.handle][v.first:v.first + d.n]   # noqa: E731
        flat = [x for row in U.products([vec(d.rows[r]) for r in range(d.n_rows)], [vec(d.cols[c]) for c in range(d.n_cols)], self.q)
                for x in row]
        if buf is not None:
            C.memmove(buf, S.encode(flat), 32 * len(flat))
        if h is not None:
            self.sets[h._obj.value][first_out:first_out + len(flat)] = flat
        return 0


class _Curve:
    _ctx = "ctx"

    def __init__(self, q):
        self.params = {"order": q}


def test_methods_reach_the_library(monkeypatch):
    """innerProducts hands the library the descriptor its arguments describe; evaluatePolynomials is one power vector per
    point, ONE batched call, and the vectors freed -- also when the call fails; both refuse before the library"""
    from msm_zprize_amd import parallel
    q = S.order("pallas")
    rng = random.Random(13)
    lib = _ModelLib(q)
    monkeypatch.setattr(parallel, "lib", lambda: lib)
    curve = _Curve(q)
    par = parallel._Parallel(curve)
    data = [[rng.randrange(q) for _ in range(40)] for _ in range(3)]
    f, g, h = (parallel.DeviceArray(curve, lib.add(v), 40, "scalars") for v in data)
    got = par.innerProducts([f, (g, 8)], [(h, 2), f, (f, 1)], 30)
    assert got == U.products([data[0][:30], data[1][8:38]], [data[2][2:32], data[0][:30], data[0][1:31]], q)
    dest = parallel.DeviceArray(curve, lib.add([None] * 10), 10, "scalars")
    assert par.innerProducts([f, g], [h], out=dest, firstOut=3) is dest
    assert lib.sets[dest.handle] == [None] * 3 + [x for row in U.products(data[:2], data[2:], q) for x in row] + [None] * 5
    lib.calls.clear()
    points = [0, 1, q - 1, rng.randrange(q)]
    got = par.evaluatePolynomials([f, (g, 5)], points, 35)
    assert got == [[U.horner(c, z, q) for z in points] for c in (data[0][:35], data[1][5:])]
    assert lib.calls == ["powers"] * 4 + ["dot_many"] + ["free"] * 4 and len(lib.sets) == 4
    assert par.evaluatePolynomials([f], [5]) == [[U.horner(data[0], 5, q)]]
    lib.calls.clear()
    for bad, err in ((lambda: par.evaluatePolynomials([f], [q]), ValueError), (lambda: par.evaluatePolynomials([f], []), ValueError),
                     (lambda: par.evaluatePolynomials([f], 5), TypeError), (lambda: par.evaluatePolynomials(f, [5]), TypeError),
                     (lambda: par.evaluatePolynomials([f], [5], 41), ValueError), (lambda: par.evaluatePolynomials([f], [5] * 9), ValueError),
                     (lambda: par.innerProducts([f], [f], 41), ValueError), (lambda: par.innerProducts([f], [f], out=f), ValueError)):
        with pytest.raises(err):
            bad()
    assert lib.calls == [] and len(lib.sets) == 4


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in ("msmz_scalars_dot_many", "msmz_test_dot_many_geometry", "msmz_test_set_dot_many_groups"):
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    assert (_native.MSMZ_DOT_MANY_MAX_ROWS, _native.MSMZ_DOT_MANY_MAX_COLS) == (128, 8)
    header = open(os.path.join(ROOT, "include", "msmz.h")).read()
    assert "enum { MSMZ_DOT_MANY_MAX_ROWS = 128, MSMZ_DOT_MANY_MAX_COLS = 8 };" in header
    assert ("int msmz_scalars_dot_many(msmz_ctx* ctx, const msmz_dot_many* d, uint8_t* out_le32, uint64_t first_out, "
            "uint64_t* out_handle);") in header


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof and the offset of every field of msmz_scalar_vec and msmz_dot_many, and the two limits, C side == ctypes
    side.  msmz_dot_many in the field order of the header (pointer, count, pointer, count, n, flags) is 48 bytes on an
    LP64 target: each count is followed by four bytes of padding in front of the next 8-byte field."""
    from msm_zprize_amd import _native as N
    prints, want = [], []
    for cname, ctype in (("msmz_scalar_vec", N.MsmzScalarVec), ("msmz_dot_many", N.MsmzDotMany)):
        prints.append(f'printf("%zu ", sizeof({cname}));')
        want.append(C.sizeof(ctype))
        for fname, _ in ctype._fields_:
            prints.append(f'printf("%zu ", offsetof({cname}, {fname}));')
            want.append(getattr(ctype, fname).offset)
    prints.append('printf("%d %d ", MSMZ_DOT_MANY_MAX_ROWS, MSMZ_DOT_MANY_MAX_COLS);')
    want += [N.MSMZ_DOT_MANY_MAX_ROWS, N.MSMZ_DOT_MANY_MAX_COLS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msmz.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()] == want
    assert want == [16, 0, 8, 48, 0, 8, 16, 24, 32, 40, 128, 8]


def test_geometry_accessor(lib):
    """msmz_test_dot_many_geometry == the constants the host driver was compiled with; the tile is msmz_scalars_dot's;
    needs no context"""
    tile, groups, dot_tile, rg = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), (C.c_uint32 * 8)()
    lib.msmz_test_dot_many_geometry(C.byref(tile), C.byref(groups), rg)
    lib.msmz_test_scalar_dot_geometry(C.byref(dot_tile), None)
    g = _geometry()
    assert (tile.value, groups.value, list(rg)) == (g["tile"], g["groups"], g["rg"]) and tile.value == dot_tile.value
    lib.msmz_test_dot_many_geometry(None, None, None)


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG and the outputs untouched"""
    from msm_zprize_amd import _native as N
    v = (N.MsmzScalarVec * 1)(N.MsmzScalarVec(1, 0))
    d = N.MsmzDotMany(v, 1, v, 1, 4, 0)
    h = C.c_uint64(0)
    buf = C.create_string_buffer(b"\xaa" * 32, 32)
    assert lib.msmz_scalars_dot_many(None, C.byref(d), buf, 0, C.byref(h)) == 1
    assert h.value == 0 and buf.raw == b"\xaa" * 32
    assert lib.msmz_test_set_dot_many_groups(None, 1) == 1
