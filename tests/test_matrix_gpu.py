"""Sparse matrices over resident scalar sets on the GPU (k_matrix_pack / k_matrix_mul / k_matrix_fold,
csrc/matrix_kernels.h) through the C ABI and the Python methods, byte for byte against Python integers mod the group
order (tests/matrix_util.py).  Sizes come from msmz_test_matrix_geometry: around one run, a wave of runs, one tile, and
past two and three tiles; the row structures put segment boundaries on and across the run and tile edges.  Then the
identities a product must keep (transpose, adjoint, gather), the output rules, every error, and an R1CS taken from its
witness through the three products into a whole sumcheck."""
import ctypes as C
import random

import pytest

import matrix_util as M
import mle_util as MLE
import scalar_ops_util as S

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
MAIN = ["bls12-377", "pallas"]


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


@pytest.fixture(scope="module")
def curves(mod):
    cache = {}

    def get(label):
        if label not in cache:
            params = mod.curves.BY_LABEL[label]
            cache[label] = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


def _geometry():
    t, r, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _lib().msmz_test_matrix_geometry(C.byref(t), C.byref(r), C.byref(p))
    return t.value, r.value, p.value


def _upload(curve, vals):
    return curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set: msmz_import_scalars_into converts before it reports, so after
    its MSMZ_ERR_RANGE the refused value is what the handle holds (as tests/test_scalar_ops_gpu.py does)"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


def _product(curve, rows, cols, vals, x_arr, shape, transpose=False):
    """one matrix, one product, everything freed: the result as ints"""
    m = curve.Parallel.sparseMatrix(rows, cols, vals, shape=shape, orientations="cols" if transpose else "rows")
    y = curve.Parallel.matVec(m, x_arr, transpose=transpose)
    got = curve.Scalar.toBigints(y)
    y.free(); m.free()
    return got


# -- the C ABI, status and outputs as they are ------------------------------------------------------------------
def _c_create(curve, rows, cols, n_rows, n_cols, vals=0, val_first=0, flags=0, nnz=None, h0=0, null=()):
    from msm_zprize_amd._native import MsmzSparse
    r = (C.c_uint32 * max(1, len(rows)))(*rows)
    c = (C.c_uint32 * max(1, len(cols)))(*cols)
    s = MsmzSparse(None if "row" in null else r, None if "col" in null else c, vals if isinstance(vals, int) else vals.handle,
                   val_first, len(rows) if nnz is None else nnz, n_rows, n_cols, flags)
    h = C.c_uint64(h0)
    st = _lib().msmz_matrix_create(curve._ctx, None if "s" in null else C.byref(s), None if "h" in null else C.byref(h))
    return st, h.value


def _c_mul(curve, m, x, x_first=0, flags=0, first_out=0, out=0):
    from msm_zprize_amd._native import MsmzMatvec
    v = MsmzMatvec(m if isinstance(m, int) else m.handle, x if isinstance(x, int) else x.handle, x_first, flags)
    h = C.c_uint64(out if isinstance(out, int) else out.handle)
    st = _lib().msmz_matrix_mul(curve._ctx, C.byref(v), first_out, C.byref(h))
    return st, h.value


# -- every size x every structure -------------------------------------------------------------------------------
def _run_structures(curve, label, nnz, seed):
    q = S.order(label)
    T, E, _ = _geometry()
    rng = random.Random(seed)
    n_cols = max(1, min(nnz, 61))
    x = M.x_for(n_cols, q, rng)
    x_arr = _upload(curve, x)
    bad = []
    for si, (name, (rows, n_rows)) in enumerate(M.structures(nnz, T, E, seed).items()):
        cols = M.columns(nnz, n_cols, rng, duplicates=si % 2 == 0)
        vals = M.values_for(nnz, q, rng)
        if si % 3 == 0:
            rows, cols, vals = M.shuffled(rows, cols, vals, rng)
        for v in (vals, None):
            got = _product(curve, rows, cols, v, x_arr, (n_rows, n_cols))
            if got != M.matvec(rows, cols, v, x, n_rows, q):
                bad.append((name, v is None))
    x_arr.free()
    assert not bad, bad


def _size_ids():
    return ["1", "E-1", "E", "E+1", "64E-1", "64E", "T-1", "T", "T+1", "2T+5", "3T"]


@pytest.mark.parametrize("which", range(11), ids=_size_ids())
@pytest.mark.parametrize("label", MAIN)
def test_sizes_and_structures(curves, label, which):
    """nnz over the run and tile edges x {one row (carries chain across every tile); one non-zero per row; a row from
    the last run of tile 0 to the first run of tile 2; boundaries exactly on run and tile edges; empty rows first, last
    and at the tile edge; power-law lengths}, with duplicate pairs, shuffled triples, values over {0, 1, q - 1, random}
    and the value-less form, x holding 0 and q - 1: byte for byte the Python model"""
    T, E, _ = _geometry()
    _run_structures(curves(label), label, M.sizes(T, E)[which], 100 * MAIN.index(label) + which)


@pytest.mark.parametrize("label", ["bls12-381", "ed-on-bls12-377"])
def test_other_curves(curves, label):
    T, E, _ = _geometry()
    _run_structures(curves(label), label, 2 * T + 5, 7 + S.ALL.index(label))


def test_fold_loops_over_passes(curves):
    """more tiles than the one workgroup of the fold takes per pass (carries_per_pass of the geometry hook): one row over
    all of them, so the sum crosses from pass to pass; a row that ends exactly with the last tile of the first pass; a row
    per tile; tiles in pairs.  Value-less: the products are not what this is about"""
    import array
    label = "pallas"
    curve, q = curves(label), S.order(label)
    T, _, P = _geometry()
    rng = random.Random(27)
    nnz = (P + 2) * T + 3
    x = M.x_for(17, q, rng)
    x_arr = _upload(curve, x)
    cols = array.array("I", M.columns(nnz, 17, rng))
    for rows in ([0] * nnz, [0] * (P * T) + [2] * (nnz - P * T), [k // T for k in range(nnz)], [k // (2 * T) for k in range(nnz)]):
        n_rows = max(rows) + 2
        assert _product(curve, array.array("I", rows), cols, None, x_arr, (n_rows, 17)) == M.matvec(rows, cols, None, x, n_rows, q)
    x_arr.free()


# -- identities -------------------------------------------------------------------------------------------------
def _random_matrix(q, rng, n_rows, n_cols, nnz):
    rows = [rng.randrange(n_rows) for _ in range(nnz)]
    cols = [rng.randrange(n_cols) for _ in range(nnz)]
    # (column 0 is referenced by every third triple: the transposed form has one long row)
    cols = [0 if k % 3 == 0 else c for k, c in enumerate(cols)]
    return rows, cols, M.values_for(nnz, q, rng)


@pytest.mark.parametrize("label", MAIN)
def test_transpose_and_adjoint(curves, label):
    """matVec(transpose=True) of a matrix built for both == matVec of the explicitly transposed matrix == the model;
    <y, M x> == <M^T y, x> through innerProduct; two calls return the same bytes"""
    curve, q = curves(label), S.order(label)
    T, E, _ = _geometry()
    rng = random.Random(21)
    n_rows, n_cols, nnz = 700, 300, T + 3 * E + 1
    rows, cols, vals = _random_matrix(q, rng, n_rows, n_cols, nnz)
    x, y = M.x_for(n_cols, q, rng), M.x_for(n_rows, q, rng)
    xa, ya = _upload(curve, x), _upload(curve, y)
    m = curve.Parallel.sparseMatrix(rows, cols, vals, shape=(n_rows, n_cols), orientations="both")
    mt = curve.Parallel.sparseMatrix(cols, rows, vals, shape=(n_cols, n_rows))
    assert (m.shape, m.nnz, mt.shape) == ((n_rows, n_cols), nnz, (n_cols, n_rows))
    mx = curve.Parallel.matVec(m, xa)
    mty = curve.Parallel.matVec(m, ya, transpose=True)
    mty2 = curve.Parallel.matVec(mt, ya)
    again = curve.Parallel.matVec(m, xa)
    assert curve.Scalar.toBigints(mx) == M.matvec(rows, cols, vals, x, n_rows, q) == curve.Scalar.toBigints(again)
    assert curve.Scalar.toBigints(mty) == curve.Scalar.toBigints(mty2) == M.matvec(rows, cols, vals, y, n_cols, q, transpose=True)
    assert curve.Parallel.innerProduct(ya, mx) == curve.Parallel.innerProduct(mty, xa)
    for a in (xa, ya, mx, mty, mty2, again, m, mt):
        a.free()


@pytest.mark.parametrize("label", MAIN)
def test_gather(curves, label):
    """a 0/1 matrix with one entry per row, value-less and with explicit ones: the rows of x it selects"""
    curve, q = curves(label), S.order(label)
    T, _, _ = _geometry()
    rng = random.Random(22)
    n, n_cols = T + 77, 500
    x_arr = curve.Parallel.randomScalars(n_cols, 5)
    x = curve.Scalar.toBigints(x_arr)
    pick = [rng.randrange(n_cols) for _ in range(n)]
    want = [x[j] for j in pick]
    assert _product(curve, list(range(n)), pick, None, x_arr, (n, n_cols)) == want
    assert _product(curve, list(range(n)), pick, [1] * n, x_arr, (n, n_cols)) == want
    x_arr.free()


# -- the output rules -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_output_into_a_range_and_overlaps(curves, label):
    """a new handle; a range of another set and of x's own set apart from x, the guard entries on both sides unchanged
    (rows without entries are written as 0 over what was there); every overlap with the x range, the exact one
    included, is MSMZ_ERR_ARG with nothing written"""
    curve, q = curves(label), S.order(label)
    rng = random.Random(23)
    n_rows, n_cols, nnz = 40, 48, 150
    rows = [rng.randrange(1, n_rows - 1) for _ in range(nnz)]       # rows 0 and n_rows - 1 are empty
    cols = [rng.randrange(n_cols) for _ in range(nnz)]
    vals = M.values_for(nnz, q, rng)
    big = M.x_for(200, q, rng)
    x_first = 100
    want = M.matvec(rows, cols, vals, big[x_first:x_first + n_cols], n_rows, q)
    assert want[0] == want[-1] == 0
    m = curve.Parallel.sparseMatrix(rows, cols, vals, shape=(n_rows, n_cols))
    arr, other = _upload(curve, big), _upload(curve, big)
    st, h = _c_mul(curve, m, arr, x_first)                          # a new handle
    assert st == 0 and h not in (0, arr.handle, other.handle, m.handle)
    from msm_zprize_amd.parallel import DeviceArray
    new = DeviceArray(curve, h, n_rows, "scalars")
    assert curve.Scalar.toBigints(new) == want
    new.free()
    y = curve.Parallel.matVec(m, arr, firstX=x_first, out=other, firstOut=7)
    assert y is other and curve.Scalar.toBigints(other) == big[:7] + want + big[7 + n_rows:]
    for first_out in (x_first - n_rows, x_first + n_cols, 0, 200 - n_rows):       # the same set, apart from x
        assert _c_mul(curve, m, arr, x_first, 0, first_out, arr) == (0, arr.handle)
        expect = big[:first_out] + want + big[first_out + n_rows:]
        assert curve.Scalar.toBigints(arr) == expect
        arr.free()
        arr = _upload(curve, big)
    for first_out in (x_first, x_first - n_rows + 1, x_first + n_cols - 1, x_first + 3, x_first - 1):
        assert _c_mul(curve, m, arr, x_first, 0, first_out, arr) == (MSMZ_ERR_ARG, arr.handle)
        with pytest.raises(ValueError):
            curve.Parallel.matVec(m, arr, firstX=x_first, out=arr, firstOut=first_out)
    assert curve.Scalar.toBigints(arr) == big
    square = curve.Parallel.sparseMatrix([0, 1], [1, 0], shape=(2, 2))          # the exact range
    assert _c_mul(curve, square, arr, 10, 0, 10, arr) == (MSMZ_ERR_ARG, arr.handle)
    assert _c_mul(curve, square, arr, 10, 0, 12, arr) == (0, arr.handle)
    assert curve.Scalar.toBigints(arr) == big[:12] + [big[11], big[10]] + big[14:]
    square.free()
    for a in (arr, other, m):
        a.free()


# -- MSMZ_ERR_RANGE ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_value_not_below_q(curves, label):
    """a value >= q at the first, a middle and the last non-zero of the value range: MSMZ_ERR_RANGE, no handle made, the
    context usable; just outside the range on either side it is not read"""
    curve, q = curves(label), S.order(label)
    T, _, _ = _geometry()
    rng = random.Random(24)
    nnz, first = T + 9, 5
    rows = [rng.randrange(30) for _ in range(nnz)]
    cols = [rng.randrange(20) for _ in range(nnz)]
    x = M.x_for(20, q, rng)
    x_arr = _upload(curve, x)
    for index, status in ((first, MSMZ_ERR_RANGE), (first + nnz // 2, MSMZ_ERR_RANGE), (first + nnz - 1, MSMZ_ERR_RANGE),
                          (first - 1, 0), (first + nnz, 0)):
        vals = S.random_below_2_250(nnz + 10, rng)
        arr = _upload(curve, vals)
        _plant(curve, arr, index, q if index % 2 else (1 << 256) - 1)
        for flags in (1, 3):
            st, h = _c_create(curve, rows, cols, 30, 20, arr, first, flags, h0=55)
            assert st == status and (h == 55) == (status != 0)
            if status == 0:
                _lib().msmz_free(curve._ctx, h)
        # the context is usable and no handle was left behind: ids go up by one per handle made
        m = curve.Parallel.sparseMatrix(rows, cols, vals[first:first + nnz], shape=(30, 20))   # (uploads a set: one id)
        y = curve.Parallel.matVec(m, x_arr)
        assert curve.Scalar.toBigints(y) == M.matvec(rows, cols, vals[first:first + nnz], x, 30, q)
        st, h2 = _c_create(curve, rows, cols, 30, 20, arr, first, 1)
        assert st == status and (status != 0 or h2 == y.handle + 1)
        if status == 0:
            _lib().msmz_free(curve._ctx, h2)
        else:
            probe = curve.Parallel.randomScalars(1, 1)
            assert probe.handle == y.handle + 1
            probe.free()
        for a in (arr, m, y):
            a.free()
    x_arr.free()


@pytest.mark.parametrize("label", MAIN)
def test_entry_of_x_not_below_q(curves, label):
    """an entry of x >= q that a non-zero reads: MSMZ_ERR_RANGE, *out_handle as it was and no handle made; one that no
    non-zero reads -- inside the x range, or just outside it -- is not an error, with values and without"""
    curve, q = curves(label), S.order(label)
    T, _, _ = _geometry()
    rng = random.Random(25)
    nnz, n_cols, x_first = T + 9, 24, 3
    unread = 11
    cols = [c if c != unread else 12 for c in (rng.randrange(n_cols) for _ in range(nnz))]
    cols[0], cols[nnz // 2], cols[-1] = 0, 5, n_cols - 1
    rows = [rng.randrange(30) for _ in range(nnz)]
    vals = M.values_for(nnz, q, rng)
    x = M.x_for(n_cols + 6, q, rng)
    for values in (vals, None):
        m = curve.Parallel.sparseMatrix(rows, cols, values, shape=(30, n_cols), orientations="both")
        for index, status in ((x_first + 0, MSMZ_ERR_RANGE), (x_first + 5, MSMZ_ERR_RANGE), (x_first + n_cols - 1, MSMZ_ERR_RANGE),
                              (x_first + unread, 0), (x_first - 1, 0), (x_first + n_cols, 0)):
            arr = _upload(curve, x)
            _plant(curve, arr, index, q)
            st, h = _c_mul(curve, m, arr, x_first)
            assert st == status and (h == 0) == (status != 0)
            if status == 0:
                from msm_zprize_amd.parallel import DeviceArray
                y = DeviceArray(curve, h, 30, "scalars")
                assert curve.Scalar.toBigints(y) == M.matvec(rows, cols, values, x[x_first:x_first + n_cols], 30, q)
                y.free()
            else:
                probe = curve.Parallel.randomScalars(1, 1)      # no handle leaked: the next id follows arr's
                assert probe.handle == arr.handle + 1
                probe.free()
            arr.free()
        # the transposed product reads x by row index
        arr = _upload(curve, M.x_for(30, q, rng))
        _plant(curve, arr, rows[7], q + 1)
        assert _c_mul(curve, m, arr, 0, 1) == (MSMZ_ERR_RANGE, 0)
        arr.free(); m.free()


# -- MSMZ_ERR_ARG -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_argument_errors(curves, label):
    """every argument error of the two calls, the outputs untouched; a handle of the wrong kind either way; a wrong
    orientation; msmz_free of a matrix"""
    curve, q = curves(label), S.order(label)
    lib = _lib()
    rows, cols = [0, 1, 2, 2], [1, 0, 3, 3]
    sc = curve.Parallel.randomScalars(16, 2)
    pts = curve.Parallel.randomPointsFast(16, 2)
    ok = dict(rows=rows, cols=cols, n_rows=3, n_cols=4)
    bad = [dict(ok, null=("s",)), dict(ok, null=("row",)), dict(ok, null=("col",)), dict(ok, null=("h",)),
           dict(ok, nnz=0), dict(ok, nnz=1 << 32), dict(ok, n_rows=0), dict(ok, n_cols=0),
           dict(ok, n_rows=2), dict(ok, n_cols=3), dict(ok, rows=[0, 1, 2, 3]), dict(ok, cols=[1, 0, 3, 4]),
           dict(ok, flags=4), dict(ok, flags=0x80000001), dict(ok, vals=999), dict(ok, vals=pts), dict(ok, vals=sc, val_first=13),
           dict(ok, vals=sc, val_first=(1 << 64) - 1), dict(ok, val_first=1)]
    for kw in bad:
        st, h = _c_create(curve, **dict(kw, h0=55))
        assert (st, h) == (MSMZ_ERR_ARG, 55), kw
    st, mh = _c_create(curve, vals=sc, val_first=12, **ok)        # the last four values of the set; flags 0 = ROWS
    assert st == 0
    r, c, n, f = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    assert lib.msmz_matrix_info(curve._ctx, mh, C.byref(r), C.byref(c), C.byref(n), C.byref(f)) == 0
    assert (r.value, c.value, n.value, f.value) == (3, 4, 4, 1)
    assert lib.msmz_matrix_info(curve._ctx, mh, None, None, None, None) == 0
    for h in (sc.handle, pts.handle, 999, 0):
        assert lib.msmz_matrix_info(curve._ctx, h, C.byref(r), None, None, None) == MSMZ_ERR_ARG
    st, both = _c_create(curve, flags=3, **ok)
    assert st == 0
    # matrix_mul
    for args in ((999, sc), (0, sc), (sc.handle, sc), (pts.handle, sc),                    # the matrix
                 (mh, 999), (mh, 0), (mh, pts), (mh, mh), (mh, sc, 13), (mh, sc, (1 << 64) - 2),       # x
                 (mh, sc, 0, 2), (mh, sc, 0, 1),                                            # flags; built for ROWS only
                 (mh, sc, 0, 0, 1), (mh, sc, 0, 0, 0, 999), (mh, sc, 0, 0, 0, pts), (mh, sc, 0, 0, 0, mh),   # the destination
                 (mh, sc, 0, 0, 14, sc), (both, sc, 0, 1, 13, sc)):
        out = args[5] if len(args) > 5 else 0
        st, h = _c_mul(curve, *args)
        assert (st, h) == (MSMZ_ERR_ARG, out if isinstance(out, int) else out.handle), args
    st, cols_only = _c_create(curve, flags=2, **ok)
    assert st == 0 and _c_mul(curve, cols_only, sc) == (MSMZ_ERR_ARG, 0)
    st, h = _c_mul(curve, cols_only, sc, 0, 1)
    assert st == 0
    assert lib.msmz_free(curve._ctx, h) == 0
    from msm_zprize_amd._native import MsmzMatvec
    v = MsmzMatvec(mh, sc.handle, 0, 0)
    hh = C.c_uint64(0)
    assert lib.msmz_matrix_mul(curve._ctx, None, 0, C.byref(hh)) == MSMZ_ERR_ARG
    assert lib.msmz_matrix_mul(curve._ctx, C.byref(v), 0, None) == MSMZ_ERR_ARG
    # a matrix handle where the older calls want a point or scalar set
    from msm_zprize_amd._native import MsmzError
    from msm_zprize_amd.parallel import DeviceArray
    fake = DeviceArray(curve, mh, 4, "scalars")
    fake_pts = DeviceArray(curve, mh, 4, "points")
    for call in (lambda: curve.Scalar.toBigints(fake), lambda: curve.Parallel.combineScalars(1, fake),
                 lambda: curve.Parallel.combineScalars(2, sc, N=4, out=fake), lambda: curve.Parallel.innerProduct(fake),
                 lambda: curve.Parallel.msm(fake, pts, 4), lambda: curve.Parallel.msm(sc, fake_pts, 4)):
        with pytest.raises(MsmzError) as e:
            call()
        assert e.value.status == MSMZ_ERR_ARG
    # the Python checks refuse before the library is asked
    m = curve.Parallel.sparseMatrix(rows, cols, shape=(3, 4))
    with pytest.raises(TypeError):
        curve.Parallel.matVec(sc, sc)
    with pytest.raises(TypeError):
        curve.Parallel.matVec(m, pts)
    with pytest.raises(ValueError):
        curve.Parallel.matVec(m, sc, transpose=True)
    with pytest.raises(ValueError):
        curve.Parallel.sparseMatrix(rows, [1, 0, 3, 4], shape=(3, 4))
    # msmz_free frees a matrix, once
    for h in (mh, both, cols_only):
        assert lib.msmz_free(curve._ctx, h) == 0
        assert lib.msmz_free(curve._ctx, h) == MSMZ_ERR_ARG
        assert _c_mul(curve, h, sc) == (MSMZ_ERR_ARG, 0)
    m.free()
    assert m.handle is None
    with pytest.raises(ValueError):
        curve.Parallel.matVec(m, sc)
    # the matrix kept its own copy of the values: the set may change or go
    vals = _upload(curve, [3, 4, 5, 6])
    m = curve.Parallel.sparseMatrix(rows, cols, vals, shape=(3, 4))
    curve.Parallel.combineScalars(2, vals, out=vals)
    vals.free()
    x = _upload(curve, [1, 10, 100, 1000])
    y = curve.Parallel.matVec(m, x)
    assert curve.Scalar.toBigints(y) == [3 * 10, 4 * 1, 11 * 1000]
    for a in (m, x, y, sc, pts):
        a.free()


@pytest.mark.parametrize("label", MAIN)
def test_multi_engine_context_is_unsupported(mod, label):
    """devices = [0, 0]: a gather reads across every block of 2^16 entries -- the calls answer MSMZ_ERR_UNSUPPORTED and
    leave their outputs as they were; the older calls on the same context still work"""
    mod.startThreads(devices=[0, 0])
    params = mod.curves.BY_LABEL[label]
    multi = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
    try:
        f = multi.Parallel.randomScalars(64, 3)
        assert _c_create(multi, [0, 1], [1, 0], 2, 2, h0=55) == (MSMZ_ERR_UNSUPPORTED, 55)
        assert _c_mul(multi, 1, f) == (MSMZ_ERR_UNSUPPORTED, 0)
        r = C.c_uint32(9)
        assert _lib().msmz_matrix_info(multi._ctx, 1, C.byref(r), None, None, None) == MSMZ_ERR_UNSUPPORTED and r.value == 9
        assert multi.Parallel.innerProduct(f) == sum(multi.Scalar.toBigints(f)) % S.order(label)
        f.free()
    finally:
        multi.close()
        mod.startThreads()


# -- end to end: witness -> Az, Bz, Cz -> sumcheck --------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_r1cs_through_a_whole_sumcheck(curves, label):
    """2^6 constraints over 2^6 variables: sparse random A and B, a random witness z, C with one entry per row chosen so
    that Cz = Az o Bz.  The three tables come from three products on the device; with an eq table, the first round of
    the sumcheck over eq (A B) - eq C gives g(0) + g(1) == 0, and the whole protocol with bindMle ends in the value the
    model predicts; the transposed product against the eq table is the model's too"""
    curve, q = curves(label), S.order(label)
    rng = random.Random(26 + MAIN.index(label))
    v = 6
    n = 1 << v
    z = [1] + [rng.randrange(q) for _ in range(n - 1)]

    def sparse_rows():
        rows, cols, vals = [], [], []
        for i in range(n):
            for j in rng.sample(range(n), rng.randrange(1, 4)) + ([0] if i % 2 else []):   # (the constant column)
                rows.append(i); cols.append(j); vals.append(rng.choice([1, q - 1, rng.randrange(q)]))
        return rows, cols, vals

    A, B = sparse_rows(), sparse_rows()
    az, bz = M.matvec(*A, z, n, q), M.matvec(*B, z, n, q)
    c_cols = [rng.randrange(1, n) for _ in range(n)]
    c_cols = [j if z[j] else 0 for j in c_cols]
    Cm = (list(range(n)), c_cols, [az[i] * bz[i] * pow(z[c_cols[i]], -1, q) % q for i in range(n)])
    assert M.matvec(*Cm, z, n, q) == [a * b % q for a, b in zip(az, bz)]
    z_arr = _upload(curve, z)
    mats = [curve.Parallel.sparseMatrix(r, c, w, shape=(n, n), orientations="both") for r, c, w in (A, B, Cm)]
    tabs = [curve.Parallel.matVec(m, z_arr) for m in mats]
    assert [curve.Scalar.toBigints(t) for t in tabs] == [az, bz, M.matvec(*Cm, z, n, q)]
    tau = [rng.randrange(q) for _ in range(v)]
    eq = curve.Parallel.eqTable(tau)
    tables = [eq] + tabs
    model = [MLE.eq(tau, q), az, bz, M.matvec(*Cm, z, n, q)]
    terms = [(None, 0b0111), (q - 1, 0b1001)]
    claim = 0
    point = []
    for rnd in range(v):
        g = curve.Parallel.sumcheckRound(tables, terms, nVars=v - rnd)
        assert g == MLE.round_poly(model, terms, q, False)
        assert (g[0] + g[1]) % q == claim
        r = rng.randrange(q)
        point.append(r)
        claim = MLE.interpolate(g, r, q)
        tables = [curve.Parallel.bindMle(t, r, nVars=v - rnd, out=t) for t in tables]
        model = [MLE.bind(t, r, q) for t in model]
    e, a, b, c = (curve.Scalar.toBigints(t, 0, 1)[0] for t in tables)
    assert [e, a, b, c] == [t[0] for t in model]
    assert e * (a * b - c) % q == claim
    # Spartan's second table: (r_A A + r_B B + r_C C)^T eq(r_x), r_x the point bound above in the round order
    rx = point[::-1]                               # (the rounds bound the high variable first)
    eq_rx = curve.Parallel.eqTable(rx)
    assert (sum(x * y for x, y in zip(MLE.eq(rx, q), az)) % q) == a
    cols_t = [curve.Parallel.matVec(m, eq_rx, transpose=True) for m in mats]
    for t, mat in zip(cols_t, (A, B, Cm)):
        assert curve.Scalar.toBigints(t) == M.matvec(*mat, MLE.eq(rx, q), n, q, transpose=True)
    assert curve.Parallel.innerProduct(cols_t[0], z_arr) == a      # <A^T eq(r_x), z> == (Az)(r_x)
    for x in [z_arr, eq, eq_rx] + mats + tabs + cols_t:
        x.free()
