"""msmz_scalars_dot_many on the GPU (k_scalars_dot_many, csrc/dot_kernels.h) through the C ABI and the Python methods: bit
for bit against Python integers (tests/dot_many_util.py) AND against msmz_scalars_dot, pair by pair.  Every vector of a
case is a range of ONE scalar set, at a non-zero first, 7 entries from its neighbours: rows and columns share a handle
and overlap.  Sizes around a wave, a workgroup pass and a tile; shapes at one result, one row of every column count,
a row tail, both limits.  Then a lowered workgroup bound, the destinations, the error paths, a context of two engines
and scratch that was poisoned before the call."""
import ctypes as C
import random

import pytest

import dot_many_util as U
import scalar_ops_util as S

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
MAIN = "bls12-377"
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5)
FILL = b"\xaa"


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


def _create(mod, label):
    params = mod.curves.BY_LABEL[label]
    return (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)


@pytest.fixture(scope="module")
def curves(mod):
    cache = {}

    def get(label):
        if label not in cache:
            cache[label] = _create(mod, label)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


def _geometry():
    tile, groups, rg = C.c_uint32(0), C.c_uint32(0), (C.c_uint32 * 8)()
    _lib().msmz_test_dot_many_geometry(C.byref(tile), C.byref(groups), rg)
    return tile.value, groups.value, list(rg)


def _shapes():
    """one result; one row of the most columns; a few rows of one column; one row more than a block of three columns; the
    most rows"""
    rg3 = _geometry()[2][2]
    return [(1, 1), (1, 8), (3, 1), (rg3 + 1, 3), (128, 1)]


def _c_many(curve, rows, cols, n, host=True, handle=None, first_out=0, flags=0, n_rows=None, n_cols=None):
    """rows / cols: [(array or raw handle, first)] or None; handle: None (no resident destination), 0 (a new set) or an
    array -> (status, the host bytes or None, the handle word afterwards or None)"""
    from msm_zprize_amd import _native as N

    def pack(pairs):
        if pairs is None:
            return None
        return (N.MsmzScalarVec * max(1, len(pairs)))(*[N.MsmzScalarVec(a if isinstance(a, int) else a.handle, f) for a, f in pairs])

    nr = len(rows or ()) if n_rows is None else n_rows
    nc = len(cols or ()) if n_cols is None else n_cols
    d = N.MsmzDotMany(pack(rows), nr, pack(cols), nc, n, flags)
    size = 32 * max(1, min(nr, 128) * min(nc, 8))
    buf = C.create_string_buffer(FILL * size, size) if host else None
    h = None if handle is None else C.c_uint64(handle if isinstance(handle, int) else handle.handle)
    st = _lib().msmz_scalars_dot_many(curve._ctx, C.byref(d), buf, first_out, None if h is None else C.byref(h))
    return st, None if buf is None else buf.raw, None if h is None else h.value


def _dot(curve, x, fx, y, fy, n):
    buf = C.create_string_buffer(32)
    assert _lib().msmz_scalars_dot(curve._ctx, x.handle, fx, y.handle, fy, n, buf) == 0
    return buf.raw


def _check_pool(curve, label, n, shapes, seed):
    """one pool per (curve, n); every shape reads rows from vector 0 on and columns from vector 130 on"""
    q = S.order(label)
    values = U.pool(label, n, seed)
    arr = curve.Parallel.scalarsFromBytes(S.encode(values), len(values))
    try:
        for n_rows, n_cols in shapes:
            rk, ck = list(range(n_rows)), [U.MAX_ROWS + 2 + c for c in range(n_cols)]
            want = U.products([U.vector(values, k, n) for k in rk], [U.vector(values, k, n) for k in ck], q)
            st, raw, _ = _c_many(curve, [(arr, U.first(k)) for k in rk], [(arr, U.first(k)) for k in ck], n)
            assert st == 0, (n, n_rows, n_cols)
            assert raw == S.encode([v for row in want for v in row]), (n, n_rows, n_cols)
            pairs = b"".join(_dot(curve, arr, U.first(r), arr, U.first(c), n) for r in rk for c in ck)
            assert raw == pairs, (n, n_rows, n_cols)
    finally:
        arr.free()


@pytest.mark.parametrize("n", SIZES)
def test_every_shape_at_every_size(curves, n):
    shapes = _shapes() + ([(128, 8)] if n == 65 else [])
    _check_pool(curves(MAIN), MAIN, n, shapes, 700 + n)


@pytest.mark.parametrize("label", S.ALL)
def test_all_curves(curves, label):
    rg3 = _geometry()[2][2]
    _check_pool(curves(label), label, 257, [(rg3 + 1, 3)], 31)
    _check_pool(curves(label), label, 2049, [(1, 8)], 32)


def test_workgroups_stride_over_the_tiles(curves):
    """with the workgroup bound lowered to 2, the 5 tiles of 10 000 entries make every workgroup stride two or three
    times; a bound above the built-in one is refused and 0 restores it"""
    curve = curves(MAIN)
    tile, groups, rg = _geometry()
    n = 10_000
    assert n > 4 * tile
    assert _lib().msmz_test_set_dot_many_groups(curve._ctx, groups + 1) == MSMZ_ERR_ARG
    assert _lib().msmz_test_set_dot_many_groups(None, 2) == MSMZ_ERR_ARG
    assert _lib().msmz_test_set_dot_many_groups(curve._ctx, 2) == 0
    try:
        _check_pool(curve, MAIN, n, [(rg[1] + 1, 2), (5, 4), (2, 8)], 33)
    finally:
        assert _lib().msmz_test_set_dot_many_groups(curve._ctx, 0) == 0
    _check_pool(curve, MAIN, n, [(rg[1] + 1, 2)], 33)


def test_one_range_as_row_and_column_and_constant_vectors(curves):
    """a row that IS a column (a sum of squares), all-zero and all-(q - 1) vectors, at a tile and a bit"""
    curve, q = curves(MAIN), S.order(MAIN)
    par = curve.Parallel
    n = _geometry()[0] + 67
    values = U.pool(MAIN, n, 34)
    a = par.scalarsFromBytes(S.encode(values), len(values))
    zero = par.scalarsFromBytes(bytes(32 * n), n)
    top = par.scalarsFromBytes(S.encode([q - 1]) * n, n)
    try:
        x, y = U.vector(values, 0, n), U.vector(values, 1, n)
        rows = [(a, U.first(0)), (zero, 0), (top, 0), (a, U.first(1))]
        cols = [(a, U.first(0)), (top, 0), (zero, 0)]
        want = U.products([x, [0] * n, [q - 1] * n, y], [x, [q - 1] * n, [0] * n], q)
        assert want[0][0] == sum(v * v for v in x) % q and want[2][1] == n % q and want[1] == [0, 0, 0]
        st, raw, _ = _c_many(curve, rows, cols, n)
        assert st == 0 and raw == S.encode([v for row in want for v in row])
        assert par.innerProducts([a, zero], [(a, 0), top], n) == U.products([values[:n], [0] * n], [values[:n], [q - 1] * n], q)
    finally:
        for arr in (a, zero, top):
            arr.free()


def test_destinations(curves):
    """to the host only, to a new set only, to both, and into a range of an existing set whose neighbours stay; the
    resident values then pass through combineScalars unchanged"""
    curve, q = curves(MAIN), S.order(MAIN)
    par = curve.Parallel
    n, n_rows, n_cols = 300, 5, 3
    values = U.pool(MAIN, n, 35)
    a = par.scalarsFromBytes(S.encode(values), len(values))
    rows = [(a, U.first(k)) for k in range(n_rows)]
    cols = [(a, U.first(40 + k)) for k in range(n_cols)]
    want = U.products([U.vector(values, k, n) for k in range(n_rows)], [U.vector(values, 40 + k, n) for k in range(n_cols)], q)
    flat = [v for row in want for v in row]
    made = []
    try:
        st, raw, _ = _c_many(curve, rows, cols, n)
        assert (st, raw) == (0, S.encode(flat))
        st, raw, h = _c_many(curve, rows, cols, n, host=False, handle=0)
        assert st == 0 and raw is None and h != 0
        from msm_zprize_amd.parallel import DeviceArray
        made.append(DeviceArray(curve, h, len(flat), "scalars"))
        assert curve.Scalar.toBigints(made[-1]) == flat
        st, raw, h = _c_many(curve, rows, cols, n, host=True, handle=0)
        assert st == 0 and raw == S.encode(flat) and h != 0
        made.append(DeviceArray(curve, h, len(flat), "scalars"))
        assert curve.Scalar.toBigints(made[-1]) == flat
        dest = par.scalarsFromBytes(S.encode([7] * (len(flat) + 9)), len(flat) + 9)
        made.append(dest)
        assert par.innerProducts(rows, cols, n, out=dest, firstOut=4) is dest
        assert curve.Scalar.toBigints(dest) == [7] * 4 + flat + [7] * 5
        same = par.combineScalars(1, dest, N=len(flat), firstX=4)
        made.append(same)
        assert curve.Scalar.toBigints(same) == flat
        assert par.innerProducts(rows, cols, n) == want
        # the destination inside the set the vectors come from, apart from every range read
        tail = U.first(40 + n_cols - 1) + n
        assert len(values) - tail >= len(flat)
        assert par.innerProducts(rows, cols, n, out=a, firstOut=tail) is a
        assert curve.Scalar.toBigints(a) == values[:tail] + flat + values[tail + len(flat):]
    finally:
        for arr in made + [a]:
            arr.free()


def test_evaluate_polynomials(curves):
    """5 polynomials of 300 coefficients at 0, 1, q - 1 and a random point, against Horner"""
    curve, q = curves(MAIN), S.order(MAIN)
    par = curve.Parallel
    rng = random.Random(36)
    values = U.pool(MAIN, 300, 36)
    a = par.scalarsFromBytes(S.encode(values), len(values))
    try:
        points = [0, 1, q - 1, rng.randrange(2, q - 1)]
        polys = [(a, U.first(k)) for k in range(5)]
        got = par.evaluatePolynomials(polys, points, 300)
        assert got == [[U.horner(U.vector(values, k, 300), z, q) for z in points] for k in range(5)]
        whole = par.evaluatePolynomials([a], [points[3]])
        assert whole == [[U.horner(values, points[3], q)]]
    finally:
        a.free()


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set: msmz_import_scalars_into converts before it reports, so after
    its MSMZ_ERR_RANGE the refused value is what the handle holds (as tests/test_mle_gpu.py does)"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


def test_resident_entry_out_of_range(curves):
    """q in the last element of the last row (the row tail of a block): MSMZ_ERR_RANGE, no handle, the host bytes as they
    were; the entry just outside the range is not read; and the next call is right"""
    curve, q = curves(MAIN), S.order(MAIN)
    par = curve.Parallel
    n, n_rows, n_cols = 2049, 3, 2
    values = U.pool(MAIN, n, 37)
    a = par.scalarsFromBytes(S.encode(values), len(values))
    b = par.scalarsFromBytes(S.encode(values), len(values))
    rows = [(a, U.first(k)) for k in range(n_rows)]
    cols = [(b, U.first(60 + k)) for k in range(n_cols)]
    at = U.first(n_rows - 1) + n - 1
    good = S.encode([values[at]])
    try:
        _plant(curve, a, at, q)
        st, raw, h = _c_many(curve, rows, cols, n, host=True, handle=0)
        assert (st, raw, h) == (MSMZ_ERR_RANGE, FILL * (32 * n_rows * n_cols), 0)
        with pytest.raises(Exception):
            par.innerProducts(rows, cols, n)
        # the same rows one entry shorter do not address the planted entry
        want = U.products([U.vector(values, k, n - 1) for k in range(n_rows)], [U.vector(values, 60 + k, n - 1) for k in range(n_cols)], q)
        assert par.innerProducts(rows, cols, n - 1) == want
        from msm_zprize_amd._native import MsmzSrc
        src = MsmzSrc(C.cast(C.c_char_p(good), C.c_void_p), 0, 32, 0, None, None)
        assert _lib().msmz_import_scalars_into(curve._ctx, a.handle, at, C.byref(src), 1) == 0
        want = U.products([U.vector(values, k, n) for k in range(n_rows)], [U.vector(values, 60 + k, n) for k in range(n_cols)], q)
        assert par.innerProducts(rows, cols, n) == want
    finally:
        a.free(), b.free()


def test_argument_errors_write_nothing(curves):
    """every MSMZ_ERR_ARG of the header: the outputs and the arrays stay; the neighbours of each are accepted"""
    curve = curves(MAIN)
    par = curve.Parallel
    a = par.randomScalars(64, 5)
    d = par.randomScalars(64, 6)
    pts = par.randomPoints(4, 1) if hasattr(par, "randomPoints") else None
    before = curve.Scalar.toBigints(a), curve.Scalar.toBigints(d)
    buf = C.create_string_buffer(64)
    arg = (MSMZ_ERR_ARG, FILL * 32, None)
    try:
        assert _lib().msmz_scalars_dot_many(curve._ctx, None, buf, 0, None) == MSMZ_ERR_ARG
        assert _c_many(curve, None, [(a, 0)], 8, n_rows=1)[0] == MSMZ_ERR_ARG
        assert _c_many(curve, [(a, 0)], None, 8, n_cols=1)[0] == MSMZ_ERR_ARG
        assert _c_many(curve, [(a, 0)], [(a, 0)], 8, host=False)[0] == MSMZ_ERR_ARG              # no destination at all
        assert _c_many(curve, [], [(a, 0)], 8) == arg and _c_many(curve, [(a, 0)], [], 8) == arg
        assert _c_many(curve, [(a, 0)] * 129, [(a, 0)], 8)[0] == MSMZ_ERR_ARG and _c_many(curve, [(a, 0)] * 128, [(a, 0)], 8)[0] == 0
        assert _c_many(curve, [(a, 0)], [(a, 0)] * 9, 8)[0] == MSMZ_ERR_ARG and _c_many(curve, [(a, 0)], [(a, 0)] * 8, 8)[0] == 0
        assert _c_many(curve, [(a, 0)], [(a, 0)], 0) == arg and _c_many(curve, [(a, 0)], [(a, 0)], 1 << 32) == arg
        assert _c_many(curve, [(a, 0)], [(a, 0)], 8, flags=1) == arg
        assert _c_many(curve, [(a, 0)], [(a, 0)], 8, first_out=1) == arg                         # first_out without a set
        assert _c_many(curve, [(a, 0)], [(a, 0)], 8, handle=0, first_out=1) == (MSMZ_ERR_ARG, FILL * 32, 0)
        assert _c_many(curve, [(a.handle + 1000, 0)], [(a, 0)], 8) == arg and _c_many(curve, [(0, 0)], [(a, 0)], 8) == arg
        if pts is not None:
            assert _c_many(curve, [(pts, 0)], [(a, 0)], 4) == arg                                # not a scalar set
        assert _c_many(curve, [(a, 57)], [(a, 0)], 8) == arg and _c_many(curve, [(a, 56)], [(a, 0)], 8)[0] == 0
        assert _c_many(curve, [(a, 0)], [(a, 65)], 1) == arg and _c_many(curve, [(a, 0)], [(a, 63)], 1)[0] == 0
        assert _c_many(curve, [(a, 0)], [(a, 0)], 8, handle=d, first_out=64) == (MSMZ_ERR_ARG, FILL * 32, d.handle)
        assert _c_many(curve, [(a, 0)], [(a, 0)], 8, handle=d, first_out=63)[0] == 0
        before = before[0], curve.Scalar.toBigints(d)
        # the destination on an input range of the same set: at its start, at its last entry, a column's; next to it: fine
        two = [(a, 0), (a, 8)]
        for first_out in (0, 7, 15, 19, 20, 27):
            got = _c_many(curve, two, [(a, 20)], 8, handle=a, first_out=first_out)
            assert got == (MSMZ_ERR_ARG, FILL * 64, a.handle), first_out
        assert (curve.Scalar.toBigints(a), curve.Scalar.toBigints(d)) == before
        assert _c_many(curve, two, [(a, 20)], 8, handle=a, first_out=28)[0] == 0
        assert _c_many(curve, two, [(a, 20)], 8, handle=a, first_out=16)[0] == 0
        with pytest.raises(ValueError):
            par.innerProducts(two, [(a, 20)], 8, out=a, firstOut=15)
        with pytest.raises(TypeError):
            par.innerProducts(a, [a])
    finally:
        a.free(), d.free()
        if pts is not None:
            pts.free()


def test_multi_engine_context_is_unsupported(mod):
    """devices = [0, 0]: MSMZ_ERR_UNSUPPORTED, the outputs as they were; msmz_scalars_dot on the same context still works"""
    mod.startThreads(devices=[0, 0])
    multi = _create(mod, MAIN)
    try:
        f = multi.Parallel.randomScalars(64, 3)
        assert _c_many(multi, [(f, 0)], [(f, 0)], 64, handle=0) == (MSMZ_ERR_UNSUPPORTED, FILL * 32, 0)
        assert _lib().msmz_test_set_dot_many_groups(multi._ctx, 2) == MSMZ_ERR_UNSUPPORTED
        assert multi.Parallel.innerProduct(f) == sum(multi.Scalar.toBigints(f)) % S.order(MAIN)
        f.free()
    finally:
        multi.close()
        mod.startThreads()


def test_scratch_poisoned_before_the_call(mod):
    """a fresh context: the same bytes before and after msmz_test_poison filled every scratch buffer and armed the
    allocations, on the host and in a new set (as tests/test_expr_poison_gpu.py)"""
    curve = _create(mod, MAIN)
    q = S.order(MAIN)
    par = curve.Parallel
    n = 3 * _geometry()[0] + 70
    values = U.pool(MAIN, n, 38)
    want = U.products([U.vector(values, k, n) for k in range(5)], [U.vector(values, 50 + k, n) for k in range(3)], q)

    def run():
        a = par.scalarsFromBytes(S.encode(values), len(values))
        rows, cols = [(a, U.first(k)) for k in range(5)], [(a, U.first(50 + k)) for k in range(3)]
        st, raw, h = _c_many(curve, rows, cols, n, host=True, handle=0)
        assert st == 0
        from msm_zprize_amd.parallel import DeviceArray
        new = DeviceArray(curve, h, 15, "scalars")
        got = raw, curve.Scalar.toBigints(new)
        a.free(), new.free()
        return got

    try:
        base = run()
        assert base == (S.encode([v for row in want for v in row]), [v for row in want for v in row])
        for pattern in (0x00, 0xa5, 0x5a):
            assert _lib().msmz_test_poison(curve._ctx, pattern, None, None) == 0
            assert run() == base, hex(pattern)
        assert _lib().msmz_test_poison(curve._ctx, -1, None, None) == 0
    finally:
        curve.close()
