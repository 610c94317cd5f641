"""Multiplicities of a column in a table on the GPU (k_lookup_insert / k_lookup_count / k_lookup_emit,
csrc/lookup_kernels.h) through the C ABI and the Python method, byte for byte against Python integers
(tests/lookup_util.py: collections.Counter plus the first index of each value).  Sizes come from
msmz_test_lookup_geometry: the smallest tables (2 and 4 slots, where every probe wraps), around a wave and a workgroup,
and past several workgroups; the tables make every thread of the insert race for one slot or walk one chain, the
columns put runs of equal values on and across wave and workgroup edges.  Then the output rules, every error, the
poisoned scratch, and a whole logUp identity with nothing but 32-byte values downloaded."""
import ctypes as C
import random

import numpy as np
import pytest

import lookup_util as L
import scalar_ops_util as S

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
MAIN = ["bls12-377", "pallas"]
CURVE_ID = {"bls12-377": 0, "pallas": 1, "bls12-381": 2, "ed-on-bls12-377": 3}
UNTOUCHED = (11, 12, 13)


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


def _W():
    s, w = C.c_uint32(0), C.c_uint32(0)
    _lib().msmz_test_lookup_geometry(C.byref(s), C.byref(w))
    assert s.value == 2
    return w.value


def _slot_of(label, n):
    return lambda v: _lib().msmz_test_lookup_slot(CURVE_ID[label], v.to_bytes(32, "little"), n)


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


def _check(curve, table, column, positions=True, t_arr=None):
    """one call on fresh uploads against the model; -> the multiplicities as ints"""
    t = t_arr if t_arr is not None else _upload(curve, table)
    f = _upload(curve, column)
    m, info = curve.Parallel.lookupMultiplicities(f, t, positions=positions)
    want_m, want_pos, want_info = L.model(table, column)
    got = curve.Scalar.toBigints(m)
    assert len(m) == len(table) and got == want_m
    if positions:
        pos = info.pop("positions")
        assert pos.dtype == np.uint32 and pos.tolist() == want_pos
    assert info == want_info
    m.free(); f.free()
    if t_arr is None:
        t.free()
    return got


# -- the C ABI, status and outputs as they are ------------------------------------------------------------------
def _c_lookup(curve, t, t_first, t_n, f, f_first, f_n, first_out=0, out=0, flags=0, positions=None, null=()):
    from msm_zprize_amd._native import MsmzLookup, MsmzLookupResult
    hd = lambda a: a if isinstance(a, int) else a.handle   # noqa: E731
    l = MsmzLookup(hd(t), t_first, t_n, hd(f), f_first, f_n,
                   None if positions is None else positions.ctypes.data_as(C.POINTER(C.c_uint32)), flags)
    h = C.c_uint64(hd(out))
    res = MsmzLookupResult(*UNTOUCHED)
    st = _lib().msmz_scalars_lookup(curve._ctx, None if "l" in null else C.byref(l), first_out, None if "h" in null else C.byref(h),
                                    None if "res" in null else C.byref(res))
    return st, h.value, (res.n_missing, res.first_missing, res.n_distinct)


# -- table_n x col_n --------------------------------------------------------------------------------------------
def _table_sizes(W):
    return [1, 2, 3, 63, 64, 65, W - 1, W, W + 1, 1000, 4097]


def _column_sizes(W):
    return [1, 63, 64, 65, W - 1, W + 1, 5000, (1 << 16) + 3]


@pytest.mark.parametrize("which", range(11), ids=["1", "2", "3", "63", "64", "65", "W-1", "W", "W+1", "1000", "4097"])
@pytest.mark.parametrize("label", MAIN)
def test_grid(curves, label, which):
    """a table of distinct random values at every table size x every column size; the columns draw from the table, every
    other one with two entries that are in no table (the lowest is reported), positions asked for every other time"""
    curve, q = curves(label), S.order(label)
    W = _W()
    n = _table_sizes(W)[which]
    rng = random.Random(1000 * which + S.ALL.index(label))
    table = L.distinct(n, q, rng)
    t = _upload(curve, table)
    for k, cn in enumerate(_column_sizes(W)):
        column = [rng.choice(table) for _ in range(cn)]
        if k % 2 and cn >= 3:
            column[cn // 3], column[cn - 1] = L.distinct(2, q, rng, avoid=table)
        _check(curve, table, column, positions=k % 3 != 0, t_arr=t)
    t.free()


@pytest.mark.parametrize("label", ["bls12-381", "ed-on-bls12-377"])
def test_other_curves(curves, label):
    curve, q = curves(label), S.order(label)
    rng = random.Random(31 + S.ALL.index(label))
    W = _W()
    table = L.tables(W + 1, q, rng)["thrice"]
    _check(curve, table, L.columns(5000, table, q, rng, W)["missing_two"])
    _check(curve, [0, q - 1, 1, 0], [q - 1, 0, 0, 2, 1])


# -- the tables -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 65, "W+1", 1000, "small+1"])
@pytest.mark.parametrize("label", MAIN)
def test_table_kinds(curves, label, n):
    """random distinct; 0 .. n - 1; all entries equal (every thread of the insert races for one slot: m_0 = col_n, the
    rest 0); every value twice; each value three times at scattered indices; 0, 1 and q - 1 as keys; keys that all start
    at one slot, and at the last slot (built with msmz_test_lookup_slot; up to W + 1 entries) -- under a uniform
    column, a column of runs and one with misses; the last size is the first that k_lookup_count takes"""
    curve, q = curves(label), S.order(label)
    W = _W()
    n = W + 1 if n == "W+1" else _small()[0] + 1 if n == "small+1" else n
    rng = random.Random(7 * n + S.ALL.index(label))
    cn = 2 * W + 9
    for name, table in L.tables(n, q, rng, _slot_of(label, n) if n <= W + 1 else None).items():
        cols = L.columns(cn, table, q, rng, W)
        for cname in ("uniform", "runs", "missing_two"):
            got = _check(curve, table, cols[cname], positions=cname != "runs")
            if name == "all_equal" and cname == "uniform":
                assert got == [cn] + [0] * (n - 1)


@pytest.mark.parametrize("label", MAIN)
def test_every_insert_races_for_one_slot(curves, label):
    """2^16 + 3 equal entries, 257 workgroups of the insert on one slot: the index ends with entry 0"""
    curve, q = curves(label), S.order(label)
    n, cn = (1 << 16) + 3, 777
    v = q - 1
    t = curve.Parallel.scalarPowers(1, n)
    curve.Parallel.combineScalars(v, t, out=t)                  # n copies of q - 1
    f = _upload(curve, [v] * cn)
    m, info = curve.Parallel.lookupMultiplicities(f, t, positions=True)
    assert curve.Scalar.toBigints(m, 0, 3) == [cn, 0, 0] and curve.Parallel.innerProduct(m) == cn
    assert info["positions"].tolist() == [0] * cn and (info["missing"], info["firstMissing"], info["distinct"]) == (0, None, 1)
    for a in (m, f, t):
        a.free()


# -- the columns ------------------------------------------------------------------------------------------------
def _small():
    p, g = C.c_uint32(0), C.c_uint32(0)
    return _lib().msmz_test_lookup_small_table(C.byref(p), C.byref(g)), p.value, g.value


@pytest.mark.parametrize("cn", ["W+1", 5000, (1 << 16) + 3])
@pytest.mark.parametrize("kernel", ["small", "large"])
@pytest.mark.parametrize("label", MAIN)
def test_column_kinds(curves, label, kernel, cn):
    """uniform over the table; constant; one value in 63 of every 64 lanes; runs of equal values crossing wave and
    workgroup edges; all missing; exactly one missing at index 0, at the last index, at a wave edge (first_missing is the
    lowest); two missing -- over a table of 300 entries (k_lookup_count_small: the counts in LDS, a workgroup loops) and
    over one just too long for that (k_lookup_count: the heads of a workgroup's waves merged)"""
    curve, q = curves(label), S.order(label)
    W = _W()
    cn = W + 1 if cn == "W+1" else cn
    rng = random.Random(cn + S.ALL.index(label))
    table = L.tables(300 if kernel == "small" else _small()[0] + 300, q, rng)["thrice"]
    t = _upload(curve, table)
    for k, (name, column) in enumerate(L.columns(cn, table, q, rng, W).items()):
        _check(curve, table, column, positions=k % 2 == 0, t_arr=t)
    t.free()


@pytest.mark.parametrize("label", MAIN)
def test_both_sides_of_the_small_table_threshold(curves, label):
    """the largest table that k_lookup_count_small takes and the smallest that k_lookup_count takes, under the same
    columns"""
    curve, q = curves(label), S.order(label)
    W = _W()
    small = _small()[0]
    rng = random.Random(61 + S.ALL.index(label))
    for n in (small - 1, small, small + 1):
        table = L.tables(n, q, rng)["thrice"]
        t = _upload(curve, table)
        cols = L.columns(2 * W + 9, table, q, rng, W)
        for k, name in enumerate(("uniform", "constant", "mostly_one", "runs", "missing_two", "all_missing")):
            _check(curve, table, cols[name], positions=k % 2 == 0, t_arr=t)
        t.free()


@pytest.mark.parametrize("label", MAIN)
def test_small_table_kernel_at_its_most_workgroups(curves, label):
    """a column long enough that k_lookup_count_small launches its most workgroups and each loops for more than its
    least passes, made on the device: column i = w^i for a 256th root of unity w, the table w^0 .. w^255, so entry j is
    hit by every i = j mod 256; then the same column against a table that lacks w^255"""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    W = _W()
    small, passes, groups = _small()
    n = W * passes * groups + 300
    w = par.rootOfUnity(8)
    f, t = par.scalarPowers(w, n), par.scalarPowers(w, 256)
    m, info = par.lookupMultiplicities(f, t, positions=True)
    assert curve.Scalar.toBigints(m) == [(n - j + 255) // 256 for j in range(256)]
    assert (info["missing"], info["firstMissing"], info["distinct"]) == (0, None, 256)
    assert (info["positions"] == (np.arange(n, dtype=np.uint64) % 256).astype(np.uint32)).all()
    m.free()
    m, info = par.lookupMultiplicities(f, t, tableN=255)
    assert curve.Scalar.toBigints(m) == [(n - j + 255) // 256 for j in range(255)]
    assert (info["missing"], info["firstMissing"], info["distinct"]) == ((n - 255 + 255) // 256, 255, 255)
    for a in (m, f, t):
        a.free()


def test_without_positions_nothing_is_written(curves):
    """the caller's buffer belongs to the call only if the descriptor names it"""
    curve, q = curves("pallas"), S.order("pallas")
    rng = random.Random(5)
    table = L.distinct(100, q, rng)
    column = L.columns(700, table, q, rng)["missing_two"]
    t, f = _upload(curve, table), _upload(curve, column)
    guard = np.full(700 + 16, 0xabababab, dtype=np.uint32)
    st, h, res = _c_lookup(curve, t, 0, 100, f, 0, 700)
    assert st == 0 and (guard == 0xabababab).all()
    _lib().msmz_free(curve._ctx, h)
    pos = guard[8:708]
    st, h, res = _c_lookup(curve, t, 0, 100, f, 0, 700, positions=pos)
    want_m, want_pos, info = L.model(table, column)
    assert st == 0 and pos.tolist() == want_pos and (guard[:8] == 0xabababab).all() and (guard[708:] == 0xabababab).all()
    assert res == (info["missing"], info["firstMissing"], info["distinct"])
    _lib().msmz_free(curve._ctx, h)
    st, h, res = _c_lookup(curve, t, 0, 100, f, 0, 700, null=("res",))      # the result record is optional
    assert st == 0 and res == UNTOUCHED
    _lib().msmz_free(curve._ctx, h)
    t.free(); f.free()


# -- the output rules -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_output_into_a_range_and_overlaps(curves, label):
    """a new handle; a range of another set and of the inputs' own set apart from both ranges, the guard entries on both
    sides unchanged; every overlap with the table range and with the column range, the exact ranges included, is
    MSMZ_ERR_ARG with nothing written; table and column may overlap each other"""
    from msm_zprize_amd.parallel import DeviceArray
    curve, q = curves(label), S.order(label)
    rng = random.Random(23)
    vals = L.distinct(40, q, rng)
    big = [rng.choice(vals) for _ in range(400)]
    t_first, t_n, f_first, f_n = 100, 48, 200, 90
    table, column = big[t_first:t_first + t_n], big[f_first:f_first + f_n]
    want = L.model(table, column)[0]
    arr, other = _upload(curve, big), _upload(curve, big)
    st, h, res = _c_lookup(curve, arr, t_first, t_n, arr, f_first, f_n)                  # a new handle
    assert st == 0 and h not in (0, arr.handle, other.handle)
    new = DeviceArray(curve, h, t_n, "scalars")
    assert curve.Scalar.toBigints(new) == want
    new.free()
    m, _ = curve.Parallel.lookupMultiplicities(arr, arr, firstColumn=f_first, N=f_n, firstTable=t_first, tableN=t_n, out=other, firstOut=7)
    assert m is other and curve.Scalar.toBigints(other) == big[:7] + want + big[7 + t_n:]
    for first_out in (0, t_first - t_n, t_first + t_n, f_first - t_n, f_first + f_n, 400 - t_n):    # the same set, apart from both
        assert _c_lookup(curve, arr, t_first, t_n, arr, f_first, f_n, first_out, arr)[:2] == (0, arr.handle)
        assert curve.Scalar.toBigints(arr) == big[:first_out] + want + big[first_out + t_n:]
        arr.free()
        arr = _upload(curve, big)
    clash = [t_first, t_first - t_n + 1, t_first + t_n - 1, t_first + 3, t_first - 1,            # the table range
             f_first, f_first - t_n + 1, f_first + f_n - 1, f_first + 20, f_first - 1]              # the column range
    for first_out in clash:
        assert _c_lookup(curve, arr, t_first, t_n, arr, f_first, f_n, first_out, arr) == (MSMZ_ERR_ARG, arr.handle, UNTOUCHED)
        with pytest.raises(ValueError):
            curve.Parallel.lookupMultiplicities(arr, arr, firstColumn=f_first, N=f_n, firstTable=t_first, tableN=t_n, out=arr, firstOut=first_out)
    # the table in one set, the column in another: each refuses only its own range
    assert _c_lookup(curve, arr, t_first, t_n, other, f_first, f_n, t_first, arr)[0] == MSMZ_ERR_ARG
    assert _c_lookup(curve, arr, t_first, t_n, other, 300, f_n, 300 + f_n - 1, other)[0] == MSMZ_ERR_ARG
    assert _c_lookup(curve, other, 0, t_n, arr, 0, t_n, 0, arr)[0] == MSMZ_ERR_ARG                   # exactly the column
    assert curve.Scalar.toBigints(arr) == big
    st, h, _ = _c_lookup(curve, arr, t_first, t_n, other, 300, f_n, f_first, arr)           # arr's old column range is free
    assert (st, h) == (0, arr.handle)
    arr.free()
    arr = _upload(curve, big)
    # table and column overlapping each other: the same range, and a partial overlap
    for (tf, tn, ff, fn) in ((50, 60, 50, 60), (50, 60, 80, 100), (80, 100, 50, 60)):
        m, info = curve.Parallel.lookupMultiplicities(arr, arr, firstColumn=ff, N=fn, firstTable=tf, tableN=tn, positions=True)
        wm, wp, wi = L.model(big[tf:tf + tn], big[ff:ff + fn])
        assert curve.Scalar.toBigints(m) == wm and info["positions"].tolist() == wp and info["missing"] == wi["missing"]
        m.free()
    arr.free(); other.free()


# -- MSMZ_ERR_RANGE ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_entries_not_below_q(curves, label):
    """an entry >= q at the first, a middle and the last index of the table range, and of the column range:
    MSMZ_ERR_RANGE, *out_handle, *res and positions as they were and no handle made (the ids show it), the context
    usable; the same entries just outside the ranges on either side are not read"""
    from msm_zprize_amd.parallel import DeviceArray
    curve, q = curves(label), S.order(label)
    W = _W()
    rng = random.Random(25)
    t_first, t_n, f_first, f_n = 5, W + 9, 3, 2 * W + 5
    table = L.distinct(t_n + 10, q, rng)
    column = [rng.choice(table[t_first:t_first + t_n]) for _ in range(f_n + 6)]
    want = L.model(table[t_first:t_first + t_n], column[f_first:f_first + f_n])
    plan = [("t", t_first, MSMZ_ERR_RANGE), ("t", t_first + t_n // 2, MSMZ_ERR_RANGE), ("t", t_first + t_n - 1, MSMZ_ERR_RANGE),
            ("t", t_first - 1, 0), ("t", t_first + t_n, 0),
            ("f", f_first, MSMZ_ERR_RANGE), ("f", f_first + f_n // 2, MSMZ_ERR_RANGE), ("f", f_first + f_n - 1, MSMZ_ERR_RANGE),
            ("f", f_first - 1, 0), ("f", f_first + f_n, 0)]
    for k, (which, index, status) in enumerate(plan):
        t, f = _upload(curve, table), _upload(curve, column)
        _plant(curve, t if which == "t" else f, index, q if k % 2 else (1 << 256) - 1)
        pos = np.full(f_n, 0xabababab, dtype=np.uint32)
        st, h, res = _c_lookup(curve, t, t_first, t_n, f, f_first, f_n, positions=pos)
        assert st == status, (which, index)
        if status:
            assert h == 0 and res == UNTOUCHED and (pos == 0xabababab).all()
            probe = curve.Parallel.randomScalars(1, 1)          # no handle leaked: the next id follows f's
            assert probe.handle == f.handle + 1
            probe.free()
            # into an existing set: the handle stays, the context goes on
            dst = _upload(curve, [1] * t_n)
            assert _c_lookup(curve, t, t_first, t_n, f, f_first, f_n, 0, dst)[:2] == (MSMZ_ERR_RANGE, dst.handle)
            dst.free()
        else:
            assert h == f.handle + 1 and pos.tolist() == want[1]
            assert res == (want[2]["missing"], (1 << 64) - 1, want[2]["distinct"])
            y = DeviceArray(curve, h, t_n, "scalars")
            assert curve.Scalar.toBigints(y) == want[0]
            y.free()
        t.free(); f.free()
    _check(curve, table, column)


# -- MSMZ_ERR_ARG -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_argument_errors(curves, label):
    """every argument error, the outputs untouched; a point set and a matrix where a scalar set is wanted"""
    curve = curves(label)
    sc = curve.Parallel.randomScalars(16, 2)
    big = curve.Parallel.randomScalars(64, 3)
    pts = curve.Parallel.randomPointsFast(16, 2)
    mat = curve.Parallel.sparseMatrix([0, 1], [1, 0], shape=(2, 2))
    ok = dict(t=sc, t_first=0, t_n=16, f=big, f_first=0, f_n=64)
    bad = [dict(ok, null=("l",)), dict(ok, null=("h",)), dict(ok, t_n=0), dict(ok, f_n=0), dict(ok, t_n=(1 << 30) + 1),
           dict(ok, f_n=1 << 32), dict(ok, f_n=(1 << 64) - 1), dict(ok, flags=1), dict(ok, flags=0x80000000),
           dict(ok, t=999), dict(ok, t=0), dict(ok, f=999), dict(ok, f=0), dict(ok, t=pts), dict(ok, f=pts), dict(ok, t=mat),
           dict(ok, f=mat), dict(ok, t_n=17), dict(ok, t_first=1), dict(ok, t_first=(1 << 64) - 1, t_n=2), dict(ok, f_n=65),
           dict(ok, f_first=60, f_n=5), dict(ok, f_first=(1 << 64) - 8, f_n=16), dict(ok, first_out=1),
           dict(ok, out=999), dict(ok, out=pts), dict(ok, out=mat), dict(ok, t_n=8, f=sc, f_first=8, f_n=8, out=big, first_out=57),
           dict(ok, out=sc), dict(ok, out=big), dict(ok, t_n=4, out=sc, first_out=3), dict(ok, t_n=4, out=big, first_out=60)]
    for kw in bad:
        out = kw.get("out", 0)
        st, h, res = _c_lookup(curve, **kw)
        assert (st, h, res) == (MSMZ_ERR_ARG, out if isinstance(out, int) else out.handle, UNTOUCHED), kw
    assert _lib().msmz_scalars_lookup(None, None, 0, None, None) == MSMZ_ERR_ARG
    st, h, res = _c_lookup(curve, sc, 12, 4, big, 60, 4, 12, big)      # the last four of each, next to each other
    assert (st, h) == (0, big.handle) and res[0] + sum(curve.Scalar.toBigints(big, 12, 4)) == 4
    # the Python checks refuse before the library is asked
    for call in (lambda: curve.Parallel.lookupMultiplicities(pts, sc), lambda: curve.Parallel.lookupMultiplicities(big, mat),
                 lambda: curve.Parallel.lookupMultiplicities(big, sc, out=pts)):
        with pytest.raises(TypeError):
            call()
    for kw in (dict(N=65), dict(tableN=0), dict(firstOut=1), dict(out=sc), dict(positions=True, firstTable=16)):
        with pytest.raises(ValueError):
            curve.Parallel.lookupMultiplicities(big, sc, **kw)
    for a in (sc, big, pts, mat):
        a.free()


# -- engines ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_two_engines_on_one_gpu(mod, curves, label):
    """two contexts of one engine each on the same GPU, their calls interleaved: each gives the bytes it gives alone"""
    curve, q = curves(label), S.order(label)
    other = _create(mod, label)
    try:
        rng = random.Random(41)
        W = _W()
        cases = []
        for n, cn in ((3, 65), (W + 1, 5000), (1000, 3 * W)):
            table = L.tables(n, q, rng)["thrice" if n >= 3 else "distinct"]
            cases.append((table, L.columns(cn, table, q, rng, W)["missing_two"]))
        alone = []
        for table, column in cases:
            t, f = _upload(curve, table), _upload(curve, column)
            m, info = curve.Parallel.lookupMultiplicities(f, t, positions=True)
            alone.append((curve.Scalar.toBigints(m), info["positions"].tobytes(), info["missing"], info["firstMissing"],
                          info["distinct"]))
            assert curve.Scalar.toBigints(m) == L.model(table, column)[0]
            for a in (t, f, m):
                a.free()
        held = []
        for k in range(len(cases)):                      # context A runs case k, context B case k + 1, turn by turn
            for ctx, (table, column) in ((curve, cases[k]), (other, cases[(k + 1) % len(cases)])):
                held.append((ctx, _upload(ctx, table), _upload(ctx, column)))
        results = [ctx.Parallel.lookupMultiplicities(f, t, positions=True) for ctx, t, f in held]
        for j, ((ctx, t, f), (m, info)) in enumerate(zip(held, results)):
            k = (j // 2 + j % 2) % len(cases)
            got = (ctx.Scalar.toBigints(m), info["positions"].tobytes(), info["missing"], info["firstMissing"], info["distinct"])
            assert got == alone[k], (j, k)
            for a in (t, f, m):
                a.free()
    finally:
        other.close()


@pytest.mark.parametrize("label", MAIN)
def test_multi_engine_context_is_unsupported(mod, label):
    """devices = [0, 0]: a probe reads across every block of 2^16 entries -- the call answers MSMZ_ERR_UNSUPPORTED and
    leaves its outputs as they were; the older calls on the same context still work"""
    mod.startThreads(devices=[0, 0])
    multi = _create(mod, label)
    try:
        f = multi.Parallel.randomScalars(64, 3)
        pos = np.full(64, 0xabababab, dtype=np.uint32)
        assert _c_lookup(multi, f, 0, 16, f, 0, 64, positions=pos) == (MSMZ_ERR_UNSUPPORTED, 0, UNTOUCHED)
        assert (pos == 0xabababab).all()
        assert multi.Parallel.innerProduct(f) == sum(multi.Scalar.toBigints(f)) % S.order(label)
        f.free()
    finally:
        multi.close()
        mod.startThreads()


# -- scratch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_nothing_depends_on_what_scratch_held(mod, label):
    """the same calls after msmz_test_poison(ctx, 0x00) and after 0xff -- the pattern that makes an uncleared slot array
    look full, an uncleared count array huge and first_missing already set -- give the bytes of the plain run; the sizes
    go down as well as up, so a later call runs inside scratch a larger one left behind"""
    q = S.order(label)
    curve = _create(mod, label)
    try:
        rng = random.Random(43)
        W = _W()
        cases = []
        for n, cn in ((1000, 5000), (3, 65), (W + 1, W + 1), (1, 1), (4097, 700)):
            table = L.tables(n, q, rng)["thrice" if n >= 3 else "distinct"]
            cases.append((table, L.columns(cn, table, q, rng, W)["missing_two" if cn >= 3 else "uniform"]))

        def run():
            out = []
            for table, column in cases:
                t, f = _upload(curve, table), _upload(curve, column)
                m, info = curve.Parallel.lookupMultiplicities(f, t, positions=True)
                out.append((curve.Scalar.toBigints(m), info["positions"].tolist(), info["missing"], info["firstMissing"], info["distinct"]))
                for a in (t, f, m):
                    a.free()
            return out

        base = run()
        for (table, column), got in zip(cases, base):
            wm, wp, wi = L.model(table, column)
            assert got == (wm, wp, wi["missing"], wi["firstMissing"], wi["distinct"])
        for pattern in (0x00, 0xff):
            nb, by = C.c_uint64(0), C.c_uint64(0)
            assert _lib().msmz_test_poison(curve._ctx, pattern, C.byref(nb), C.byref(by)) == 0
            assert nb.value >= 3 and by.value >= 4 * (L.slots(4097) + 4097)      # the index and the counts are among them
            assert run() == base, hex(pattern)
        assert _lib().msmz_test_poison(curve._ctx, -1, None, None) == 0
    finally:
        curve.close()


# -- end to end: a logUp identity -------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_logup_identity(curves, label):
    """sum_j m_j / (beta + t_j) == sum_i 1 / (beta + f_i) for a table of 300 entries with duplicates and a column of 5000
    with nothing missing, beta random, everything on the device and only 32-byte values downloaded; with one column
    entry replaced by a value outside the table (n_missing == 1) the two sides differ"""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    rng = random.Random(47 + S.ALL.index(label))
    table = L.tables(300, q, rng)["thrice"]
    assert len(set(table)) < 300
    column = [rng.choice(table) for _ in range(5000)]
    beta = rng.randrange(1, q)
    while any((beta + v) % q == 0 for v in table):
        beta = rng.randrange(1, q)
    t = _upload(curve, table)

    def sides(col):
        f = _upload(curve, col)
        m, info = par.lookupMultiplicities(f, t)
        ones_t, ones_f = par.scalarPowers(1, len(table), 1), par.scalarPowers(1, len(col), 1)
        dt = par.combineScalars(1, t, beta, ones_t)              # beta + t_j
        df = par.combineScalars(1, f, beta, ones_f)              # beta + f_i
        (it, zt), (jf, zf) = par.invertScalars(dt), par.invertScalars(df)
        assert zt == zf == 0
        left, right = par.innerProduct(m, it), par.innerProduct(jf)
        for a in (f, m, ones_t, ones_f, dt, df, it, jf):
            a.free()
        return left, right, info

    left, right, info = sides(column)
    assert info == {"missing": 0, "firstMissing": None, "distinct": len(set(table))}
    assert left == right == sum(pow(beta + v, -1, q) for v in column) % q
    outside = L.distinct(1, q, rng, avoid=table + [(-beta) % q])[0]
    column[1234] = outside
    left, right, info = sides(column)
    assert (info["missing"], info["firstMissing"]) == (1, 1234)
    assert left != right and (right - left) % q == pow(beta + outside, -1, q)
    t.free()
