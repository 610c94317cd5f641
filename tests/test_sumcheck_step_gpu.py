"""msmz_scalars_sumcheck_step on the GPU (k_scalars_sumcheck_step / k_scalars_sumcheck_last, csrc/mle_kernels.h) through
the C ABI and the Python methods: byte for byte against the two-call route it replaces (mle_bind of every table, then
sumcheck_round over what that wrote) on copies of the same inputs, and against Python integers
(tests/sumcheck_step_util.py).  Sizes come from msmz_test_sumcheck_step_geometry: one thread, a partial wave, one wave,
half a tile, one tile, two and four tiles of new pair indices; no table is longer than 2^16 entries.  Then the overlap
rules, the argument and range errors, a multi-engine context, a whole protocol through sumcheckProve and scratch that
was poisoned before the call."""
import ctypes as C
import random

import pytest

import mle_util as M
import scalar_ops_util as S
import sumcheck_step_util as U

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
LOW = 1
UNTOUCHED = (99, b"\xaa" * 160)
MODEL_VARS = 8          # the integer model of the round runs up to this size; above it the two-call route is the reference
CURVES = ("bls12-377", "bls12-381")


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


def _log_tile():
    t = C.c_uint32(0)
    _lib().msmz_test_sumcheck_step_geometry(C.byref(t))
    assert t.value >= 64 and t.value & (t.value - 1) == 0
    return t.value.bit_length() - 1


def _sizes():
    """n_vars: one thread (1: the last step, 2), a partial wave (3), one full wave of 64 new pair indices (8), half a
    tile, exactly one tile, two tiles (the fold adds), four tiles"""
    lt = _log_tile()
    sizes = [1, 2, 3, 8, lt + 1, lt + 2, lt + 3, lt + 4]
    assert max(sizes) <= 16, "no table is longer than 2^16 entries"
    return sizes


def _le(v):
    return int(v).to_bytes(32, "little")


def _c_step(curve, tables, outs, n_vars, terms, r, flags=0, n_tables=None, n_terms=None, degree=True, evals=True):
    """tables / outs: [(array or raw handle, first)] (outs None: in place), terms: [(coeff or None, mask)] or None
    -> (status, *degree, the 160 bytes)"""
    from msm_zprize_amd import _native as N

    def pack(pairs):
        if pairs is None:
            return None
        return (N.MsmzSumcheckTable * max(1, len(pairs)))(*[N.MsmzSumcheckTable(a if isinstance(a, int) else a.handle, f) for a, f in pairs])

    trms = None if terms is None else (N.MsmzSumcheckTerm * max(1, len(terms)))(
        *[N.MsmzSumcheckTerm(None if c is None else _le(c), m) for c, m in terms])
    s = N.MsmzSumcheckStep(pack(tables), pack(outs), len(tables or ()) if n_tables is None else n_tables, n_vars, trms,
                           len(terms or ()) if n_terms is None else n_terms, flags, None if r is None else _le(r))
    d = C.c_uint32(99)
    ev = C.create_string_buffer(b"\xaa" * 160, 160)
    st = _lib().msmz_scalars_sumcheck_step(curve._ctx, C.byref(s), C.byref(d) if degree else None, ev if evals else None)
    return st, d.value, ev.raw


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set: msmz_import_scalars_into converts before it reports, so after
    its MSMZ_ERR_RANGE the refused value is what the handle holds (as tests/test_mle_gpu.py does)"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


_data = {}


def _source(label, v, k):
    """table k of 2^v values of a curve as (ints, bytes), made once and left unchanged: the planted rows of the scalar-set
    tests (0, 1, q - 1, the value with seven full low words, pairs summing to q) in front and at the end"""
    if (label, v, k) not in _data:
        vals = S.build_vectors(label, 1 << v, 7000 + 100 * v + k)[k % 2]
        _data[(label, v, k)] = (vals, S.encode(vals))
    return _data[(label, v, k)]


def _terms(label, nt):
    return U.mixed_terms(nt, S.order(label), random.Random(50 + nt))


def _r(label, v, nt):
    q = S.order(label)
    return (random.Random(v * 16 + nt).randrange(2, q), q - 1)[(v + nt) % 5 == 0]


_refs = {}


def _two_call(curve, label, v, nt, low):
    """the two-call route on fresh copies: bindMle per table into new arrays, sumcheckRound over them -> (bound tables as
    bytes, degree, the values as bytes); once per case, shared by the variants.  One variable: no round is left, the model
    gives the claim."""
    key = (label, v, nt, low)
    if key not in _refs:
        par, q = curve.Parallel, S.order(label)
        terms, r = _terms(label, nt), _r(label, v, nt)
        srcs = [par.scalarsFromBytes(_source(label, v, k)[1], 1 << v) for k in range(nt)]
        bound = [par.bindMle(f, r, v, low=low) for f in srcs]
        raw = [par.scalarsToBytes(b) for b in bound]
        if v > 1:
            values = par.sumcheckRound(bound, terms, v - 1, low=low)
        else:
            values = [U.claim([S.decode(b) for b in raw], terms, q)]
        if v <= MODEL_VARS:   # the reference against its own reference
            mb, md, mv = U.step([_source(label, v, k)[0] for k in range(nt)], terms, r, q, low)
            assert [S.decode(b) for b in raw] == mb and values == mv and md == len(values) - 1
        for a in srcs + bound:
            a.free()
        _refs[key] = (raw, len(values) - 1, b"".join(_le(x) for x in values))
    return _refs[key]


def _check_case(curve, label, v, nt, variant):
    """one step against the two-call route: variant "in place" (high order, out NULL), "high" and "low" (into the middle of
    other, longer arrays that held junk)"""
    par = curve.Parallel
    low = variant == "low"
    n, h = 1 << v, 1 << (v - 1)
    terms, r = _terms(label, nt), _r(label, v, nt)
    want_bound, want_degree, want_values = _two_call(curve, label, v, nt, low)
    # sources sit at offset 3 of their arrays, so a wrong `first` shows
    pad = _le(5) * 3
    srcs = [par.scalarsFromBytes(pad + _source(label, v, k)[1] + pad, n + 6) for k in range(nt)]
    outs, dsts = None, []
    if variant != "in place":
        dsts = [par.scalarsFromBytes(_le(7) * (h + 4), h + 4) for _ in range(nt)]
        outs = [(d, 2) for d in dsts]
    st, degree, ev = _c_step(curve, [(f, 3) for f in srcs], outs, v, terms, r, LOW if low else 0)
    assert (st, degree) == (0, want_degree), (label, v, nt, variant, st)
    assert ev == want_values + b"\xaa" * (160 - len(want_values)), (label, v, nt, variant)
    for k in range(nt):
        src_now = par.scalarsToBytes(srcs[k])
        if variant == "in place":
            assert src_now[:96 + 32 * h] == pad + want_bound[k], (label, v, nt, k)
            assert src_now[96 + 32 * h:] == _source(label, v, k)[1][32 * h:] + pad     # the high half and what follows stay
        else:
            assert src_now == pad + _source(label, v, k)[1] + pad                         # the sources stay
            assert par.scalarsToBytes(dsts[k]) == _le(7) * 2 + want_bound[k] + _le(7) * 2, (label, v, nt, variant, k)
    for a in srcs + dsts:
        a.free()


@pytest.mark.parametrize("variant", ("in place", "high", "low"))
@pytest.mark.parametrize("label", CURVES)
def test_step_equals_bind_then_round(curves, label, variant):
    """every size x 1, 2, 4, 6 tables (BLS12-381: the one-tile size and the last step), terms of mixed degree: degree,
    values, destinations and everything around them byte for byte those of the two-call route"""
    lt = _log_tile()
    sizes = _sizes() if label == CURVES[0] else [1, lt + 2]
    for v in sizes:
        for nt in (1, 2, 4, 6):
            _check_case(curves(label), label, v, nt, variant)


@pytest.mark.parametrize("variant", ("in place", "high", "low"))
def test_every_table_count(curves, variant):
    """1 .. 6 tables at 2^9 entries (two waves and a partial block of new pair indices)"""
    for nt in range(1, 7):
        _check_case(curves(CURVES[0]), CURVES[0], 9, nt, variant)


def test_python_method_returns_the_model(curves):
    """Parallel.sumcheckStep at a model size: (degree, ints) and the arrays written == the integer model, in place and
    into `out`, and the last step returns the claim"""
    label = CURVES[0]
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    v, nt = 6, 3
    terms, r = _terms(label, nt), _r(label, v, nt)
    data = [_source(label, v, k)[0] for k in range(nt)]
    for low in (False, True):
        bound, degree, values = U.step(data, terms, r, q, low)
        srcs = [par.scalarsFromBytes(_source(label, v, k)[1], 1 << v) for k in range(nt)]
        outs = [par.scalarsFromBytes(bytes(32 << (v - 1)), 1 << (v - 1)) for _ in range(nt)]
        assert par.sumcheckStep(srcs, terms, v, r, out=outs, low=low) == (degree, values)
        assert [curve.Scalar.toBigints(o) for o in outs] == bound
        if not low:
            assert par.sumcheckStep(srcs, terms, None, r) == (degree, values)
            assert [curve.Scalar.toBigints(f, 0, 1 << (v - 1)) for f in srcs] == bound
        for a in srcs + outs:
            a.free()
    ones = [par.scalarsFromBytes(S.encode(d[:2]), 2) for d in data]
    bound, degree, values = U.step([d[:2] for d in data], terms, r, q)
    assert par.sumcheckStep(ones, terms, 1, r) == (0, values) and degree == 0
    assert [curve.Scalar.toBigints(f, 0, 1) for f in ones] == bound
    for a in ones:
        a.free()


@pytest.mark.parametrize("low", (False, True))
def test_overlapping_sources(curves, low):
    """two tables that are the same range (a square) and a third overlapping them in part, destinations apart: the values
    of the model, on both sides of the one-tile size in turn"""
    label = CURVES[0]
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    v = 7
    vals = _source(label, v + 1, 0)[0]
    f = par.scalarsFromBytes(_source(label, v + 1, 0)[1], 1 << (v + 1))
    firsts = [0, 0, 40]
    terms = [(None, 0b011), (q - 2, 0b100), (3, 0b111)]
    r = _r(label, v, 3)
    bound, degree, values = U.step([vals[a:a + (1 << v)] for a in firsts], terms, r, q, low)
    outs = [par.scalarsFromBytes(bytes(32 << (v - 1)), 1 << (v - 1)) for _ in firsts]
    st, d, ev = _c_step(curve, [(f, a) for a in firsts], [(o, 0) for o in outs], v, terms, r, LOW if low else 0)
    assert (st, d) == (0, degree) and ev[:32 * (degree + 1)] == b"".join(_le(x) for x in values)
    assert [curve.Scalar.toBigints(o) for o in outs] == bound
    assert par.scalarsToBytes(f) == _source(label, v + 1, 0)[1]
    for a in [f] + outs:
        a.free()


def test_forbidden_overlaps_write_nothing(curves):
    """the high half, a partial overlap, in place with MSMZ_MLE_LOW (out NULL and named), a destination on another
    table's source, two destinations overlapping: MSMZ_ERR_ARG each, and no array changes"""
    label = CURVES[0]
    curve, par = curves(label), curves(label).Parallel
    v, n, h = 5, 32, 16
    raw = [_source(label, 7, k)[1] for k in range(3)]
    f, g, d = (par.scalarsFromBytes(b, 128) for b in raw)
    t1, t2 = [(None, 1)], [(None, 0b11)]
    bad = [
        ([(f, 8)], [(f, 8 + h)], 0, t1),                  # the high half
        ([(f, 8)], [(f, 9)], 0, t1), ([(f, 8)], [(f, 7)], 0, t1),       # partial overlaps with the low half
        ([(f, 8)], [(f, 8 + h - 1)], 0, t1), ([(f, 8)], [(f, 8 + n - 1)], 0, t1), ([(f, 8)], [(f, 0)], 0, t1),
        ([(f, 8)], None, LOW, t1), ([(f, 8)], [(f, 8)], LOW, t1),       # in place in the low order
        ([(f, 8)], [(f, 8 + h)], LOW, t1), ([(f, 8)], [(f, 10)], LOW, t1),
        ([(f, 0), (g, 0)], [(g, 0), (d, 0)], 0, t2), ([(f, 0), (g, 0)], [(d, 0), (f, n - 1)], 0, t2),   # another table's source
        ([(f, 0), (f, 0)], None, 0, t2), ([(f, 0), (f, 8)], None, 0, t2),   # ... in place, where the sources overlap
        ([(f, 0), (g, 0)], [(d, 0), (d, h - 1)], 0, t2), ([(f, 0), (g, 0)], [(d, 5), (d, 5)], 0, t2),   # two destinations
        ([(f, 0), (g, 0)], [(f, 0), (f, h - 1)], 0, t2),
    ]
    for tables, outs, flags, terms in bad:
        assert _c_step(curve, tables, outs, v, terms, 5, flags) == (MSMZ_ERR_ARG,) + UNTOUCHED, (tables, outs, flags)
    assert [par.scalarsToBytes(a) for a in (f, g, d)] == raw
    # the neighbours of the refused shapes that are allowed
    ok = [([(f, 8)], [(f, 8)], 0, t1), ([(f, 8)], [(f, 8 + n)], 0, t1), ([(f, 16)], [(f, 0)], LOW, t1),
          ([(f, 0), (g, 0)], [(d, 0), (d, h)], 0, t2), ([(f, 0), (f, n)], None, 0, t2)]
    for tables, outs, flags, terms in ok:
        assert _c_step(curve, tables, outs, v, terms, 5, flags)[0] == 0, (tables, outs, flags)
    for a in (f, g, d):
        a.free()


def test_argument_errors(curves):
    """every MSMZ_ERR_ARG of the header and a host value >= q (MSMZ_ERR_RANGE): the outputs and the arrays stay"""
    label = CURVES[0]
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    raw = _source(label, 6, 0)[1]
    f, d = par.scalarsFromBytes(raw, 64), par.scalarsFromBytes(raw, 64)
    pts = par.randomPointsFast(4)
    T, O, t1 = [(f, 0)], [(d, 0)], [(None, 1)]
    step = lambda *a, **k: _c_step(curve, *a, **k)
    arg = (MSMZ_ERR_ARG,) + UNTOUCHED
    assert _lib().msmz_scalars_sumcheck_step(curve._ctx, None, C.byref(C.c_uint32(0)), C.create_string_buffer(160)) == MSMZ_ERR_ARG
    assert step(None, O, 5, t1, 5, n_tables=1) == arg and step(T, O, 5, None, 5, n_terms=1) == arg      # null tables / terms
    assert step(T, O, 5, t1, None) == arg                                                               # null r
    assert step(T, O, 5, t1, 5, degree=False) == arg and step(T, O, 5, t1, 5, evals=False) == arg       # null outputs
    assert step(T, O, 0, t1, 5) == arg and step(T, O, 32, t1, 5) == arg                                 # n_vars
    assert step(T, O, 5, t1, 5, flags=2) == arg and step(T, O, 5, t1, 5, flags=3) == arg                # unknown flag bits
    assert step(T, O, 5, t1, 5, n_tables=0) == arg and step(T * 7, [(d, 0)] * 7, 1, t1, 5) == arg      # table counts
    assert step(T, O, 5, t1, 5, n_terms=0) == arg and step(T, O, 5, t1 * 9, 5) == arg                  # term counts
    for mask in (0, 2, 1 << 6):
        assert step(T, O, 5, [(None, mask)], 5) == arg
    assert step(T * 5, [(d, 2 * k) for k in range(5)], 1, [(None, 0b11111)], 5) == arg                  # five factors
    assert step([(987654, 0)], O, 5, t1, 5) == arg and step(T, [(987654, 0)], 5, t1, 5) == arg         # unknown handles
    assert step([(pts, 0)], O, 1, t1, 5) == arg and step(T, [(pts, 0)], 1, t1, 5) == arg               # not a scalar set
    assert step([(f, 33)], O, 5, t1, 5) == arg and step(T, [(d, 49)], 5, t1, 5) == arg                 # beyond the set
    assert step([(f, 1 << 63)], O, 5, t1, 5) == arg and step(T, [(d, (1 << 64) - 8)], 5, t1, 5) == arg
    assert step(T, O, 7, t1, 5) == arg and step([(f, 64)], O, 1, t1, 5) == arg
    rng_err = (MSMZ_ERR_RANGE,) + UNTOUCHED
    assert step(T, O, 5, t1, q) == rng_err and step(T, O, 5, [(q, 1)], 5) == rng_err                   # host values >= q
    assert step(T, O, 5, [(None, 1), ((1 << 256) - 1, 1)], q - 1) == rng_err
    assert step([(f, 33)], O, 5, t1, q) == arg                                                          # ARG comes first
    assert par.scalarsToBytes(f) == raw and par.scalarsToBytes(d) == raw
    with pytest.raises(ValueError):
        par.sumcheckStep([f], [(1, 1)], 5, q, out=[d])
    with pytest.raises(TypeError):
        par.sumcheckStep([pts], [(1, 1)], 1, 5)
    f.free(); d.free(); pts.free()


@pytest.mark.parametrize("low", (False, True))
def test_resident_entry_out_of_range(curves, low):
    """a record >= q just outside a source range: no error, the values of a clean run.  Inside it (the first record, one
    in the high half, the last): MSMZ_ERR_RANGE, *degree and the bytes as they were, and the context still works -- at a
    size of one tile and a bit, at the one-thread size and in the last step"""
    label = CURVES[0]
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    lt = _log_tile()
    flags = LOW if low else 0
    for v in (lt + 3, 2, 1):
        n, h = 1 << v, 1 << (v - 1)
        base = _source(label, v, 0)[1]
        terms, r = [(None, 0b11), (q - 1, 0b01)], _r(label, v, 2)
        g = par.scalarsFromBytes(_source(label, v, 1)[1], n)
        outs = [par.scalarsFromBytes(bytes(32 * h), h) for _ in range(2)]
        O = [(o, 0) for o in outs]

        def fresh(bad_at=None):
            a = par.scalarsFromBytes(_le(1) + base + _le(1), n + 2)
            if bad_at is not None:
                _plant(curve, a, bad_at, q + 3)
            return a

        clean = fresh()
        want = _c_step(curve, [(clean, 1), (g, 0)], O, v, terms, r, flags)
        assert want[0] == 0
        want_out = [par.scalarsToBytes(o) for o in outs]
        for at in (0, n + 1):                               # just outside
            a = fresh(at)
            assert _c_step(curve, [(a, 1), (g, 0)], O, v, terms, r, flags) == want
            assert [par.scalarsToBytes(o) for o in outs] == want_out
            a.free()
        for at in (1, 1 + h + (h >> 1), n):                 # inside
            a = fresh(at)
            assert _c_step(curve, [(a, 1), (g, 0)], O, v, terms, r, flags) == (MSMZ_ERR_RANGE,) + UNTOUCHED, (v, at)
            assert _c_step(curve, [(clean, 1), (g, 0)], O, v, terms, r, flags) == want          # the context stays usable
            assert [par.scalarsToBytes(o) for o in outs] == want_out
            a.free()
        for a in [clean, g] + outs:
            a.free()


def test_multi_engine_context_is_unsupported(mod):
    """devices = [0, 0]: MSMZ_ERR_UNSUPPORTED, the outputs as they were; the older calls on the same context still work"""
    label = CURVES[0]
    mod.startThreads(devices=[0, 0])
    multi = _create(mod, label)
    try:
        f = multi.Parallel.randomScalars(64, 3)
        d = multi.Parallel.randomScalars(64, 4)
        assert _c_step(multi, [(f, 0)], [(d, 0)], 2, [(None, 1)], 5) == (MSMZ_ERR_UNSUPPORTED,) + UNTOUCHED
        assert _c_step(multi, [(f, 0)], None, 1, [(None, 1)], 5) == (MSMZ_ERR_UNSUPPORTED,) + UNTOUCHED
        assert multi.Parallel.innerProduct(f) == sum(multi.Scalar.toBigints(f)) % S.order(label)
        f.free(); d.free()
    finally:
        multi.close()
        mod.startThreads()


@pytest.mark.parametrize("low", (False, True))
@pytest.mark.parametrize("label", CURVES)
def test_whole_protocol(curves, label, low):
    """sumcheckProve at v = 10 over eq A B - eq C and a table alone: every g_k(0) + g_k(1) is g_(k-1)(r_(k-1)), the first is
    the claimed sum, the final claim is the terms over the final one-entry tables (the tables at the challenges), and the
    round polynomials are those of the two-call route on copies, challenge for challenge"""
    curve, q, par = curves(label), S.order(label), curves(label).Parallel
    v, nt = 10, 4
    rng = random.Random(77 + low)
    terms = [(None, 0b0111), (q - 1, 0b1001), (rng.randrange(q), 0b0100)]
    data = [_source(label, v, k) for k in range(nt)]

    def challenge(values):
        return (int.from_bytes(b"".join(_le(x) for x in values), "little") * 0x9E3779B97F4A7C15 + 12345) % q

    tables = [par.scalarsFromBytes(raw, 1 << v) for _, raw in data]
    polys, rs, claim = par.sumcheckProve(tables, terms, v, challenge, low=low)
    for a in tables:
        a.free()
    assert len(polys) == len(rs) == v and rs == [challenge(p) for p in polys]
    total = sum(U.claim([[d[0][i]] for d in data], terms, q) for i in range(1 << v)) % q
    assert (polys[0][0] + polys[0][1]) % q == total
    for k in range(1, v):
        assert len(polys[k]) == 4 and (polys[k][0] + polys[k][1]) % q == M.interpolate(polys[k - 1], rs[k - 1], q)
    assert claim == M.interpolate(polys[-1], rs[-1], q)
    point = rs if low else rs[::-1]
    assert claim == U.claim([[M.mle_eval(d[0], point, q)] for d in data], terms, q)
    # the two-call route: sumcheckRound, then bindMle of every table, on copies
    cur = [par.scalarsFromBytes(raw, 1 << v) for _, raw in data]
    for k in range(v):
        assert par.sumcheckRound(cur, terms, v - k, low=low) == polys[k]
        nxt = [par.bindMle(f, rs[k], v - k, low=low) for f in cur]
        for a in cur:
            a.free()
        cur = nxt
    assert claim == U.claim([curve.Scalar.toBigints(f) for f in cur], terms, q)
    for a in cur:
        a.free()


def test_scratch_poisoned_before_the_call(mod):
    """one step of two tiles and a bit, and a last step, in a context whose scratch msmz_test_poison filled with 0xa5 and
    then with 0x5a: the same bytes both times, those of a context nothing poisoned"""
    label = CURVES[0]
    v, nt = _log_tile() + 3, 3
    terms, r = _terms(label, nt), _r(label, v, nt)
    runs = []
    for pattern in (None, 0xA5, 0x5A):
        curve = _create(mod, label)
        try:
            par = curve.Parallel
            if pattern is not None:
                nb, by = C.c_uint64(0), C.c_uint64(0)
                assert _lib().msmz_test_poison(curve._ctx, pattern, C.byref(nb), C.byref(by)) == 0
            srcs = [par.scalarsFromBytes(_source(label, v, k)[1], 1 << v) for k in range(nt)]
            got = [_c_step(curve, [(f, 0) for f in srcs], None, v, terms, r)]
            got.append([par.scalarsToBytes(f, 0, 1 << (v - 1)) for f in srcs])
            got.append(_c_step(curve, [(f, 6) for f in srcs], None, 1, terms, r))
            runs.append(got)
        finally:
            curve.close()
    assert runs[0][0][0] == 0 and runs[0][2][:2] == (0, 0)
    assert runs[1] == runs[0] and runs[2] == runs[0]
