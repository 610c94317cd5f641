"""Number-theoretic transforms over resident scalar sets on the GPU (k_ntt_pass, csrc/ntt_kernels.h): downloads against
a transform over Python integers, bit-exact, at every size up to two stages past the one-pass limit; above that against
the calls that were there before (innerProduct of the input with scalarPowers of g w^k, the transform of a unit vector,
the round trip) at the smallest full two-pass size and the smallest three-pass size; cosets, short inputs, batches,
ranges and in-place destinations, two uses (a polynomial product, a commitment from evaluations), the errors, and a
two-engine context; more vectors than a launch has rows of workgroups, so that a workgroup's loop over its vectors goes
round again; more (log_n, root) keys than the twiddle cache keeps.  Sizes come from msmz_test_ntt_plan,
msmz_test_ntt_geometry and msmz_test_cache_geometry."""
import ctypes as C
import random

import pytest

import check_points_util as CP
import ntt_util as N
import scalar_ops_util as S
from oracle import params as P

pytestmark = pytest.mark.gpu

MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6
INVERSE, COSET = N.INVERSE, N.COSET
MARK = (1 << 200) + 0xA5A5


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


def _handle(v):
    return 0 if v is None else (v if isinstance(v, int) else v.handle)


def _le(v):
    return None if v is None else int(v).to_bytes(32, "little")


def _ntt(curve, x, log_n, flags=0, n_in=0, count=1, first=0, first_out=0, out=0, root=None, shift=None):
    """msmz_scalars_ntt through the C ABI -> (status, *out_handle afterwards)"""
    from msm_zprize_amd._native import MsmzNtt
    t = MsmzNtt(_handle(x), first, log_n, flags, n_in, count, _le(root), _le(shift))
    h = C.c_uint64(_handle(out))
    st = _lib().msmz_scalars_ntt(curve._ctx, C.byref(t), first_out, C.byref(h))
    return st, h.value


def _upload(curve, vals):
    return curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))


def _raw(curve, arr, first, n):
    buf = C.create_string_buffer(32 * n)
    assert _lib().msmz_download_scalars(curve._ctx, _handle(arr), first, n, buf) == 0
    return buf.raw


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set, as tests/test_scalar_scan_gpu.py does"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert curve.Scalar.toBigints(arr, index, 1) == [value]


def _plan(label, log_n):
    st, stages = N.plan(_lib(), N.curve_id(label), log_n)
    assert st == 0 and sum(stages) == log_n
    return stages


def _sizes():
    """(the one-pass limit, the smallest size of two full passes, the smallest three-pass size), as log_n on BLS12-377"""
    limit = N.pass_log(_lib())
    assert len(_plan("bls12-377", limit)) == 1 and len(_plan("bls12-377", limit + 1)) == 2
    three = next(k for k in range(limit + 1, 32) if len(_plan("bls12-377", k)) == 3)
    assert three <= 22
    return limit, three - 1, three


# ---------------------------------------------------------------------------------------------- against Python integers
def _full_comparison(curves, label, log_ns):
    curve, q = curves(label), S.order(label)
    for log_n in log_ns:
        n = 1 << log_n
        w = N.root(label, log_n)
        assert curve.Parallel.rootOfUnity(log_n) == w
        xs = N.inputs(label, n, 100 * log_n + S.ALL.index(label))
        x = _upload(curve, xs)
        for inverse in (False, True):
            y = curve.Parallel.ntt(x, log_n, inverse=inverse)
            assert len(y) == n and y.kind == "scalars"
            got = curve.Scalar.toBigints(y)
            want = N.transform(q, xs, n, w, inverse)
            bad = [(i, hex(g), hex(v)) for i, (g, v) in enumerate(zip(got, want)) if g != v]
            assert not bad, (label, log_n, inverse, _plan(label, log_n), bad[:3])
            back = curve.Parallel.ntt(y, log_n, inverse=not inverse)
            assert _raw(curve, back, 0, n) == S.encode(xs), (label, log_n, inverse)
            y.free(); back.free()
        x.free()


def test_every_size_through_the_first_two_pass_plans(curves):
    """BLS12-377, log_n = 0, 1, 2, ..., pass limit + 2 (a partial tile, exactly one tile, the first two-pass plans):
    forward and inverse, every entry against the Python-integer transform, and the round trip byte for byte; the inputs
    hold 0, 1, q - 1 and the value with full low words"""
    limit = _sizes()[0]
    _full_comparison(curves, "bls12-377", range(0, limit + 3))


@pytest.mark.parametrize("label", ["pallas", "bls12-381"])
def test_tile_edge_and_first_two_pass_size_other_fields(curves, label):
    limit = _sizes()[0]
    _full_comparison(curves, label, [limit, limit + 1])


def test_twisted_edwards_field_has_two_transforms(curves):
    """ed-on-bls12-377: q - 1 = 2 * odd.  log_n 0 and 1 are right, 2 is MSMZ_ERR_UNSUPPORTED by rule"""
    label = "ed-on-bls12-377"
    curve, q = curves(label), S.order(label)
    assert N.two_adicity(label) == 1
    _full_comparison(curves, label, [0, 1])
    assert curve.Parallel.rootOfUnity(1) == q - 1
    x = _upload(curve, [3, 4, 5, 6])
    assert _ntt(curve, x, 2) == (MSMZ_ERR_UNSUPPORTED, 0)
    assert _ntt(curve, x, 40) == (MSMZ_ERR_UNSUPPORTED, 0)
    buf = C.create_string_buffer(32)
    assert _lib().msmz_scalars_root_of_unity(N.curve_id(label), 2, buf) == MSMZ_ERR_UNSUPPORTED
    assert N.plan(_lib(), N.curve_id(label), 2)[0] == MSMZ_ERR_UNSUPPORTED
    x.free()


# ---------------------------------------------------------------------------------------------- against the merged calls
def _indices(label, log_n, seed):
    """32 output indices: 0, 1, n / 2, n - 1, both sides of every boundary between the digits of the plan's passes and of
    the tile, the rest random"""
    n = 1 << log_n
    ks = [0, 1, n // 2, n - 1]
    edges, done = [1 << N.pass_log(_lib())], 0
    for s in _plan(label, log_n)[:-1]:
        done += s
        edges += [1 << done, n >> done]
    for e in edges:
        ks += [e - 1, e, n - e - 1, n - e]
    ks = [k for k in dict.fromkeys(ks) if 0 <= k < n][:32]
    rng = random.Random(seed)
    while len(ks) < 32:
        k = rng.randrange(n)
        if k not in ks:
            ks.append(k)
    return ks


def _check_entries(curve, q, x, n_in, y, n, base, w, ks, what):
    """y_k == <x, powers of base w^k> for k in ks, with innerProduct and scalarPowers as the oracle"""
    par = curve.Parallel
    got = S.decode(_raw(curve, y, 0, n))
    for k in ks:
        pw = par.scalarPowers(base * pow(w, k, q) % q, n_in)
        want = par.innerProduct(x, pw, n_in)
        pw.free()
        assert got[k] == want, (what, k)


@pytest.mark.parametrize("which", ["two-pass", "three-pass"])
@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_large_sizes_against_inner_products(curves, label, which):
    """the smallest size at which two passes are both full, and the smallest three-pass size: 32 output entries against
    innerProduct(x, scalarPowers(w^k)), the transform of a unit vector against scalarPowers(w^j), the round trip, the
    same on a coset, and n_in = n / 4 against the zero-padded vector"""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    _, two, three = _sizes()
    log_n = two if which == "two-pass" else three
    assert len(_plan(label, log_n)) == (2 if which == "two-pass" else 3)
    n = 1 << log_n
    w = N.root(label, log_n)
    ks = _indices(label, log_n, log_n)
    x = par.randomScalars(n, 1000 + log_n)
    y = par.ntt(x, log_n)
    _check_entries(curve, q, x, n, y, n, 1, w, ks, "forward")
    back = par.ntt(y, log_n, inverse=True)
    assert _raw(curve, back, 0, n) == _raw(curve, x, 0, n)
    y.free(); back.free()
    # a unit vector: column j of the transform
    for j in (1, ks[-1]):
        e = _upload(curve, [0] * j + [1])
        col = par.ntt(e, log_n, nIn=j + 1)
        pw = par.scalarPowers(pow(w, j, q), n)
        assert _raw(curve, col, 0, n) == _raw(curve, pw, 0, n), j
        e.free(); col.free(); pw.free()
    # a coset
    g = random.Random(log_n).randrange(2, q)
    y = par.ntt(x, log_n, shift=g)
    _check_entries(curve, q, x, n, y, n, g, w, ks, "coset")
    back = par.ntt(y, log_n, inverse=True, shift=g)
    assert _raw(curve, back, 0, n) == _raw(curve, x, 0, n)
    y.free(); back.free()
    # a short input equals the zero-padded one
    raw = _raw(curve, x, 0, n // 4)
    padded = par.scalarsFromBytes(raw + bytes(32 * (n - n // 4)), n)
    a, b = par.ntt(x, log_n, nIn=n // 4, shift=g), par.ntt(padded, log_n, shift=g)
    assert _raw(curve, a, 0, n) == _raw(curve, b, 0, n)
    _check_entries(curve, q, x, n // 4, a, n, g, w, ks, "short input")
    for arr in (a, b, padded, x):
        arr.free()


# ---------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("count", [3, 64])
def test_batch_equals_one_at_a_time(curves, count):
    """count transforms of 2^(limit + 2) entries in one call == the same transforms one by one, forward with a coset and
    inverse; with n_in < n the input vectors are n_in apart and the output vectors n"""
    label = "bls12-377"
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    log_n = _sizes()[0] + 2
    n = 1 << log_n
    x = par.randomScalars(count * n, 7 + count)
    g = 5
    def one_by_one(n_in, **kw):
        raw = b""
        for k in range(count):
            one = par.ntt(x, log_n, nIn=n_in, first=k * n_in, **kw)
            raw += _raw(curve, one, 0, n)
            one.free()
        return raw

    for kw in (dict(shift=g), dict(inverse=True), dict(inverse=True, shift=g)):
        y = par.ntt(x, log_n, count=count, **kw)
        assert len(y) == count * n
        assert _raw(curve, y, 0, count * n) == one_by_one(n, **kw), kw   # every vector of the batch
        y.free()
    n_in = n // 2 + 3
    y = par.ntt(x, log_n, nIn=n_in, count=count)
    assert _raw(curve, y, 0, count * n) == one_by_one(n_in)
    y.free(); x.free()


def _cache_geometry():
    """(twiddle sets an engine keeps, fixed-base tables it keeps, vectors that get a workgroup row of their own)"""
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _lib().msmz_test_cache_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _assert_vectors(got, want, n, what):
    """two downloads of whole vectors of n entries: equal, or the first vectors that differ"""
    if got != want:
        assert len(got) == len(want), what
        bad = [v for v in range(len(want) // (32 * n)) if got[32 * n * v:32 * n * (v + 1)] != want[32 * n * v:32 * n * (v + 1)]]
        raise AssertionError((what, "vectors that differ", len(bad), bad[:4], bad[-2:]))


@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_more_vectors_than_workgroup_rows(curves, label):
    """count = ntt_grid_vectors + 2 transforms of 8 entries (n_in = 5): k_ntt_pass launches ntt_grid_vectors rows of
    workgroups, and the rows of vectors 0 and 1 go round their loop a second time, for vectors ntt_grid_vectors and
    ntt_grid_vectors + 1 -- the only place where the barrier behind the store, the error flag carried from one trip to the
    next and the two strides of a second trip (in_stride = 5, out_stride = 8) are exercised.

    Forward on a coset into a new handle, every entry against the Python-integer transform (vector v is m_v times one of
    four base vectors, so its transform is m_v times that vector's); the inverse on the coset back to the zero-padded
    inputs; a plain transform in place with n_in = n; log_n = 0, where a vector is one entry and a pass has no stage.  One
    entry >= q in the first vector of a second trip (and, apart from it, in vector 1: a first trip with a clean second one
    behind it) is MSMZ_ERR_RANGE and leaves no handle; the source set ends in such an entry one past the addressed
    range throughout, which is never read.

    A plan of two passes at this count would need more than 2^27 entries and as much again in scratch: it is left out.
    The loop over the vectors is the same code in every pass."""
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    G = _cache_geometry()[2]
    count, log_n, n, n_in, g = G + 2, 3, 8, 5, 7
    assert count * n == 524296 and G + 1 < count
    w = N.root(label, log_n)
    rng = random.Random(G + S.ALL.index(label))
    base = [N.inputs(label, n_in, 3)] + [[rng.randrange(q) for _ in range(n_in)] for _ in range(3)]
    mult = [1, 1, 1, 1] + [rng.randrange(1, q) for _ in range(count - 4)]
    mult[G], mult[G + 1] = q - 1, 2   # (vector G = - vector 3, vector G + 1 = twice vector 0: neither equals a first trip's)
    xs = [m * b % q for v, m in enumerate(mult) for b in base[v % 4]]
    x = _upload(curve, xs + [0])
    _plant(curve, x, count * n_in, q)   # one past the addressed range, for every call below

    def scaled(vectors):
        return S.encode([m * t % q for v, m in enumerate(mult) for t in vectors[v % 4]])
    raw_in = S.encode(xs)
    # forward on a coset, n_in < n
    y = par.ntt(x, log_n, shift=g, nIn=n_in, count=count)
    assert len(y) == count * n
    _assert_vectors(_raw(curve, y, 0, count * n), scaled([N.transform(q, b, n, w, False, g) for b in base]), n, "forward")
    # the inverse back: the zero-padded inputs
    padded = b"".join(raw_in[32 * n_in * v:32 * n_in * (v + 1)] + bytes(32 * (n - n_in)) for v in range(count))
    back = par.ntt(y, log_n, inverse=True, shift=g, count=count)
    _assert_vectors(_raw(curve, back, 0, count * n), padded, n, "inverse")
    y.free()
    # plain, in place, n_in = n
    assert par.ntt(back, log_n, count=count, out=back) is back
    _assert_vectors(_raw(curve, back, 0, count * n), scaled([N.transform(q, b, n, w) for b in base]), n, "in place")
    back.free()
    # one entry per vector, no stage
    for inverse in (False, True):
        one = par.ntt(x, 0, count=count, inverse=inverse)
        _assert_vectors(_raw(curve, one, 0, count), raw_in[:32 * count], 1, ("log_n = 0", inverse))
        one.free()
    # an entry >= q in a second trip, and in a first trip that a clean second trip follows
    for vector in (G, 1):
        bad = _upload(curve, xs)
        _plant(curve, bad, vector * n_in + 2, q + vector)
        for flags, shift, cnt in ((COSET, g, count), (0, None, G + 1)):
            assert _ntt(curve, bad, log_n, flags, n_in, cnt, shift=shift) == (MSMZ_ERR_RANGE, 0), (vector, flags, cnt)
        _good_call_is_correct(curve, label)
        bad.free()
    # the call after it, over the same rows
    y = par.ntt(x, log_n, shift=g, nIn=n_in, count=count)
    _assert_vectors(_raw(curve, y, 0, count * n), scaled([N.transform(q, b, n, w, False, g) for b in base]), n, "afterwards")
    y.free(); x.free()


# ---------------------------------------------------------------------------------------------- the twiddle cache
def _ntt_built(curve):
    b = C.c_uint64(1 << 40)
    assert _lib().msmz_test_ntt_tables(curve._ctx, C.byref(b)) == 0
    return b.value


@pytest.mark.parametrize("armed", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("ends", ["one-pass", "two-pass"])
def test_twiddle_cache_evicts_the_oldest(mod, ends, armed):
    """ntt_sets + 1 keys on a context of its own, each transform against the Python-integer one and each building one
    set; the first key again is built again (its set left when the last one came) and is right; the keys used last are
    served from the cache; the second key, which left when the first came back, is built again: first in, first out.  An
    inverse transform of a cached size builds one more set (the inverse root is another key), a custom root equal to
    the default one builds none.  `two-pass`: the first and the last key are the two smallest sizes of two passes, so
    that the set which leaves, and the one built in its place, are large ones.  `poisoned`: the same with
    msmz_test_poison armed at 0xa5, so that a set freed and handed out again, or read before it is filled, shows"""
    from test_scratch_poison_gpu import fresh, poison
    label = "bls12-377"
    q = S.order(label)
    sets = _cache_geometry()[0]
    limit = _sizes()[0]
    keys = list(range(1, sets + 2))
    if ends == "two-pass":
        keys[0], keys[-1] = limit + 1, limit + 2
    assert len(set(keys)) == sets + 1 and max(keys) <= N.two_adicity(label)
    with fresh(mod, label) as curve:
        if armed:
            poison(curve, 0xa5)
        par = curve.Parallel

        def run(log_n, builds, what, inverse=False, root=None):
            n = 1 << log_n
            xs = N.inputs(label, n, 300 + log_n)
            x = _upload(curve, xs)
            before = _ntt_built(curve)
            y = par.ntt(x, log_n, inverse=inverse, root=root)
            assert _ntt_built(curve) - before == builds, (what, log_n, "built")
            want = N.transform(q, xs, n, N.root(label, log_n), inverse)
            assert _raw(curve, y, 0, n) == S.encode(want), (what, log_n)
            x.free(); y.free()

        assert _ntt_built(curve) == 0
        for k in keys:
            run(k, 1, "fill")
        run(keys[0], 1, "the oldest has left")          # keys[1] leaves
        run(keys[0], 0, "the most recent")
        run(keys[-1], 0, "the one before it")
        run(keys[1], 1, "first in, first out")          # keys[2] leaves
        run(keys[-1], 1, "the inverse root is another key", inverse=True)   # keys[3] leaves
        run(keys[-1], 0, "the inverse root, cached", inverse=True)
        run(keys[-1], 0, "the default root, given", root=N.root(label, keys[-1]))
        run(keys[0], 0, "still cached")
        assert _ntt_built(curve) == sets + 4


# ---------------------------------------------------------------------------------------------- ranges
@pytest.mark.parametrize("log_n", ["limit", "limit + 1"])
def test_ranges_and_in_place(curves, log_n):
    """in place over a middle range of a larger set whose neighbours hold a marker and are found intact (a one-pass and
    a two-pass plan); a destination in another handle at an offset; a partial overlap is MSMZ_ERR_ARG and writes nothing"""
    label = "bls12-377"
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    log_n = _sizes()[0] + (0 if log_n == "limit" else 1)
    n = 1 << log_n
    w = N.root(label, log_n)
    lead, tail = 37, 29
    xs = N.inputs(label, 2 * n, 3)
    vals = [MARK] * lead + xs + [MARK + 1] * tail
    v = _upload(curve, vals)
    want = N.transform(q, xs[:n], n, w) + N.transform(q, xs[n:], n, w)
    assert par.ntt(v, log_n, count=2, first=lead, out=v, firstOut=lead) is v
    assert curve.Scalar.toBigints(v) == [MARK] * lead + want + [MARK + 1] * tail
    assert par.ntt(v, log_n, inverse=True, count=2, first=lead, out=v, firstOut=lead) is v
    assert curve.Scalar.toBigints(v) == vals
    # another handle at an offset; the same handle, apart
    o = _upload(curve, [MARK] * (n + 20))
    par.ntt(v, log_n, first=lead + n, out=o, firstOut=11)
    assert curve.Scalar.toBigints(o) == [MARK] * 11 + want[n:] + [MARK] * 9
    par.ntt(v, log_n, first=lead, out=v, firstOut=lead + n)
    assert curve.Scalar.toBigints(v) == [MARK] * lead + xs[:n] + want[:n] + [MARK + 1] * tail
    before = _raw(curve, v, 0, len(vals))
    for first, first_out, n_in in ((lead, lead + 1, 0), (lead + 1, lead, 0), (lead, lead + n - 1, 0), (lead + n - 1, lead, 0),
                                   (lead, lead, n // 2), (lead + 5, lead, n // 2), (lead, lead + n // 2 - 1, n // 2)):
        assert _ntt(curve, v, log_n, 0, n_in, 1, first, first_out, v) == (MSMZ_ERR_ARG, v.handle), (first, first_out, n_in)
    assert _raw(curve, v, 0, len(vals)) == before
    # a short input next to its destination in one handle: apart is allowed
    st, h = _ntt(curve, v, log_n, 0, n // 2, 1, lead, lead + n // 2, v)
    assert (st, h) == (0, v.handle)
    assert curve.Scalar.toBigints(v, lead + n // 2, n) == N.transform(q, xs[:n // 2], n, w)
    v.free(); o.free()


# ---------------------------------------------------------------------------------------------- uses
def test_polynomial_product(curves):
    """two polynomials of degree 63 through forward transforms of length 128, a pointwise product (combineScalars with a
    resident coefficient) and the inverse transform == the schoolbook product"""
    label = "bls12-381"
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    rng = random.Random(64)
    a = [rng.randrange(q) for _ in range(64)]
    b = [rng.randrange(q) for _ in range(64)]
    a[63], b[63], a[0] = q - 1, q - 1, 0
    ab = _upload(curve, a + b)
    ev = par.ntt(ab, 7, nIn=64, count=2)
    prod = par.combineScalars(ev, ev, N=128, firstA=0, firstX=128)
    c = par.ntt(prod, 7, inverse=True)
    want = [0] * 128
    for i, u in enumerate(a):
        for j, v in enumerate(b):
            want[i + j] = (want[i + j] + u * v) % q
    assert curve.Scalar.toBigints(c) == want
    for arr in (ab, ev, prod, c):
        arr.free()


def test_commitment_from_evaluations(curves):
    """msm(inverse_ntt(evaluations), SRS) == msm(coefficients, SRS): a column that arrives in evaluation form is
    committed without leaving the device"""
    label = "bls12-377"
    curve, params, q = curves(label), P.CURVES[label], S.order(label)
    par = curve.Parallel
    log_n = _sizes()[0] + 1
    n = 1 << log_n
    srs = par.randomPointsFast(n, 9)
    coeffs = par.randomScalars(n, 10)
    evals = par.ntt(coeffs, log_n)
    assert _raw(curve, evals, 0, n) != _raw(curve, coeffs, 0, n)
    back = par.ntt(evals, log_n, inverse=True)
    c1, c2 = par.msm(back, srs, n)["result"], par.msm(coeffs, srs, n)["result"]
    assert c1 == c2 and not c1["isZero"]
    for arr in (srs, coeffs, evals, back):
        arr.free()


# ---------------------------------------------------------------------------------------------- roots
def test_custom_root(curves):
    """root = the inverse of the default root: the output is the default output with its indices mirrored (k -> n - k);
    roots that are not primitive n-th roots of unity are MSMZ_ERR_ARG, a root >= q MSMZ_ERR_RANGE"""
    label = "pallas"
    curve, q = curves(label), S.order(label)
    par = curve.Parallel
    log_n = _sizes()[0] + 1
    n = 1 << log_n
    w = N.root(label, log_n)
    x = par.randomScalars(n, 21)
    y = S.decode(_raw(curve, par.ntt(x, log_n), 0, n))
    z = S.decode(_raw(curve, par.ntt(x, log_n, root=pow(w, -1, q)), 0, n))
    assert z == [y[(n - k) % n] for k in range(n)]
    z = S.decode(_raw(curve, par.ntt(x, log_n, root=pow(w, 3, q)), 0, n))
    assert z == [y[3 * k % n] for k in range(n)]
    for bad in (1, 0, w * w % q, N.root(label, log_n + 1), 5, q - 1):
        assert _ntt(curve, x, log_n, root=bad) == (MSMZ_ERR_ARG, 0), bad
    for bad in (q, (1 << 256) - 1):
        assert _ntt(curve, x, log_n, root=bad) == (MSMZ_ERR_RANGE, 0)
    one = _upload(curve, [7])
    assert _ntt(curve, one, 0, root=q - 1) == (MSMZ_ERR_ARG, 0)
    st, h = _ntt(curve, one, 0, root=1)
    assert st == 0 and _raw(curve, h, 0, 1) == S.encode([7])
    x.free(); one.free()


# ---------------------------------------------------------------------------------------------- errors
def _good_call_is_correct(curve, label):
    q = S.order(label)
    xs = N.inputs(label, 64, 5)
    x = _upload(curve, xs)
    y = curve.Parallel.ntt(x, 6)
    assert curve.Scalar.toBigints(y) == N.transform(q, xs, 64, N.root(label, 6))
    x.free(); y.free()


def test_resident_entry_out_of_range(curves):
    """ONE entry >= q at the first, a middle and the last index of the source of a one-pass and of a two-pass transform:
    MSMZ_ERR_RANGE, no handle, a following good call is correct; the same entry outside the addressed range (before it,
    behind it, and behind n_in inside a vector) is not read"""
    label = "bls12-377"
    curve, q = curves(label), S.order(label)
    limit = _sizes()[0]
    for log_n in (limit, limit + 1):
        n = 1 << log_n
        xs = N.inputs(label, n + 2, log_n)
        for index, value in ((1, q), (n // 2 + 1, (1 << 256) - 1), (n, q + 1)):
            bad = _upload(curve, xs)
            _plant(curve, bad, index, value)
            for flags, shift in ((0, None), (INVERSE, None), (COSET, 3), (INVERSE | COSET, 3)):
                assert _ntt(curve, bad, log_n, flags, 0, 1, 1, shift=shift) == (MSMZ_ERR_RANGE, 0), (log_n, index, flags)
            _good_call_is_correct(curve, label)
            bad.free()
        w = N.root(label, log_n)
        for index, first, n_in in ((0, 1, n), (n + 1, 1, n), (n // 2 + 1, 1, n // 2)):
            bad = _upload(curve, xs)
            _plant(curve, bad, index, q)
            st, h = _ntt(curve, bad, log_n, 0, n_in, 1, first)
            assert st == 0 and h != 0, (log_n, index)
            assert S.decode(_raw(curve, h, 0, n)) == N.transform(q, xs[first:first + n_in], n, w), (log_n, index)
            assert _lib().msmz_free(curve._ctx, h) == 0
            bad.free()


@pytest.mark.parametrize("label", ["bls12-377", "pallas"])
def test_argument_errors(curves, label):
    """every MSMZ_ERR_ARG row of include/msmz.h, before any launch and with *out_handle untouched; shift >= q is
    MSMZ_ERR_RANGE; log_n above the 2-adicity is MSMZ_ERR_UNSUPPORTED"""
    from msm_zprize_amd._native import MsmzNtt
    curve, q = curves(label), S.order(label)
    n = 256
    sc = curve.Parallel.randomScalars(4 * n, 2)
    pts = curve.Parallel.randomPointsFast(n, 2)
    before = _raw(curve, sc, 0, 4 * n)
    lib = _lib()
    h = C.c_uint64(0)
    t = MsmzNtt(sc.handle, 0, 8, 0, 0, 1, None, None)
    assert lib.msmz_scalars_ntt(None, C.byref(t), 0, C.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_ntt(curve._ctx, None, 0, C.byref(h)) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_ntt(curve._ctx, C.byref(t), 0, None) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_root_of_unity(N.curve_id(label), 3, None) == MSMZ_ERR_ARG
    assert lib.msmz_scalars_root_of_unity(99, 3, C.create_string_buffer(32)) == MSMZ_ERR_ARG
    big = (1 << 64) - 1
    for kw in [dict(flags=4), dict(flags=1 << 31), dict(count=0), dict(log_n=31, count=2), dict(log_n=20, count=1 << 12),
               dict(n_in=n + 1), dict(n_in=big), dict(flags=INVERSE, n_in=n - 1), dict(flags=INVERSE, n_in=1),
               dict(shift=3), dict(flags=COSET), dict(flags=COSET, shift=0), dict(flags=INVERSE | COSET, shift=0),
               dict(x=0xDEAD), dict(x=pts), dict(out=0xDEAD), dict(out=pts), dict(x=0),
               dict(first=3 * n + 1), dict(first=big), dict(count=5), dict(count=4, first=1), dict(n_in=n // 2, count=9),
               dict(first_out=1), dict(out=sc, first_out=3 * n + 1), dict(out=sc, first_out=big), dict(out=sc, count=4, first_out=1)]:
        args = dict(x=sc, log_n=8, out=0)
        args.update(kw)
        x = args.pop("x")
        out = args["out"]
        assert _ntt(curve, x, **args) == (MSMZ_ERR_ARG, _handle(out)), kw
    for bad in (q, q + 1, (1 << 256) - 1):
        assert _ntt(curve, sc, 8, COSET, shift=bad) == (MSMZ_ERR_RANGE, 0)
        assert _ntt(curve, sc, 8, COSET, out=sc, shift=bad) == (MSMZ_ERR_RANGE, sc.handle)
    S_adic = N.two_adicity(label)
    assert _ntt(curve, sc, S_adic + 1) == (MSMZ_ERR_UNSUPPORTED, 0)
    assert _ntt(curve, sc, 32) == ((MSMZ_ERR_ARG if S_adic >= 32 else MSMZ_ERR_UNSUPPORTED), 0)
    assert _raw(curve, sc, 0, 4 * n) == before
    _good_call_is_correct(curve, label)
    with pytest.raises(ValueError):
        curve.Parallel.ntt(sc, 8, shift=0)
    with pytest.raises(TypeError):
        curve.Parallel.ntt(pts, 8)
    with pytest.raises(ValueError):
        curve.Parallel.ntt(sc, 8, out=sc, firstOut=1)
    sc.free(); pts.free()


def test_two_engine_context(mod, curves):
    """devices = [0, 0]: every transform is MSMZ_ERR_UNSUPPORTED (after the checks that need no handle), the helpers that
    need no context still answer"""
    label = "bls12-377"
    mod.startThreads(devices=[0, 0])
    multi = mod.Weierstrass.create(mod.curves.BY_LABEL[label])
    try:
        x = multi.Parallel.randomScalars(1 << 12, 3)
        for log_n, flags, shift in ((0, 0, None), (5, 0, None), (12, INVERSE, None), (12, COSET, 5)):
            assert _ntt(multi, x, log_n, flags, shift=shift) == (MSMZ_ERR_UNSUPPORTED, 0)
            assert _ntt(multi, x, log_n, flags, out=x, shift=shift) == (MSMZ_ERR_UNSUPPORTED, x.handle)
        assert _ntt(multi, x, 5, 8) == (MSMZ_ERR_ARG, 0)
        assert _ntt(multi, x, 5, count=0) == (MSMZ_ERR_ARG, 0)
        assert multi.Parallel.rootOfUnity(12) == N.root(label, 12)
        x.free()
    finally:
        multi.close()
        mod.startThreads()
