"""Gate expressions on the GPU (k_scalars_expr, csrc/expr_kernels.h) through the C ABI and the Python method, bit for bit
against Python integers (tests/expr_util.py: lists mod q with cyclic rotation), the statuses of both compared.  Sizes
come from msmz_test_expr_geometry: the smallest sets (where every rotation wraps), around a wave and a workgroup, and a
few workgroups plus a partial wave; every rotation class at each of them; the limits of the description; every form of
the output; agreement with combineScalars and innerProduct; three protocol steps of a PLONK-ish prover with nothing but
the checked values downloaded; every error; a multi-engine context."""
import ctypes as C
import random

import pytest

import expr_util as E
import scalar_ops_util as S

pytestmark = pytest.mark.gpu

MSMZ_OK, MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 0, 1, 4, 6
MAIN = ["bls12-377", "pallas"]
PROTOCOL = "bls12-377"


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
    """(output entries of one workgroup, the largest operand count of the register-resident kernel or 0)"""
    w, s = C.c_uint32(0), C.c_uint32(0)
    _lib().msmz_test_expr_geometry(C.byref(w), C.byref(s))
    assert w.value % 64 == 0 and w.value >= 64 and s.value in (0, 2, 4, 8)
    return w.value, s.value


def _sizes():
    W, _ = _geometry()
    return [1, 2, 3, 63, 64, 65, W - 1, W, W + 1, 3 * W + 70]


SIZE_IDS = ["1", "2", "3", "63", "64", "65", "W-1", "W", "W+1", "3W+70"]


def _upload(curve, vals):
    return curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))


def _download(curve, arr, first=0, count=None):
    return curve.Scalar.toBigints(arr, first, count)


def _plant(curve, arr, index, value):
    """make `value` (>= q) entry `index` of a resident set: msmz_import_scalars_into converts before it reports, so after
    its MSMZ_ERR_RANGE the refused value is what the handle holds (the idiom of tests/test_mle_gpu.py)"""
    from msm_zprize_amd._native import MsmzSrc
    raw = S.encode([value])
    src = MsmzSrc(C.cast(C.c_char_p(raw), C.c_void_p), 0, 32, 0, None, None)
    assert _lib().msmz_import_scalars_into(curve._ctx, arr.handle, index, C.byref(src), 1) == MSMZ_ERR_RANGE
    assert _download(curve, arr, index, 1) == [value]


# -- the C ABI, status and handle as they are -------------------------------------------------------------------
def _c_expr(curve, columns, terms, n, first_out=0, out=0, flags=0, reserved=0, null=(), n_columns=None, n_terms=None,
            n_factors=None):
    """columns: [(array or handle, first)]; terms as everywhere; -> (status, *out_handle afterwards).  null: any of
    "e", "h", "columns", "terms", "factors" passes that pointer as NULL; n_columns / n_terms / n_factors override the
    counts the lists give (n_factors: of the first term)"""
    from msm_zprize_amd import _native as N
    hd = lambda a: a if isinstance(a, int) else a.handle   # noqa: E731
    cols = (N.MsmzExprColumn * max(1, len(columns)))(*[N.MsmzExprColumn(hd(a), f) for a, f in columns])
    keep, trms = [], (N.MsmzExprTerm * max(1, len(terms)))()
    for k, (c, fs) in enumerate(terms):
        fs = [E.factor(f) for f in fs]
        fa = (N.MsmzExprFactor * max(1, len(fs)))(*[N.MsmzExprFactor(col & 0xffffffff, rot) for col, rot in fs])
        raw = None if c is None else c.to_bytes(32, "little")
        keep += [fa, raw]
        nf = n_factors if (k == 0 and n_factors is not None) else len(fs)
        trms[k] = N.MsmzExprTerm(raw, None if "factors" in null or not fs else fa, nf, reserved if k == len(terms) - 1 else 0)
    e = N.MsmzExpr(None if "columns" in null else cols, len(columns) if n_columns is None else n_columns,
                   len(terms) if n_terms is None else n_terms, None if "terms" in null else trms, n, flags)
    h = C.c_uint64(hd(out))
    st = _lib().msmz_scalars_expr(curve._ctx, None if "e" in null else C.byref(e), first_out, None if "h" in null else C.byref(h))
    return st, h.value


def _free_handle(curve, h):
    assert _lib().msmz_free(curve._ctx, h) == 0


def _both(curve, q, columns, terms, n, arrays=None):
    """the expression over host `columns` (lists of ints) through the Python method and through the C ABI, each into a new
    handle: both MSMZ_OK, both the model's values; -> those values"""
    arrs = arrays if arrays is not None else [_upload(curve, col) for col in columns]
    want = E.model(columns, terms, n, q)
    out = curve.Parallel.evaluateExpression(arrs, terms, N=n)
    assert len(out) == n and _download(curve, out) == want
    out.free()
    st, h = _c_expr(curve, [(a, 0) for a in arrs], terms, n)
    assert st == MSMZ_OK and h != 0
    from msm_zprize_amd.parallel import DeviceArray
    got = DeviceArray(curve, h, n, "scalars")
    assert _download(curve, got) == want
    got.free()
    if arrays is None:
        for a in arrs:
            a.free()
    return want


# -- sizes x rotations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(10), ids=SIZE_IDS)
@pytest.mark.parametrize("label", MAIN)
def test_every_rotation_at_every_size(curves, label, which):
    """n in {1, 2, 3, 63, 64, 65, W - 1, W, W + 1, 3 W + 70} x rot in {0, 1, -1, n - 1, n, -n, n + 1, 2^31 - 1, -2^31}: a
    product of a rotated and an unrotated column plus a rotated column alone; then the same column at three rotations in
    one term"""
    curve, q = curves(label), S.order(label)
    n = _sizes()[which]
    rng = random.Random(100 * which + MAIN.index(label))
    cols = E.edge_columns(2, n, q, rng)
    arrs = [_upload(curve, c) for c in cols]
    c0 = rng.randrange(q)
    for rot in E.rotations(n):
        _both(curve, q, cols, [(c0, [(0, rot), 1]), (None, [(1, rot)])], n, arrays=arrs)
    _both(curve, q, cols, [(c0, [(0, 1), (0, -1), (0, 2), 1]), (q - 1, [(0, E.INT32_MIN), (0, E.INT32_MAX), (0, 0)])], n, arrays=arrs)
    for a in arrs:
        a.free()


# -- the limits of a description --------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_every_term_set(curves, label):
    """16 columns, 32 terms, degree 8, a^8, degrees 0 .. 8 mixed, constants only, 1 to 32 operands -- every set of
    expr_util at one workgroup + 1 entries; the operand counts include register_slots, register_slots + 1 and 32, the
    edges between the two kernels when the register-resident one is built"""
    curve, q = curves(label), S.order(label)
    W, slots = _geometry()
    n = W + 1
    rng = random.Random(7 + MAIN.index(label))
    sets = E.term_sets(q, n, seed=11)
    counts = {len(E.operands(terms, n)) for _, terms in sets.values()}
    assert {2, 3, 4, 5, 8, 9, 32} <= counts and (slots == 0 or {slots, slots + 1} <= counts)
    assert max(nc for nc, _ in sets.values()) == E.MAX_COLUMNS and max(len(t) for _, t in sets.values()) == E.MAX_TERMS
    pool = E.edge_columns(E.MAX_COLUMNS, n, q, rng)
    arrs = [_upload(curve, c) for c in pool]
    for name, (nc, terms) in sets.items():
        _both(curve, q, pool[:nc], terms, n, arrays=arrs[:nc])
    for a in arrs:
        a.free()


@pytest.mark.parametrize("label", MAIN)
def test_both_kernels_give_the_same_bytes(curves, label):
    """one expression of 1, 2, 4 and 8 operands as it is, and again with a term of coefficient 0 that names further
    operands until there are 9: the second form is past every register-resident instance and takes k_scalars_expr, the
    first takes the register-resident kernel where its operand count allows.  Equal bytes, the model's"""
    curve, q = curves(label), S.order(label)
    W, slots = _geometry()
    n = 2 * W + 5
    rng = random.Random(17 + MAIN.index(label))
    cols = E.edge_columns(3, n, q, rng)
    arrs = [_upload(curve, c) for c in cols]
    for n_ops in (1, 2, 4, 8):
        ops = [(k % 2, k // 2) for k in range(n_ops)]
        terms = [(rng.randrange(q), ops), (rng.randrange(q), [ops[0]] * 5), (rng.randrange(q), [])]
        pad = [(0, [(2, k) for k in range(9 - n_ops)])]
        assert len(E.operands(terms, n)) == n_ops and len(E.operands(terms + pad, n)) == 9 > max(slots, 8)
        assert _both(curve, q, cols, terms, n, arrays=arrs) == _both(curve, q, cols, terms + pad, n, arrays=arrs)
    for a in arrs:
        a.free()


@pytest.mark.parametrize("label", MAIN)
def test_an_unnamed_column_is_not_read(curves, label):
    """a constants-only expression next to a column that holds a value >= q, and a gate next to one: MSMZ_OK"""
    curve, q = curves(label), S.order(label)
    n = 70
    good, bad = _upload(curve, list(range(n))), _upload(curve, [5] * n)
    _plant(curve, bad, 3, q)
    consts = [(7, []), (None, []), (q - 1, [])]
    out = curve.Parallel.evaluateExpression([bad], consts)
    assert _download(curve, out) == [7] * n
    st, h = _c_expr(curve, [(bad, 0), (good, 0)], [(2, [1, (1, 1)])], n)
    assert st == MSMZ_OK
    from msm_zprize_amd.parallel import DeviceArray
    assert _download(curve, DeviceArray(curve, h, n, "scalars")) == [2 * i * ((i + 1) % n) % q for i in range(n)]
    assert _c_expr(curve, [(bad, 0), (good, 0)], [(2, [1, 0])], n) == (MSMZ_ERR_RANGE, 0)
    _free_handle(curve, h)
    for a in (good, bad, out):
        a.free()


# -- output forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_output_forms(curves, label):
    """a sub-range of a larger handle whose neighbours keep their bytes; in place over a column read at rotation 0;
    columns that share a handle and overlap each other"""
    curve, q = curves(label), S.order(label)
    W, _ = _geometry()
    n = W + 9
    rng = random.Random(23 + MAIN.index(label))
    big = [rng.randrange(q) for _ in range(3 * n)]
    xs = [rng.randrange(q) for _ in range(n)]
    x = _upload(curve, xs)
    # into [n - 4, 2 n - 4) of a larger set, from another handle
    o = _upload(curve, big)
    terms = [(3, [0, (0, 1)]), (None, [(0, -2)])]
    assert curve.Parallel.evaluateExpression([x], terms, out=o, firstOut=n - 4) is o
    want = E.model([xs], terms, n, q)
    assert _download(curve, o) == big[:n - 4] + want + big[2 * n - 4:]
    # in place over a column of the same handle that is read at rotation 0 (and at a multiple of n), next to a rotated
    # column of ANOTHER range of that handle that lies apart
    o2 = _upload(curve, big)
    terms = [(5, [0, (0, n), (1, 1)]), (q - 2, [(0, -n)])]
    st, h = _c_expr(curve, [(o2, n), (o2, 0)], terms, n, first_out=n, out=o2)
    assert (st, h) == (MSMZ_OK, o2.handle)
    want = E.model([big[n:2 * n], big[:n]], terms, n, q)
    assert _download(curve, o2) == big[:n] + want + big[2 * n:]
    # two columns of one handle that overlap each other, into a new handle
    terms = [(None, [0, 1]), (7, [(1, 3)])]
    out = curve.Parallel.evaluateExpression([(o, 0), (o, 5)], terms, N=n)
    now = _download(curve, o)
    assert _download(curve, out) == E.model([now[:n], now[5:5 + n]], terms, n, q)
    for a in (x, o, o2, out):
        a.free()


@pytest.mark.parametrize("label", MAIN)
def test_accumulation_in_place(curves, label):
    """out = y out + gate over three gates, each call in place with the term (y, [out]) next to the gate's: the model's
    sum gate_0 y^2 + gate_1 y + gate_2"""
    curve, q = curves(label), S.order(label)
    n = 300
    rng = random.Random(29 + MAIN.index(label))
    cols = E.edge_columns(8, n, q, rng)
    arrs = [_upload(curve, c) for c in cols]
    y = rng.randrange(q)
    gates = [E.plonk_gate(), E.permutation_wire(rng.randrange(q), rng.randrange(q), q), E.sbox_gate(rng.randrange(q), q)]
    acc = _upload(curve, [0] * n)
    want = [0] * n
    for g in gates:
        nc = 1 + max(E.factor(f)[0] for _, fs in g for f in fs)
        assert curve.Parallel.evaluateExpression(arrs[:nc] + [acc], g + [(y, [nc])], out=acc) is acc
        gv = E.model(cols, g, n, q)
        want = [(y * w + v) % q for w, v in zip(want, gv)]
        assert _download(curve, acc) == want
    for a in arrs + [acc]:
        a.free()


# -- agreement with the older calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_agrees_with_combine_and_inner_product(curves, label):
    """c_x x + c_y y == combineScalars byte for byte; the sum of x o y == innerProduct(x, y)"""
    curve, q = curves(label), S.order(label)
    n = 1000
    xs, ys = S.build_vectors(label, n, 77)
    x, y = _upload(curve, xs), _upload(curve, ys)
    rng = random.Random(31)
    cx, cy = rng.randrange(q), rng.randrange(q)
    a = curve.Parallel.combineScalars(cx, x, cy, y)
    b = curve.Parallel.evaluateExpression([x, y], [(cx, [0]), (cy, [1])])
    assert _raw(curve, a) == _raw(curve, b) and len(_raw(curve, b)) == 32 * n
    prod = curve.Parallel.evaluateExpression([x, y], [(None, [0, 1])])
    assert curve.Parallel.innerProduct(prod) == curve.Parallel.innerProduct(x, y) == sum(u * v for u, v in zip(xs, ys)) % q
    for arr in (x, y, a, b, prod):
        arr.free()


def _raw(curve, arr):
    buf = C.create_string_buffer(32 * len(arr))
    assert _lib().msmz_download_scalars(curve._ctx, arr.handle, 0, len(arr), buf) == 0
    return buf.raw


# -- protocol steps ---------------------------------------------------------------------------------------------
def _satisfied_gate(q, n, rng):
    """selectors and a witness with q_L a + q_R b + q_M a b + q_O c + q_C == 0 in every row (q_O = -1)"""
    qL, qR, qM, qC, a, b = ([rng.randrange(q) for _ in range(n)] for _ in range(6))
    qO = [q - 1] * n
    c = [(qL[i] * a[i] + qR[i] * b[i] + qM[i] * a[i] * b[i] + qC[i]) % q for i in range(n)]
    return [qL, qR, qO, qM, qC, a, b, c]


def test_protocol_arithmetic_gate(curves):
    """a satisfied PLONK arithmetic gate over 2^6 rows gives the all-zero vector; one corrupted witness entry gives
    exactly one non-zero entry, in its row"""
    curve, q = curves(PROTOCOL), S.order(PROTOCOL)
    n = 1 << 6
    rng = random.Random(41)
    cols = _satisfied_gate(q, n, rng)
    arrs = [_upload(curve, c) for c in cols]
    out = curve.Parallel.evaluateExpression(arrs, E.plonk_gate())
    assert _download(curve, out) == [0] * n
    row = 37
    cols[6][row] = (cols[6][row] + 1) % q            # b in one row
    bad_b = _upload(curve, cols[6])
    out2 = curve.Parallel.evaluateExpression(arrs[:6] + [bad_b, arrs[7]], E.plonk_gate())
    got = _download(curve, out2)
    assert [i for i, v in enumerate(got) if v] == [row] and got == E.model(cols, E.plonk_gate(), n, q)
    for a in arrs + [out, out2, bad_b]:
        a.free()


def test_protocol_permutation_check(curves):
    """the grand-product column Z of a valid copy permutation comes from scalarRecurrence (exclusive) on the device, and
    Z[i + 1] den_i - Z[i] num_i is zero in every row INCLUDING the wrap row, because the full product is 1"""
    curve, q = curves(PROTOCOL), S.order(PROTOCOL)
    par = curve.Parallel
    n = 1 << 6
    rng = random.Random(43)
    perm = list(range(n))
    rng.shuffle(perm)
    w = [0] * n
    seen = [False] * n
    for s in range(n):                                # the witness is constant on every cycle: the copies hold
        v = rng.randrange(q)
        while not seen[s]:
            seen[s], w[s] = True, v
            s = perm[s]
    ident = [i + 1 for i in range(n)]
    sigma = [ident[perm[i]] for i in range(n)]
    beta, gamma = rng.randrange(q), rng.randrange(q)
    W_, ID, SG = _upload(curve, w), _upload(curve, ident), _upload(curve, sigma)
    num = par.evaluateExpression([W_, ID], [(None, [0]), (beta, [1]), (gamma, [])])
    den = par.evaluateExpression([W_, SG], [(None, [0]), (beta, [1]), (gamma, [])])
    den_inv, zeros = par.invertScalars(den)
    assert zeros == 0
    ratio = par.evaluateExpression([num, den_inv], [(None, [0, 1])])
    Z, full = par.scalarRecurrence(ratio, None, exclusive=True)
    assert full == 1
    check = par.evaluateExpression([Z, den, num], [(None, [(0, 1), 1]), (q - 1, [0, 2])])
    assert _download(curve, check) == [0] * n
    z = _download(curve, Z)
    assert z[0] == 1 and z[1] == (w[0] + beta * ident[0] + gamma) * pow(w[0] + beta * sigma[0] + gamma, -1, q) % q
    for a in (W_, ID, SG, num, den, den_inv, ratio, Z, check):
        a.free()


def test_protocol_quotient(curves):
    """n = 2^4 rows, a gate with a next-row term; the columns go to a coset of size 4 n (coset NTTs), the gate is
    evaluated there with every rotation x 4 and multiplied by the inverted vanishing values, and the inverse coset NTT
    of the result is the quotient: zero coefficients from 3 n upwards, and quotient(z) Z_H(z) == gate(z) at a random z"""
    curve, q = curves(PROTOCOL), S.order(PROTOCOL)
    par = curve.Parallel
    lg = 4
    n, m = 1 << lg, 4 << lg
    rng = random.Random(47)
    w4 = par.rootOfUnity(lg + 2)
    w = pow(w4, 4, q)
    g = rng.randrange(2, q)
    # q_L a + q_R b + q_M a b + q_S a(wX) + q_C - c == 0 on H
    qL, qR, qM, qS, qC, a, b = ([rng.randrange(q) for _ in range(n)] for _ in range(7))
    c = [(qL[i] * a[i] + qR[i] * b[i] + qM[i] * a[i] * b[i] + qS[i] * a[(i + 1) % n] + qC[i]) % q for i in range(n)]
    host = [qL, qR, qM, qS, qC, a, b, c]
    gate = [(None, [0, 5]), (None, [1, 6]), (None, [2, 5, 6]), (None, [3, (5, 1)]), (None, [4]), (q - 1, [7])]
    ext = [(cf, [(col, 4 * rot) for col, rot in map(E.factor, fs)]) for cf, fs in gate]
    evals = [_upload(curve, col) for col in host]
    assert _download(curve, par.evaluateExpression(evals, gate)) == [0] * n
    coeffs = [par.ntt(e, lg, inverse=True, root=w) for e in evals]
    coset = [par.ntt(p, lg + 2, shift=g, root=w4, nIn=n) for p in coeffs]
    # Z_H(g w4^k) = g^n (w4^n)^k - 1, inverted
    pw = par.scalarPowers(pow(w4, n, q), m, base=pow(g, n, q))
    zh = par.evaluateExpression([pw], [(None, [0]), (q - 1, [])])
    zh_inv, zeros = par.invertScalars(zh)
    assert zeros == 0
    quot_evals = par.evaluateExpression(coset + [zh_inv], [(cf, fs + [(8, 0)]) for cf, fs in ext])
    quot = par.ntt(quot_evals, lg + 2, inverse=True, shift=g, root=w4)
    t = _download(curve, quot)
    assert t[3 * n:] == [0] * n and any(t[:3 * n])
    z = rng.randrange(q)
    at = lambda poly, x: sum(cf * pow(x, k, q) for k, cf in enumerate(poly)) % q   # noqa: E731
    p = [_download(curve, cf) for cf in coeffs]
    gate_z = (at(p[0], z) * at(p[5], z) + at(p[1], z) * at(p[6], z) + at(p[2], z) * at(p[5], z) * at(p[6], z)
              + at(p[3], z) * at(p[5], w * z % q) + at(p[4], z) - at(p[7], z)) % q
    assert at(t, z) * (pow(z, n, q) - 1) % q == gate_z and gate_z != 0
    for arr in evals + coeffs + coset + [pw, zh, zh_inv, quot_evals, quot]:
        arr.free()


# -- errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_bad_arguments(curves, label):
    """every MSMZ_ERR_ARG that needs a context: *out_handle is as it was, and the next call is correct"""
    curve, q = curves(label), S.order(label)
    n = 40
    xs = list(range(1, 101))
    x, y = _upload(curve, xs), _upload(curve, xs)
    pts = curve.Parallel.randomPointsFast(4)
    ok = [(None, [0])]
    rot = [(None, [(0, 1)])]
    many = [(None, [(k % 2, k // 2) for k in range(8 * t, 8 * t + 8)]) for t in range(4)]
    cases = [
        dict(columns=[(x, 0)], terms=ok, null=("e",)), dict(columns=[(x, 0)], terms=ok, null=("h",)),
        dict(columns=[(x, 0)], terms=ok, null=("columns",)), dict(columns=[(x, 0)], terms=ok, null=("terms",)),
        dict(columns=[(x, 0)], terms=ok, null=("factors",), n_factors=1),
        dict(columns=[(x, 0)], terms=ok, n_columns=0), dict(columns=[(x, 0)], terms=ok, n_columns=17),
        dict(columns=[(x, 0)], terms=ok, n_terms=0), dict(columns=[(x, 0)], terms=ok, n_terms=33),
        dict(columns=[(x, 0)], terms=[(None, [0] * 8)], n_factors=9),
        dict(columns=[(x, 0)], terms=ok, n=0), dict(columns=[(x, 0)], terms=ok, n=1 << 32),
        dict(columns=[(x, 0)], terms=[(None, [1])]), dict(columns=[(x, 0)], terms=[(None, [-1])]),
        dict(columns=[(x, 0)], terms=ok, flags=1), dict(columns=[(x, 0)], terms=ok, reserved=1),
        dict(columns=[(pts, 0)], terms=ok, n=2), dict(columns=[(987654, 0)], terms=ok), dict(columns=[(0, 0)], terms=ok),
        dict(columns=[(x, 0), (pts, 0)], terms=ok, n=2),                                   # an unnamed column is checked too
        dict(columns=[(x, 61)], terms=ok), dict(columns=[(x, 101)], terms=ok, n=1), dict(columns=[(x, 0), (y, 70)], terms=ok),
        dict(columns=[(x, (1 << 64) - 1)], terms=ok),
        dict(columns=[(x, 0)], terms=ok, first_out=1),                                      # a new handle starts at 0
        dict(columns=[(x, 0)], terms=ok, out=pts), dict(columns=[(x, 0)], terms=ok, out=424242),
        dict(columns=[(x, 0)], terms=ok, out=y, first_out=61),
        dict(columns=[(x, 10)], terms=ok, out=x, first_out=11), dict(columns=[(x, 10)], terms=ok, out=x, first_out=9),
        dict(columns=[(x, 10)], terms=ok, out=x, first_out=49), dict(columns=[(y, 0), (x, 10)], terms=[(None, [1])], out=x, first_out=40),
        dict(columns=[(x, 10)], terms=rot, out=x, first_out=10), dict(columns=[(x, 10)], terms=rot, out=x, first_out=49),
        dict(columns=[(x, 10)], terms=[(None, [0, (0, n), (0, 1 - n)])], out=x, first_out=10),
        dict(columns=[(x, 0), (y, 0)], terms=many + [(None, [(0, 16)])]),
    ]
    for kw in cases:
        kw = dict(kw)
        out = kw.pop("out", 0)
        want_h = out if isinstance(out, int) else out.handle
        st, h = _c_expr(curve, kw.pop("columns"), kw.pop("terms"), kw.pop("n", n), out=out, **kw)
        assert (st, h) == (MSMZ_ERR_ARG, want_h), kw
    # what is allowed right next to the refusals
    assert _c_expr(curve, [(x, 10)], ok, n, first_out=10, out=x) == (MSMZ_OK, x.handle)
    assert _c_expr(curve, [(x, 10)], rot, n, first_out=50, out=x) == (MSMZ_OK, x.handle)
    assert _c_expr(curve, [(y, 0), (x, 10)], [(None, [0])], n, first_out=20, out=x) == (MSMZ_OK, x.handle)   # unnamed: overlaps anything
    st, h = _c_expr(curve, [(x, 0), (y, 0)], many, n)
    assert st == MSMZ_OK
    _free_handle(curve, h)
    now = _download(curve, y)
    assert now == xs and _both(curve, q, [now[:n]], [(3, [0, (0, 1)])], n, arrays=[y]) == [3 * (i + 1) * ((i + 1) % n + 1) % q for i in range(n)]
    for a in (x, y, pts):
        a.free()


@pytest.mark.parametrize("label", MAIN)
def test_values_not_below_q(curves, label):
    """MSMZ_ERR_RANGE for a coefficient >= q (nothing is launched: it wins over a planted entry too) and for a planted
    entry at the first and at the last entry of a named column; MSMZ_OK for one planted one entry outside the range on
    either side.  After each refusal *out_handle is as it was and the next call is correct"""
    curve, q = curves(label), S.order(label)
    W, _ = _geometry()
    n = W + 3
    xs = [(7 * i + 1) % q for i in range(n + 2)]
    terms = [(3, [0, (0, 1)]), (None, [1])]
    y = _upload(curve, list(range(n)))

    def want(vals):
        return E.model([vals, list(range(n))], terms, n, q)

    for cbad in (q, q + 1, (1 << 256) - 1):
        x = _upload(curve, xs)
        assert _c_expr(curve, [(x, 1), (y, 0)], [(cbad, [0]), (None, [1])], n) == (MSMZ_ERR_RANGE, 0)
        assert _c_expr(curve, [(x, 1), (y, 0)], [(1, [0]), (cbad, [])], n, out=x, first_out=1) == (MSMZ_ERR_RANGE, x.handle)
        assert _download(curve, x) == xs                  # checked on the host: the destination was not touched
        x.free()
    for at, status in ((1, MSMZ_ERR_RANGE), (n, MSMZ_ERR_RANGE), (0, MSMZ_OK), (n + 1, MSMZ_OK)):
        x = _upload(curve, xs)
        _plant(curve, x, at, q)
        st, h = _c_expr(curve, [(x, 1), (y, 0)], terms, n)
        assert st == status and (h != 0) == (status == MSMZ_OK), at
        if status == MSMZ_OK:
            from msm_zprize_amd.parallel import DeviceArray
            assert _download(curve, DeviceArray(curve, h, n, "scalars")) == want(xs[1:n + 1])
            _free_handle(curve, h)
        else:
            with pytest.raises(Exception) as err:
                curve.Parallel.evaluateExpression([(x, 1), y], terms, N=n)
            assert getattr(err.value, "status", None) == MSMZ_ERR_RANGE
        _both(curve, q, [xs[1:n + 1], list(range(n))], terms, n)     # the context stays usable
        x.free()
    y.free()


# -- a multi-engine context -------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", MAIN)
def test_multi_engine_context(mod, label):
    """devices = [0, 0]: an unrotated expression is element-wise and correct across both engines, into a new handle and
    over a whole existing one; any rotation and any non-zero first is MSMZ_ERR_UNSUPPORTED, with the handle as it was"""
    q = S.order(label)
    mod.startThreads(devices=[0, 0])
    multi = _create(mod, label)
    try:
        n = (1 << 16) + 300                      # the second block of 2^16 entries lives on the second engine
        x, y = multi.Parallel.randomScalars(n, 3), multi.Parallel.randomScalars(n, 4)
        xs, ys = multi.Scalar.toBigints(x), multi.Scalar.toBigints(y)
        c = 0x1234567
        terms = [(c, [0, 1, 1]), (None, [0]), (5, []), (2, [(0, n), (1, -n)])]
        want = E.model([xs, ys], terms, n, q)
        out = multi.Parallel.evaluateExpression([x, y], terms)
        assert multi.Scalar.toBigints(out) == want
        assert multi.Parallel.evaluateExpression([x, y, out], terms + [(3, [2])], out=out) is out     # in place, whole
        assert multi.Scalar.toBigints(out) == [(v + 3 * v) % q for v in want]
        for kw in (dict(columns=[(x, 0), (y, 0)], terms=[(None, [(0, 1)])], n=n), dict(columns=[(x, 1)], terms=[(None, [0])], n=n - 1),
                   dict(columns=[(x, 0), (y, 1)], terms=[(None, [0])], n=n - 1),          # an unnamed column's first counts too
                   dict(columns=[(x, 0)], terms=[(None, [0])], n=n - 1, out=out, first_out=1),
                   dict(columns=[(x, 0)], terms=[(None, [0])], n=n - 1, out=out)):         # an existing handle in part
            o = kw.pop("out", 0)
            st, h = _c_expr(multi, kw.pop("columns"), kw.pop("terms"), kw.pop("n"), out=o, **kw)
            assert (st, h) == (MSMZ_ERR_UNSUPPORTED, o if isinstance(o, int) else o.handle), kw
        assert _c_expr(multi, [(x, 0)], [(None, [1])], n) == (MSMZ_ERR_ARG, 0)
        assert _c_expr(multi, [(x, 0)], [(q, [0])], n) == (MSMZ_ERR_RANGE, 0)
        assert multi.Parallel.innerProduct(x) == sum(xs) % q
        for a in (x, y, out):
            a.free()
    finally:
        multi.close()
        mod.startThreads()
