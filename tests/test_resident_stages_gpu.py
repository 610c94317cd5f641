"""The family stages of the resident sets (csrc/point_ops.h, scalar_ops.h, ntt_ops.h, matrix_ops.h, lookup_ops.h) share
one core (csrc/sets_core.h): one stream, one staging buffer, one error word, and ONE pinned landing, h_res_, for every
result record -- the verdicts of a point check and the positions of a lookup ride home in it behind their records, and
the window results of an MSM land in it too.  What only that sharing can break is a call that reads what another family
left there, or that finds the landing moved: so one fresh context runs one call of every family, each held against the
CPU oracle of its own test module, and a second fresh context runs the same list backwards.

The list: a point check with verdicts whose tail forces h_res_ to grow, a plain MSM (which reads h_res_ after the
growth), a lookup with positions, an inner product, a recurrence with its last value, a transform of two passes forward
and back followed by a second recurrence (a transform reports through the error word of the meta block: it no longer
touches the recurrence's record), a fixed-base multiplication whose base is a resident record (fetched through the core,
as a download is), and a sparse matrix-vector product; then the two calls that came after the list was first written and
share sdot_ and the landing with the calls above: a gate expression with rotated columns and a sumcheck step in place.

The scalar field of ed-on-bls12-377 has two-adicity 1 (tests/test_ntt_gpu.py): no transform of more than two entries
exists there, so on that curve the transform of the list is the one of length 2, a single pass."""
import ctypes as C
import random

import pytest

import check_points_util as U
import expr_util as EX
import fixed_base_util as FB
import lookup_util as LK
import matrix_util as MX
import ntt_util as NT
import points_mul_util as M
import scalar_ops_util as S
import scalar_scan_util as SC
import sumcheck_step_util as SS
from oracle import c_oracle, prng
from oracle import params as P
from test_scratch_poison_gpu import _lib, _pt, _raw_points, _raw_scalars, _strip, _upload, fresh, scratch

pytestmark = pytest.mark.gpu

LABELS = ["pallas", "ed-on-bls12-377"]
SEED_P, SEED_S = 11, 12
# Engine::init gives h_res_ the window results of one problem: 2 * kMaxWindows * XW * 4 bytes with kMaxWindows = 128
# (csrc/plan.h) and XW = 4 NW words, NW = fe_bytes / 4 -- 32768 bytes on both curves here.  The record of a point check
# is 16 bytes and one verdict byte per point follows it: 2^16 + 3 points need 65555, so the landing has to grow.
N_CHECK = (1 << 16) + 3
N_MSM, N_COL, N_TABLE, N_VEC, N_FIXED, BASE_INDEX, N_MAT, NNZ = 1 << 10, 3000, 257, 3000, 65, 5, 64, 300
STEP_VARS = 11   # the sumcheck step: tables of 2^11 entries, the first entries of the two vectors


def _h_res_initial(params):
    return 2 * 128 * (4 * (params["fe_bytes"] // 4)) * 4


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


class Data:
    """One curve's host inputs and oracle answers, computed once and left unchanged: both orders use them."""

    def __init__(self, label):
        self.label, self.params, self.q = label, P.CURVES[label], S.order(label)
        params, q = self.params, self.q
        rng = random.Random("stages" + label)
        g = U.generator(params)
        # ---- the point check: a generated set (point i = splitmix64(seed, i) G, oracle/prng.py: on the curve and in the
        # subgroup, verdict 0) with the bad points of check_points_util.planted_set at its indices
        pts, self.where = U.planted_set(label, [{}] * N_CHECK)
        self.planted = {i: pts[i] for i in self.where}
        self.verdicts = [0] * N_CHECK
        for i, p in self.planted.items():
            self.verdicts[i] = U.verdict(params, p)
        self.check = U.summary(self.verdicts)
        assert 16 + N_CHECK > _h_res_initial(params)
        # (bad points on both sides of where the landing ended before it grew; pallas has prime order: none off-subgroup)
        assert self.check[0] > 0 and any(self.verdicts[:1024]) and any(self.verdicts[_h_res_initial(params):])
        # ---- the MSM: the closed form over the generators' multipliers
        t = prng.sum_of_products_mod(prng.scalars_np(SEED_S, N_MSM, q), prng.multipliers_np(SEED_P, N_MSM), q)
        self.msm = _pt(label, c_oracle.scale(params, t, g))
        # ---- the lookup: a table with one duplicate, a column with entries that are in no table
        self.table = LK.distinct(N_TABLE, q, rng)
        self.table[200] = self.table[3]
        strangers = LK.distinct(5, q, rng, avoid=self.table)
        self.column = [rng.choice(self.table) for _ in range(N_COL)]
        for k, i in enumerate((3, 700, 701, 2998, N_COL - 1)):   # (firstMissing = 3: a minimum that a zeroed word hides)
            self.column[i] = strangers[k]
        self.lookup = LK.model(self.table, self.column)
        # ---- inner product and recurrence
        self.xs, self.ys = S.build_vectors(label, N_VEC, 7)
        self.dot = sum(a * b for a, b in zip(self.xs, self.ys)) % q
        self.rec = SC.recurrence(q, N_VEC, self.xs, self.ys)
        self.rec2 = SC.recurrence(q, N_VEC, self.ys, self.xs)
        # ---- the transform: the smallest of two passes, where the field has one
        self.log_n = None   # (needs the library: set by the first run)
        # ---- fixed base: record BASE_INDEX of the generated set
        self.fs = FB.gpu_scalars(params, N_FIXED, 5)
        base = c_oracle.scale(params, prng.point_multiplier(SEED_P, BASE_INDEX), g)
        base = U.pt(base["x"] % params["modulus"], base["y"] % params["modulus"], False)
        self.fixed = [FB.expected(label, s, base) for s in self.fs]
        # ---- the matrix
        self.rows = [rng.randrange(N_MAT) for _ in range(NNZ)]
        self.cols = [rng.randrange(N_MAT) for _ in range(NNZ)]
        self.vals = MX.values_for(NNZ, q, rng)
        self.mx = MX.x_for(N_MAT, q, rng)
        self.matvec = S.encode(MX.matvec(self.rows, self.cols, self.vals, self.mx, N_MAT, q))
        # ---- the gate expression: one wire of a permutation step over the two vectors, Z rotated by one row
        self.expr_terms = EX.permutation_wire(rng.randrange(q), rng.randrange(q), q, z=0, w=1, sigma=1, ident=0)
        self.expr = S.encode(EX.model([self.xs, self.ys], self.expr_terms, N_VEC, q))
        # ---- the sumcheck step: both tables bound in place, the next round over the bound tables
        self.step_terms = SS.mixed_terms(2, q, rng)
        self.step_r = rng.randrange(q)
        assert N_VEC >= 1 << STEP_VARS
        self.step = SS.step([self.xs[:1 << STEP_VARS], self.ys[:1 << STEP_VARS]], self.step_terms, self.step_r, q)

    def transform(self, L):
        if self.log_n is None:
            two = NT.pass_log(L) + 1
            self.two_pass = NT.two_adicity(self.label) >= two
            self.log_n = two if self.two_pass else 1
            n = 1 << self.log_n
            assert len(NT.plan(L, NT.curve_id(self.label), self.log_n)[1]) == (2 if self.two_pass else 1)
            self.v = NT.inputs(self.label, n, 21)
            self.ntt = S.encode(NT.transform(self.q, self.v, n, NT.root(self.label, self.log_n)))
        return self.log_n


_data = {}


def _data_of(label):
    if label not in _data:
        _data[label] = Data(label)
    return _data[label]


class Context:
    """the resident inputs of one fresh context"""

    def __init__(self, curve, d):
        par = curve.Parallel
        self.curve, self.par, self.d = curve, par, d
        self.gen = par.randomPointsFast(N_CHECK, SEED_P)
        fb = curve.fe_bytes
        xy, inf = _raw_points(curve, self.gen)
        xy, inf = bytearray(xy), bytearray(inf)
        for i, p in d.planted.items():
            data, flag = U.encode(d.params, [p])
            xy[2 * fb * i:2 * fb * (i + 1)] = data
            inf[i] = 1 if flag else 0
        self.planted = par.pointsFromBytes(bytes(xy), N_CHECK, bytes(inf) if any(inf) else None)
        self.sc = par.randomScalars(N_MSM, SEED_S)
        self.table, self.column = _upload(curve, d.table), _upload(curve, d.column)
        self.x, self.y = _upload(curve, d.xs), _upload(curve, d.ys)
        self.fs = _upload(curve, d.fs)
        self.mx = _upload(curve, d.mx)


def _check(c):
    r = c.par.checkPoints(c.planted, verdicts=True)
    first = U.NO_INDEX if r.firstBad is None else r.firstBad
    assert (r.offCurve, r.offSubgroup, first) == c.d.check
    assert list(r.verdicts) == c.d.verdicts


def _msm(c):
    opts = {"glv": 0} if c.d.params["kind"] == "weierstrass" else {}
    r = c.par.msm(c.sc, c.gen, N_MSM, False, opts)["result"]
    assert _pt(c.d.label, r) == c.d.msm


def _lookup(c):
    m, info = c.par.lookupMultiplicities(c.column, c.table, positions=True)
    want_m, want_pos, want_info = c.d.lookup
    assert _raw_scalars(c.curve, m) == S.encode(want_m)
    assert [int(p) for p in info.pop("positions")] == want_pos
    assert info == want_info
    m.free()


def _dot(c):
    assert c.par.innerProduct(c.x, c.y) == c.d.dot


def _recurrence(c):
    out, last = c.par.scalarRecurrence(c.x, c.y, N_VEC)
    vals, want_last = c.d.rec
    assert last == want_last and _raw_scalars(c.curve, out) == S.encode(vals)
    out.free()


def _transform(c):
    d = c.d
    log_n = d.transform(_lib())
    x = _upload(c.curve, d.v)
    f = c.par.ntt(x, log_n)
    assert _raw_scalars(c.curve, f) == d.ntt
    back = c.par.ntt(f, log_n, inverse=True)
    assert _raw_scalars(c.curve, back) == S.encode(d.v)
    # a second recurrence, other operands: its record is the recurrence's own, whatever the transform did
    out, last = c.par.scalarRecurrence(c.y, c.x, N_VEC)
    vals, want_last = d.rec2
    assert last == want_last and _raw_scalars(c.curve, out) == S.encode(vals)
    for a in (x, f, back, out):
        a.free()


def _fixed_base(c):
    out = c.par.fixedBaseMul(c.fs, base=(c.gen, BASE_INDEX))
    got = [M.canon(c.d.params, _strip(p)) for p in c.curve.Affine.toBigints(out)]
    assert got == c.d.fixed
    out.free()


def _matvec(c):
    d = c.d
    m = c.par.sparseMatrix(d.rows, d.cols, d.vals, (N_MAT, N_MAT))
    out = c.par.matVec(m, c.mx)
    assert _raw_scalars(c.curve, out) == d.matvec
    out.free()
    m.free()


def _expr(c):
    out = c.par.evaluateExpression([c.x, c.y], c.d.expr_terms, N_VEC)
    assert _raw_scalars(c.curve, out) == c.d.expr
    out.free()


def _sumcheck_step(c):
    d = c.d
    n = 1 << STEP_VARS
    f, g = _upload(c.curve, d.xs[:n]), _upload(c.curve, d.ys[:n])   # (copies: the step binds its tables in place)
    bound, want_degree, want_values = d.step
    degree, values = c.par.sumcheckStep([f, g], d.step_terms, STEP_VARS, d.step_r)
    assert (degree, values) == (want_degree, want_values)
    for arr, b, src in ((f, bound[0], d.xs), (g, bound[1], d.ys)):
        assert _raw_scalars(c.curve, arr) == S.encode(b + src[n // 2:n])   # the low half bound, the high half as it was
        arr.free()


STEPS = [_check, _msm, _lookup, _dot, _recurrence, _transform, _fixed_base, _matvec, _expr, _sumcheck_step]


@pytest.mark.parametrize("label", LABELS)
def test_every_family_in_one_context_both_orders(mod, label):
    d = _data_of(label)
    for order in (STEPS, STEPS[::-1]):
        with fresh(mod, label) as curve:
            c = Context(curve, d)
            for step in order:
                step(c)
            if order is STEPS:
                # what the list touches: meta_, stage_, check_, sdot_, sscan_, ntt_scratch_ (a plan of two passes only),
                # mat_carry_, the lookup's three; and the MSM's -- the sort's refs_, off_ and five more, three of the
                # plan or msmBasic, red_[0..3] and final_ (tests/test_scratch_poison_gpu.py counts them per path)
                assert scratch(curve)[0] >= (10 if d.two_pass else 9) + 15, scratch(curve)
