"""One launch of the tree rounds' batched-affine addition (k_batch_add, csrc/batch_kernels.h) through
msmz_test_batch_add, pair by pair against the oracle's complete affine addition.

The kernel's bookkeeping depends on where a pair sits: thread `lane` of workgroup `blk` walks the pairs
t = blk*T*B + i*T + lane for i = 0 .. ilast (ilast < B-1 in a short thread of the last workgroup); the first pair's
prefix is one, the middle ones park theirs in their output record, the last one keeps it in LDS; only ADD and DBL
pairs join the product.  The MSM only launches B > 1 for rounds of 2^18 pairs or more, where the suite's inputs are
distinct random points, so these tests place every pair kind at every position deterministically, at every B the
MSM uses and at the sizes where workgroups, threads and lanes run partly empty."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_ref as BR
from oracle import params as P

pytestmark = pytest.mark.gpu

T = 256                       # MSMZ_BATCH_T (csrc/instantiate.h)
BS = [1, 2, 4, 8, 16]         # pairs per thread the MSM launches with (Engine::batch_b)
LOC_ORIG, LOC_NEG = 0x40000000, 0x80000000
ADD, DBL, OPP, TAKE_A, TAKE_B, BOTH = range(6)   # OPP: P + (-P); TAKE_A: P + inf; TAKE_B: inf + P; BOTH: inf + inf
NAMES = ["ADD", "DBL", "OPP", "TAKE_A", "TAKE_B", "BOTH"]
NON_PRODUCT = [OPP, TAKE_A, TAKE_B, BOTH]        # pairs that stay out of the batch inversion
CURVES = ["bls12-377", "pallas", "bls12-381"]
MSMZ_ERR_ARG, MSMZ_ERR_UNSUPPORTED, MSMZ_ERR_RANGE = 1, 4, 6   # include/msmz.h


def sizes(B):
    TB = T * B
    return sorted({1, T - 1, T, TB - 1, TB, TB + 1, 3 * TB + 17})


@pytest.fixture(scope="module")
def ctxs():
    import msm_zprize_amd as m
    m.startThreads()
    cache = {}

    def get(label):
        if label not in cache:
            params = m.curves.BY_LABEL[label]
            cache[label] = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
        return cache[label]

    yield get
    for c in cache.values():
        c.close()


def _lib():
    from msm_zprize_amd import _native
    return _native.lib()


class Case:
    """A pool of NP finite points (P_k = (k+1) G, or (0, y0) in place of P_0) and the launch inputs built from it:
    point k of the resident set is P_k, point NP is infinity; slot record v holds value v, where value v < NP is P_v,
    NP <= v < 2 NP is -P_(v-NP) and 2 NP is infinity."""

    def __init__(self, curve, label, NP, x0_y=None):
        prm = P.CURVES[label]
        self.curve, self.label, self.NP = curve, label, NP
        self.fb = prm["fe_bytes"]
        self.E = BR.AffineWeierstrass(prm)
        p = self.E.p
        pool, acc = [], self.E.one
        for _ in range(NP):
            pool.append(acc)
            acc = self.E.add(acc, self.E.one)
        if x0_y is not None:
            pool[0] = (0, x0_y % p, False)
            assert self.E.is_on_curve(pool[0])
        self.vals = pool + [self.E.negate(q) for q in pool] + [self.E.zero]
        self.INF = 2 * NP
        enc = lambda q: b"\0" * (2 * self.fb) if q[2] else q[0].to_bytes(self.fb, "little") + q[1].to_bytes(self.fb, "little")
        self.enc = enc
        self.pts_xy = b"".join(enc(q) for q in pool) + b"\0" * (2 * self.fb)
        self.pts_inf = bytes(NP) + b"\1"
        self.slots_xy = b"".join(enc(q) for q in self.vals)
        self.slots_inf = bytes(2 * NP) + b"\1"
        self.n_slots = 2 * NP + 1
        self.memo = {}

    def expected_rows(self, va, vb):
        keys = va.astype(np.int64) * (2 * self.NP + 1) + vb
        uniq, inv = np.unique(keys, return_inverse=True)
        rows = np.zeros((len(uniq), 2 * self.fb), dtype=np.uint8)
        for r, k in enumerate(uniq.tolist()):
            if k not in self.memo:
                a, b = divmod(k, 2 * self.NP + 1)
                self.memo[k] = np.frombuffer(self.enc(self.E.add(self.vals[a], self.vals[b])), dtype=np.uint8)
            rows[r] = self.memo[k]
        return rows[inv.reshape(-1)]

    def operands(self, kind, t, src):
        """value ids (va, vb) of pairs of the given kinds and their location words (src bit 1: a from a slot record,
        bit 0: b from a slot record)"""
        NP, INF = self.NP, self.INF
        x = t % NP
        y = (x + 1 + (t // 2) % min(5, NP - 1)) % NP
        sa = (t // NP) & 1
        sb = (t // 5) & 1
        vx, vy, vxn = x + sa * NP, y + sb * NP, x + (1 - sa) * NP
        va = np.select([kind == TAKE_B, kind == BOTH], [INF, INF], vx)
        vb = np.select([kind == ADD, kind == DBL, kind == OPP, kind == TAKE_A, kind == TAKE_B],
                       [vy, vx, vxn, INF, vx], INF)

        def ploc(v):
            idx = np.where(v == INF, NP, v % NP)
            neg = np.where(v == INF, t & 1, v >= NP)   # (a negated infinity is still infinity)
            return (LOC_ORIG | idx | np.where(neg != 0, LOC_NEG, 0)).astype(np.uint32)

        la = np.where(src & 2, va, ploc(va)).astype(np.uint32)
        lb = np.where(src & 1, vb, ploc(vb)).astype(np.uint32)
        return va, vb, np.stack([la, lb], axis=1)

    def launch(self, safe, B, desc, out_base):
        n = len(desc)
        desc = np.ascontiguousarray(desc, dtype=np.uint32)
        out = C.create_string_buffer(2 * self.fb * n)
        err = C.c_uint32(0xdead)
        st = _lib().msmz_test_batch_add(self.curve._ctx, safe, B, self.pts_xy, self.pts_inf, self.NP + 1,
                                        self.slots_xy, self.slots_inf, self.n_slots, desc.ctypes.data, n, out_base,
                                        out, C.byref(err))
        assert st == 0, f"msmz_test_batch_add: status {st}"
        return np.frombuffer(out.raw, dtype=np.uint8).reshape(n, 2 * self.fb), err.value

    def check(self, B, kind, what, safe=1, out_base=None, src=None):
        """launch pairs of the given kinds, compare each with the oracle; returns (rows, error word)"""
        n = len(kind)
        t = np.arange(n, dtype=np.int64)
        if src is None:
            src = (t + t // T + t // (T * B)) % 4
        va, vb, desc = self.operands(kind, t, src)
        if out_base is None:
            out_base = self.n_slots + 37          # not a multiple of 64, like the engine's round_base[r]
        got, err = self.launch(safe, B, desc, out_base)
        want = self.expected_rows(va, vb)
        bad = np.nonzero((got != want).any(axis=1))[0]
        if len(bad):
            g = geometry(n, B)
            lines = [f"t={k} blk={g['blk'][k]} i={g['i'][k]} lane={g['lane'][k]} ilast={g['ilast'][k]} "
                     f"kind={NAMES[kind[k]]} src={src[k]}" for k in bad[:6].tolist()]
            pytest.fail(f"{self.label} B={B} n={n} out_base={out_base} safe={safe} {what}: {len(bad)} wrong pairs, "
                        f"first: " + "; ".join(lines))
        return got, err


def geometry(n, B):
    """position of pair t in the launch: workgroup, step i of its thread, lane, the thread's last step"""
    t = np.arange(n, dtype=np.int64)
    blk = t // (T * B)
    i = (t % (T * B)) // T
    lane = t % T
    ilast = np.minimum((n - 1 - blk * T * B - lane) // T, B - 1)
    return {"t": t, "blk": blk, "i": i, "lane": lane, "ilast": ilast}


def mixed(n, B):
    """every kind at every position: kind walks the six kinds with t, shifted per step and per workgroup"""
    g = geometry(n, B)
    return ((g["t"] * 5 + g["i"] + g["blk"]) % 6).astype(np.int64)


# placement of a kind K among ADD pairs (or of one ADD among K pairs), per thread position
PATTERNS = {
    "first": lambda g, K: np.where(g["i"] == 0, K, ADD),
    "last": lambda g, K: np.where(g["i"] == g["ilast"], K, ADD),
    "middle": lambda g, K: np.where((g["i"] > 0) & (g["i"] < g["ilast"]), K, ADD),
    "all_but_first_add": lambda g, K: np.where(g["i"] == 0, ADD, K),
    "all_but_middle_add": lambda g, K: np.where(g["i"] == g["ilast"] // 2, ADD, K),
    "all_but_last_add": lambda g, K: np.where(g["i"] == g["ilast"], ADD, K),
    "all": lambda g, K: np.full(len(g["t"]), K),
}

_cases = {}


def case(ctxs, label, NP=97, x0=False):
    key = (label, NP, x0)
    if key not in _cases:
        x0_y = {"bls12-377": 1, "bls12-381": 2}[label] if x0 else None
        _cases[key] = Case(ctxs(label), label, NP, x0_y)
    return _cases[key]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("label", CURVES)
def test_sizes_with_every_kind(ctxs, label, B):
    """every launch size where workgroups, threads (ilast < B-1) or lanes run partly empty; all six kinds mixed over
    all positions and all four operand sources; output records aligned and not aligned to 64"""
    cs = case(ctxs, label)
    for n in sizes(B):
        for ob in (cs.n_slots + 37, 256):
            cs.check(B, mixed(n, B), f"mixed kinds, n={n}", out_base=ob)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("label", CURVES)
def test_kind_at_each_thread_position(ctxs, label, B):
    """each non-ADD kind first / last / in the middle of a thread's pairs, everywhere but one ADD (first, middle,
    last), and everywhere; at 3 T B + T (B/2) + 17 pairs: three full workgroups and a partial one whose threads stop
    at ilast = B/2 or B/2 - 1"""
    cs = case(ctxs, label)
    n = 3 * T * B + T * (B // 2) + 17
    g = geometry(n, B)
    for K in (DBL, OPP, TAKE_A, TAKE_B, BOTH):
        for name, pat in PATTERNS.items():
            cs.check(B, pat(g, K).astype(np.int64), f"{NAMES[K]} {name}")


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("label", CURVES)
def test_workgroup_patterns(ctxs, label, B):
    """a workgroup without ADD / DBL pairs (it inverts a product of ones) between full ones; a workgroup whose only
    ADD is lane 255's last pair; lanes with product pairs next to lanes without (level 1 of the product tree pairs
    lane 2k with 2k+1), both ways round"""
    cs = case(ctxs, label)
    n = 3 * T * B + 17
    g = geometry(n, B)
    t, blk, i, lane = g["t"], g["blk"], g["i"], g["lane"]
    prod = np.where(t % 3 == 1, DBL, ADD)
    nonp = np.array(NON_PRODUCT)[(t + i) % 4]
    cs.check(B, np.where(blk == 1, nonp, prod), "workgroup 1 without ADD/DBL")
    cs.check(B, np.where(blk == 0, nonp, prod), "workgroup 0 without ADD/DBL")
    lone = (lane == T - 1) & (i == B - 1)
    cs.check(B, np.where(blk == 1, np.where(lone, ADD, nonp), prod), "workgroup 1's only ADD at lane 255, i=B-1")
    cs.check(B, np.where(lane % 2 == 0, prod, nonp), "even lanes ADD/DBL, odd lanes none")
    cs.check(B, np.where(lane % 2 == 1, prod, nonp), "odd lanes ADD/DBL, even lanes none")
    # lanes without any pair: 17 pairs in the last workgroup, lane 16 has one, lane 17 none
    cs.check(B, np.where(blk == 3, DBL, prod), "partial workgroup of DBL pairs")


@pytest.mark.parametrize("label", CURVES)
def test_operand_sources(ctxs, label):
    """DBL and OPP (and TAKE) pairs whose operands come from different sources: slot P with point P, slot P with
    point -P (negate bit), point -P with point -P, ... -- each source combination at every kind, at B = 1 and 16"""
    cs = case(ctxs, label)
    for B in (1, 16):
        n = 3 * T * B + 17
        t = np.arange(n, dtype=np.int64)
        for s in range(4):
            cs.check(B, mixed(n, B), f"source {s} for every pair", src=np.full(n, s))
            cs.check(B, np.where(t % 2 == 0, DBL, OPP), f"DBL/OPP, source {s}", src=np.full(n, s))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("label", ["bls12-377", "bls12-381"])
def test_points_with_x_zero(ctxs, label, B):
    """(0, +-1) on BLS12-377 and (0, +-2) on BLS12-381 lie on the curve (outside G1): their x words are all zero like
    the infinity record's, so the packed safe branch must tell them apart by y -- doubling, opposite and generic
    additions at every position"""
    cs = case(ctxs, label, NP=5, x0=True)
    assert cs.vals[0][0] == 0 and cs.vals[cs.NP][0] == 0
    n = 3 * T * B + 17
    g = geometry(n, B)
    cs.check(B, mixed(n, B), "x = 0 pool, mixed kinds")
    for K in (ADD, DBL, OPP):
        cs.check(B, np.full(n, K), f"x = 0 pool, all {NAMES[K]}")
    cs.check(B, PATTERNS["last"](g, DBL).astype(np.int64), "x = 0 pool, DBL last")
    cs.check(B, PATTERNS["middle"](g, DBL).astype(np.int64), "x = 0 pool, DBL middle")


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("label", CURVES)
def test_unsafe_variant(ctxs, label, B):
    """without degenerate pairs the unsafe variant is byte-identical to the safe one with error 0; one equal-x pair in
    any single workgroup of several raises error bit 0"""
    cs = case(ctxs, label)
    for n in (T * B + 1, 3 * T * B + 17):
        kind = np.full(n, ADD)
        ru, eu = cs.check(B, kind, "all ADD, unsafe", safe=0)
        rs, es = cs.check(B, kind, "all ADD, safe", safe=1)
        assert eu == 0 and es == 0
        assert np.array_equal(ru, rs)
    n = 3 * T * B + 17
    g = geometry(n, B)
    t = np.arange(n, dtype=np.int64)
    src = (t + t // T) % 4
    for w in (0, 1, 3):
        for K, pos in ((DBL, "last"), (OPP, "first")):
            sel = np.nonzero((g["blk"] == w) & (g["i"] == (g["ilast"] if pos == "last" else 0)))[0]
            tt = int(sel[len(sel) // 2])
            kind = np.full(n, ADD)
            kind[tt] = K
            va, vb, desc = cs.operands(kind, t, src)
            _, err = cs.launch(0, B, desc, cs.n_slots + 37)
            assert err & 1, f"{label} B={B}: {NAMES[K]} pair t={tt} in workgroup {w} did not raise the error flag"
            _, err = cs.check(B, kind, f"one {NAMES[K]} in workgroup {w}", src=src)
            assert err == 0


def test_hook_rejects_bad_arguments(ctxs):
    """host-side checks: nothing the caller passes can make the kernel read outside its buffers"""
    cs = case(ctxs, "bls12-377")
    t = np.arange(4, dtype=np.int64)
    _, _, desc = cs.operands(np.full(4, ADD), t, t % 4)
    ok = lambda **kw: _call(cs, **{"desc": desc, **kw})
    assert ok() == 0
    assert ok(B=0) == MSMZ_ERR_ARG and ok(B=17) == MSMZ_ERR_ARG and ok(safe=2) == MSMZ_ERR_ARG
    assert ok(out_base=cs.n_slots - 1) == MSMZ_ERR_ARG
    for bad in (LOC_ORIG | (cs.NP + 1), LOC_ORIG | LOC_NEG | (cs.NP + 1), cs.n_slots, LOC_NEG | 1):
        d = desc.copy()
        d[3, 1] = bad
        assert ok(desc=d) == MSMZ_ERR_ARG, hex(bad)
    big = np.frombuffer(cs.pts_xy, dtype=np.uint8).copy()
    big[cs.fb - 1] = 0xff                              # x of point 0 >= p
    assert ok(pts=bytes(big)) == MSMZ_ERR_RANGE
    te = ctxs("ed-on-bls12-377")
    err = C.c_uint32()
    out = C.create_string_buffer(64 * 4)
    st = _lib().msmz_test_batch_add(te._ctx, 1, 1, b"\0" * 64, None, 1, None, None, 0,
                                    np.zeros((4, 2), np.uint32).ctypes.data, 1, 0, out, C.byref(err))
    assert st == MSMZ_ERR_UNSUPPORTED


def _call(cs, desc, B=2, safe=1, out_base=None, pts=None):
    desc = np.ascontiguousarray(desc, dtype=np.uint32)
    out = C.create_string_buffer(2 * cs.fb * len(desc))
    err = C.c_uint32()
    return _lib().msmz_test_batch_add(cs.curve._ctx, safe, B, pts or cs.pts_xy, cs.pts_inf, cs.NP + 1, cs.slots_xy,
                                      cs.slots_inf, cs.n_slots, desc.ctypes.data, len(desc),
                                      cs.n_slots if out_base is None else out_base, out, C.byref(err))
