"""A gate expression may not depend on what device memory held before the call: the new-handle form (whose destination
is handed to the kernel as the allocator left it) and the in-place form run once as they are and again under
msmz_test_poison patterns 0x00, 0xa5 and 0x5a -- every scratch buffer of the context filled, every later allocation
filled too.  Equal bytes each time, and the answer of the Python-integer model (tests/expr_util.py).  One fresh
context per curve; the size is a few workgroups plus a partial wave."""
import ctypes as C
import random

import pytest

import expr_util as E
import scalar_ops_util as S

pytestmark = pytest.mark.gpu

MAIN = ["bls12-377", "pallas"]
PATTERNS = (0x00, 0xa5, 0x5a)


def _lib():
    from msm_zprize_amd._native import lib
    return lib()


@pytest.mark.parametrize("label", MAIN)
def test_nothing_depends_on_what_memory_held(label):
    import msm_zprize_amd as mod
    mod.startThreads()
    params = mod.curves.BY_LABEL[label]
    curve = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
    q = S.order(label)
    w = C.c_uint32(0)
    _lib().msmz_test_expr_geometry(C.byref(w), None)
    n = 3 * w.value + 70
    rng = random.Random(61 + MAIN.index(label))
    cols = E.edge_columns(8, n, q, rng)
    gate = E.plonk_gate() + [(rng.randrange(q), [(5, 1), (5, -1), (6, 2)]), (q - 1, [7] * 8)]
    y = rng.randrange(q)
    want_new = E.model(cols, gate, n, q)
    want_acc = [(y * a + g) % q for a, g in zip(cols[0], want_new)]          # out = y out + gate over column 0, in place
    up = lambda vals: curve.Parallel.scalarsFromBytes(S.encode(vals), len(vals))   # noqa: E731

    def raw(arr):
        buf = C.create_string_buffer(32 * len(arr))
        assert _lib().msmz_download_scalars(curve._ctx, arr.handle, 0, len(arr), buf) == 0
        return buf.raw

    def run():
        arrs = [up(c) for c in cols]
        shifted = [(cf, [(col + 1, rot) for col, rot in map(E.factor, fs)]) for cf, fs in gate]
        acc = up(cols[0])
        new = curve.Parallel.evaluateExpression(arrs, gate)
        assert curve.Parallel.evaluateExpression([acc] + arrs, shifted + [(y, [0])], out=acc) is acc
        got = raw(new), raw(acc)
        for a in arrs + [acc, new]:
            a.free()
        return got

    try:
        base = run()
        assert base == (S.encode(want_new), S.encode(want_acc))
        for pattern in PATTERNS:
            assert _lib().msmz_test_poison(curve._ctx, pattern, None, None) == 0
            assert run() == base, hex(pattern)
        assert _lib().msmz_test_poison(curve._ctx, -1, None, None) == 0
    finally:
        curve.close()
