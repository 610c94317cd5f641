"""msmz_points_fixed_base without a GPU: the digit slicer, the planner and the accumulation over a window table of
csrc/fixed_base.h compiled for the host (tests/native/fixed_base_test.cpp, the same MSMZ_HD functions the kernels call)
against Python integers and the oracle; the Python argument checks of fixedBaseMul; the export, the struct layout and
the behaviour without a device; the JavaScript surface.  CPU only."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import check_points_util as U
import fixed_base_util as FB
import points_mul_util as M
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fixed_base_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "fixed_base_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
CAP = 64 << 20


@pytest.fixture(scope="module")
def driver():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fixed_base.h", "curve.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])

    def run(lines):
        out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) >= len(lines), out[-3:]
        return out[:len(lines)]

    return run


# ------------------------------------------------------------------------------------------------ digits
def _all_256_bit_inputs(c, rng):
    """inputs for the range check: the edges of every window, all ones, and random 256-bit values"""
    vals = [0, 1, (1 << 256) - 1, 1 << 255]
    half = 1 << (c - 1)
    K = -(-256 // c)
    vals += [sum(half << (c * k) for k in range(K)) % (1 << 256), sum((half + 1) << (c * k) for k in range(K)) % (1 << 256)]
    for k in range(0, 256, c):
        vals += [(1 << k) - 1 if k else 0, 1 << k, ((1 << k) + 1) % (1 << 256), (half << k) % (1 << 256),
                 ((half + 1) << k) % (1 << 256)]
    return vals + [rng.getrandbits(256) for _ in range(64)]


@pytest.mark.parametrize("c", list(range(4, 17)))
def test_digits_stay_in_range_for_any_256_bit_input(driver, c):
    """no digit leaves [-2^(c-1), 2^(c-1)] whatever the 256 bits and however few windows are cut -- inputs above the
    bound included -- so no digit indexes outside the table; and the driver's digits are the rule's (fixed_base_util)"""
    rng = random.Random(c)
    half = 1 << (c - 1)
    for bits in (1, 64, 128, 253, 255, 256):
        K = FB.windows(bits, c)
        vals = _all_256_bit_inputs(c, rng)
        got = driver([f"digits {c} {K} {v:x}" for v in vals])
        for v, line in zip(vals, got):
            d = [int(x) for x in line.split()]
            assert len(d) == K and all(-half <= x <= half for x in d), (c, bits, hex(v), d)
            assert all(x == 0 or (k << (c - 1)) + abs(x) - 1 < (K << (c - 1)) for k, x in enumerate(d))
            assert d == FB.digits(v, c, K), (c, bits, hex(v))


@pytest.mark.parametrize("label", FB.ALL)
def test_digits_recombine_to_the_scalar(driver, label):
    """sum d_k 2^(ck) == s for every scalar below the bound: 0, 1, 2, q - 1, both sides of every window boundary, a carry
    through every window, 16 random ones; widths 4, 5, 13, 16; bounds 1, 64, 128 and none"""
    params = P.CURVES[label]
    rng = random.Random(FB.ALL.index(label) + 5)
    for c in FB.WIDTHS:
        for sb in FB.BOUNDS:
            K = FB.windows(FB.bound_bits(params, sb), c)
            vals = FB.edge_scalars(params, c, sb, rng)
            assert 0 in vals and 1 in vals and (sb == 1 or len(vals) >= 20)
            got = driver([f"digits {c} {K} {v:x}" for v in vals])
            for v, line in zip(vals, got):
                d = [int(x) for x in line.split()]
                assert sum(x << (c * k) for k, x in enumerate(d)) == v, (c, sb, hex(v), d)


# ------------------------------------------------------------------------------------------------ the accumulation
@pytest.mark.parametrize("c", FB.WIDTHS)
@pytest.mark.parametrize("label", FB.ALL)
def test_host_accumulation_matches_the_oracle(driver, label, c):
    """[s]B from the digits, a table built entry by entry the way k_fixed_table builds it, and the complete mixed addition
    == the oracle's [s]B: the scalars of the issue under every bound, B = G and a random [k]G; and over a shorter scalar
    list B of small order (cofactor curves), B at infinity and the twisted Edwards identity"""
    params = P.CURVES[label]
    rng = random.Random(100 * FB.ALL.index(label) + c)
    named = FB.bases(label, rng)
    lines, want = [], []
    for sb in FB.BOUNDS:
        scalars = FB.edge_scalars(params, c, sb, rng)
        for name, b in named:
            full = name in ("G", "[k]G")
            for s in (scalars if full else scalars[:4] + scalars[-6:]):
                lines.append(f"mul {label} {c} {sb} {s:x} {b['x']:x} {b['y']:x} {int(b['isZero'])}")
                want.append(FB.expected(label, s, b))
    got = []
    for line in driver(lines):
        x, y, inf = line.split()
        got.append(U.pt(int(x, 16), int(y, 16), inf == "1"))
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:3]
    assert M.neutral(params) in want and any(w != M.neutral(params) for w in want)
    assert (len(named) > 3) == (params["cofactor"] != 1)


# ------------------------------------------------------------------------------------------------ planner
SIZES = [1, 2, 64, 1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24, 1 << 26, (1 << 29) - 1]


@pytest.mark.parametrize("label", FB.ALL)
def test_planner(driver, label):
    """the table fits 64 MiB; K = ceil((bits + 1) / c) and entries = K 2^(c-1); c in [4, 16] does not fall as n grows; a
    64-bit bound needs fewer windows than none; the choice is the cheapest by the stated model"""
    params = P.CURVES[label]
    te = params["kind"] != "weierstrass"
    for sb in FB.BOUNDS:
        bits = FB.bound_bits(params, sb)
        plans = [[int(v) for v in line.split()] for line in driver([f"plan {label} {n} {sb}" for n in SIZES])]
        for n, (c, K, entries, rec) in zip(SIZES, plans):
            assert 4 <= c <= 16 and rec == 2 * params["fe_bytes"]
            assert K == FB.windows(bits, c) and entries == K << (c - 1)
            assert entries * rec <= CAP

            def cost(cc):
                kk = FB.windows(bits, cc)
                per_entry = cc * 9 + (cc // 2) * (7 if te else 10) + 14 + (2 if te else 4)
                per_point = kk * (9 if te else 10) + 14 + (4 if te else 5)
                return (kk << (cc - 1)) * per_entry + n * per_point
            fits = [cc for cc in range(4, 17) if (FB.windows(bits, cc) << (cc - 1)) * rec <= CAP]
            assert c == min(fits, key=lambda cc: (cost(cc), cc)), (n, sb)
        cs = [p[0] for p in plans]
        assert cs == sorted(cs), (sb, cs)
        assert cs[0] < cs[-1] or sb == 1
    full = [int(v) for v in driver([f"plan {label} {1 << 20} 0"])[0].split()]
    short = [int(v) for v in driver([f"plan {label} {1 << 20} 64"])[0].split()]
    assert short[1] < full[1]
    c, K = full[0], full[1]
    per_entry, per_point = [int(v) for v in driver([f"products {label} {c} {K}"])[0].split()]
    assert per_point == K * (9 if te else 10) + 14 + (4 if te else 5)
    assert per_entry == c * 9 + (c // 2) * (7 if te else 10) + 14 + (2 if te else 4)


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(kind="scalars", n=100):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, 7, n, kind)


def test_fixed_base_args():
    from msm_zprize_amd.parallel import fixed_base_args
    p, fb = 1009, 32
    a = fixed_base_args(_arr(), None, None, 0, p, fb)
    assert a == {"N": 100, "firstScalar": 0, "baseHandle": 0, "baseIndex": 0, "baseBytes": None}
    a = fixed_base_args(_arr(), {"x": 5, "y": 6}, 40, 60, p, fb)
    assert (a["N"], a["firstScalar"]) == (40, 60)
    assert a["baseBytes"] == (5).to_bytes(32, "little") + (6).to_bytes(32, "little")
    assert fixed_base_args(_arr(), {"x": 5, "y": 6, "isZero": True}, None, 0, p, fb)["baseBytes"] == bytes(64)
    pts = _arr("points", 10)
    a = fixed_base_args(_arr(), (pts, 9), None, 1, p, fb)
    assert (a["N"], a["baseHandle"], a["baseIndex"], a["baseBytes"]) == (99, 7, 9, None)
    for N, first in [(0, 0), (-1, 0), (101, 0), (41, 60), (1, 100), (1, -1), (True, 0), (1.0, 0), (1, 1.0), (1, True)]:
        with pytest.raises(ValueError):
            fixed_base_args(_arr(), None, N, first, p, fb)
    for bad in ({"x": p, "y": 0}, {"x": 0, "y": -1}, (pts, 10), (pts, -1), (pts, True)):
        with pytest.raises(ValueError):
            fixed_base_args(_arr(), bad, None, 0, p, fb)
    for bad in (b"xy", 5, pts, (pts,), (_arr("precomputed"), 0), (_arr("scalars"), 0), {"x": 1}, {"x": 1.0, "y": 2}):
        with pytest.raises(TypeError):
            fixed_base_args(_arr(), bad, None, 0, p, fb)
    for bad in (_arr("points"), b"\x01" * 32, None, 5):
        with pytest.raises(TypeError):
            fixed_base_args(bad, None, None, 0, p, fb)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_point_and_struct_layout(lib):
    """the symbol is exported and declared; msmz_fixed_base is 48 bytes with the header's field order and offsets"""
    from msm_zprize_amd import _native
    for name in ("msmz_points_fixed_base", "msmz_test_fixed_base_plan", "msmz_test_set_fixed_base_window",
                 "msmz_test_fixed_base_tables"):
        assert name in _native.EXPORTS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "msmz.h")).read()
    assert "int msmz_points_fixed_base(msmz_ctx* ctx, const msmz_fixed_base* f, uint64_t n, uint64_t* out_handle);" in header
    body = re.search(r"typedef struct msmz_fixed_base \{(.*?)\} msmz_fixed_base;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    T = _native.MsmzFixedBase
    assert fields == [f[0] for f in T._fields_]
    assert C.sizeof(T) == 48
    want = {"base_handle": 0, "base_index": 8, "base_xy_le": 16, "scalars_handle": 24, "first_s": 32, "scalar_bits": 40,
            "flags": 44}
    assert {name: getattr(T, name).offset for name in want} == want


def test_null_arguments_are_bad_arguments(lib):
    """no context, no device: MSMZ_ERR_ARG, nothing runs, *out_handle is as it was"""
    from msm_zprize_amd import _native
    f = _native.MsmzFixedBase(0, 0, None, 1, 0, 0, 0)
    h = C.c_uint64(77)
    assert lib.msmz_points_fixed_base(None, C.byref(f), 1, C.byref(h)) == 1
    assert h.value == 77
    built = C.c_uint64(5)
    assert lib.msmz_test_fixed_base_tables(None, C.byref(built)) == 1 and built.value == 5
    assert lib.msmz_test_set_fixed_base_window(None, 13) == 1


def test_plan_hook_needs_no_context(lib, driver):
    """msmz_test_fixed_base_plan == the driver's planner; its argument errors"""
    c, K, e = C.c_int32(), C.c_int32(), C.c_uint64()
    for cid, label in enumerate(FB.ALL):
        for n in (1, 1 << 12, 1 << 20):
            for bits in (0, 1, 64, 128, 256):
                assert lib.msmz_test_fixed_base_plan(cid, n, bits, C.byref(c), C.byref(K), C.byref(e)) == 0
                want = [int(v) for v in driver([f"plan {label} {n} {bits}"])[0].split()]
                assert [c.value, K.value, e.value] == want[:3]
    assert lib.msmz_test_fixed_base_plan(4, 1, 0, C.byref(c), C.byref(K), C.byref(e)) == 1
    assert lib.msmz_test_fixed_base_plan(0, 0, 0, C.byref(c), C.byref(K), C.byref(e)) == 1
    assert lib.msmz_test_fixed_base_plan(0, 1, 257, C.byref(c), C.byref(K), C.byref(e)) == 1
    assert lib.msmz_test_fixed_base_plan(0, 1, -1, C.byref(c), C.byref(K), C.byref(e)) == 1
    assert lib.msmz_test_fixed_base_plan(0, 1, 0, None, C.byref(K), C.byref(e)) == 1


# ------------------------------------------------------------------------------------------------ JavaScript
def test_js_surface():
    """the script parses, the addon's source registers fixedBaseMul, the host module and the declaration file name it"""
    script = os.path.join(ROOT, "js", "scripts", "msm-fixed-base.mjs")
    subprocess.check_call(["node", "--check", script])
    napi = open(os.path.join(ROOT, "napi", "msmz_napi.c")).read()
    assert '"fixedBaseMul"' in napi and "msmz_points_fixed_base" in napi
    assert "fixedBaseMul(" in open(os.path.join(ROOT, "js", "parallel.mjs")).read()
    assert "fixedBaseMul(" in open(os.path.join(ROOT, "js", "parallel.d.ts")).read()
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "fixed_base_js_fixture.json"))
