"""Compressed point sets without a GPU: csrc/sqrt.h and the `decompress` of both curve groups (csrc/curve.h) compiled
for the host (tests/native/sqrt_test.cpp, the templates the import kernel instantiates) against Python integers; the
Python argument helpers; the export, the new status text and the behaviour without a device.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import check_points_util as U
import compressed_util as Z
from oracle import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sqrt_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "sqrt_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


@pytest.fixture(scope="module")
def driver():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("sqrt.h", "curve.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])

    def run(lines):
        out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) >= len(lines)
        return [o.split() for o in out[:len(lines)]]

    return run


def test_field_geometry(driver):
    """S of the four base fields, C = min(4, S), N = ceil(S / C), and the shift that puts the short digit at the bottom"""
    assert driver(["info"])   # (built)
    out = subprocess.run([EXE], input="info\n", capture_output=True, text=True, check=True).stdout.split("\n")[:4]
    got = [[int(v) for v in row.split()] for row in out]
    for label, (s, c, n, delta, products) in zip(U.ALL, got):
        S, _ = Z.two_adicity(P.CURVES[label]["modulus"])
        assert s == S and c == min(4, S) and n == -(-S // c) and delta == c * n - S
        assert 0 < products < 700
    assert [g[0] for g in got] == [46, 32, 1, 47]


def _sqrt_vectors(label):
    """0, 1, 4, p - 1, b; 200 random values; for every k = 0 .. S an element of exact order 2^k times a random odd-order
    square: the first non-zero digit of the logarithm lands in every window, the short one included; k = S is a
    non-residue"""
    params = P.CURVES[label]
    p = params["modulus"]
    rng = random.Random(U.ALL.index(label) + 7)
    S, t = Z.two_adicity(p)
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    w = pow(g, t, p)
    vec = [0, 1, 4, p - 1, params.get("b", params.get("d"))] + [rng.randrange(p) for _ in range(200)]
    orders = []
    for k in range(S + 1):
        z = pow(w, 1 << (S - k), p) if k else 1
        assert pow(z, 1 << k, p) == 1 and (k == 0 or pow(z, 1 << (k - 1), p) != 1)
        odd = pow(rng.randrange(2, p), 1 << (S + 1), p)   # an odd-order element, squared
        orders.append(z * odd % p)
    return vec, orders


@pytest.mark.parametrize("label", U.ALL)
def test_sqrt_matches_euler_and_squares_back(driver, label):
    p = P.CURVES[label]["modulus"]
    vec, orders = _sqrt_vectors(label)
    out = driver([f"sqrt {label} {a:x}" for a in vec + orders])
    verdicts = []
    for a, (ok, r) in zip(vec + orders, out):
        residue = a % p == 0 or pow(a, (p - 1) // 2, p) == 1
        assert (ok == "1") == residue, hex(a)
        if residue:
            assert int(r, 16) ** 2 % p == a % p, hex(a)
        verdicts.append(residue)
    assert out[0] == ["1", "0" * len(out[0][1])]                  # sqrt(0) = 0
    assert True in verdicts[5:205] and False in verdicts[5:205]  # both outcomes among the random values
    assert verdicts[205:] == [True] * (len(orders) - 1) + [False]   # exact order 2^S: refused, every lower order: a root


def _dec_lines(label, recs):
    return [f"dec {label} {wire:x} {bit} {1 if sign == 'parity' else 0}" for wire, bit, sign in recs]


@pytest.mark.parametrize("label", U.ALL)
def test_decompress_matches_python(driver, label):
    """k G for a dozen k and the named points of the curve (zero roots, small orders), both conventions: the record
    decompresses to the point, the flipped sign bit to its negative, a sign bit on a zero root is refused"""
    params = P.CURVES[label]
    p = params["modulus"]
    rng = random.Random(5)
    g = U.generator(params)
    pts = [U.scale(params, k, g) for k in (1, 2, 3, 5, 7, 0xFFFF, params["order"] - 1, params["order"] - 2)]
    pts += [U.scale(params, rng.randrange(params["order"]), g) for _ in range(4)] + Z.on_curve_named(label)
    recs, want = [], []
    for q in pts:
        wire, other = Z.wire_other(params, q)
        for sign in Z.SIGNS:
            bit = Z.sign_of(other, p, sign)
            recs.append((wire, bit, sign))
            want.append(q)
            recs.append((wire, bit ^ 1, sign))
            want.append(None if other == 0 else Z.negated(params, q))
    zero_roots = 0
    for (wire, bit, sign), q, (st, x, y) in zip(recs, want, driver(_dec_lines(label, recs))):
        assert q == Z.decompress(params, wire, bit, sign)   # (the Python reference agrees with the vector)
        if q is None:
            assert st == "1"
            zero_roots += 1
        else:
            assert (st, int(x, 16), int(y, 16)) == ("0", q["x"], q["y"]), (hex(wire), bit, sign)
    assert zero_roots == 2 * len(Z.zero_root_wires(params))
    # the named points the issue lists are among the vectors
    named = {"bls12-377": [(0, 1), (0, p - 1), (p - 1, 0)], "bls12-381": [(0, 2), (0, p - 2)],
             "ed-on-bls12-377": [(0, 1), (0, p - 1)], "pallas": []}[label]
    have = {(q["x"], q["y"]) for q in want if q}
    assert all(v in have for v in named)


@pytest.mark.parametrize("label", U.ALL)
def test_decompress_refuses_what_has_no_root(driver, label):
    params = P.CURVES[label]
    rng = random.Random(9)
    wires = [Z.non_residue_wire(params, rng) for _ in range(6)]
    out = driver(_dec_lines(label, [(w, b, s) for w in wires for b in (0, 1) for s in Z.SIGNS]))
    assert [o[0] for o in out] == ["1"] * len(out)


@pytest.mark.parametrize("label", U.ALL)
def test_signs(driver, label):
    """fe_wire_sign, what compression writes: both conventions at 0, 1, (p-1)/2, (p+1)/2, p-1 and random values"""
    p = P.CURVES[label]["modulus"]
    rng = random.Random(2)
    vals = [0, 1, 2, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1] + [rng.randrange(p) for _ in range(20)]
    lines = [f"sign {label} {v:x} {par}" for v in vals for par in (0, 1)]
    want = [[str(Z.sign_of(v, p, "parity" if par else "largest")), str(int(v == 0))] for v in vals for par in (0, 1)]
    assert driver(lines) == want


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(kind="points", n=100):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, 1, n, kind)


def test_compressed_arg():
    from msm_zprize_amd.parallel import compressed_arg, sign_arg
    assert compressed_arg(False, "largest", False, "t") == 0
    assert compressed_arg(False, "largest", True, "t") == 0
    assert compressed_arg(True, "largest", False, "t") == 8
    assert compressed_arg(True, "parity", False, "t") == 24
    assert sign_arg("largest", "t") == 0 and sign_arg("parity", "t") == 16
    for bad in ("Largest", "odd", "", None, 1, True):
        with pytest.raises(ValueError):
            sign_arg(bad, "t")
    with pytest.raises(ValueError):
        compressed_arg(False, "parity", False, "t")   # a sign convention without compressed records
    with pytest.raises(ValueError):
        compressed_arg(True, "largest", True, "t")    # compressed Montgomery records
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError):
            compressed_arg(bad, "largest", False, "t")


def test_compressed_range_args():
    from msm_zprize_amd.parallel import compressed_range_args
    assert compressed_range_args(_arr(), 0, None, "t") == (0, 100)
    assert compressed_range_args(_arr(), 40, None, "t") == (40, 60)
    assert compressed_range_args(_arr(), 99, 1, "t") == (99, 1)
    for first, n in [(-1, 1), (100, 1), (0, 0), (0, 101), (50, 51), (0, -3), (True, 1), (0, True), (1.0, 1), (0, 2.0)]:
        with pytest.raises(ValueError):
            compressed_range_args(_arr(), first, n, "t")
    for bad in (_arr("scalars"), _arr("precomputed"), b"points", None):
        with pytest.raises(TypeError):
            compressed_range_args(bad, 0, None, "t")


class _FakeTensor:
    def __init__(self, n, k):
        self.shape, self._k = (n, k), k
        self.device = type("D", (), {"type": "cpu", "index": None})()

    def dim(self): return 2
    def stride(self, d): return self._k if d == 0 else 1
    def element_size(self): return 1
    def data_ptr(self): return 4096


def test_tensor_rows_are_one_coordinate():
    from msm_zprize_amd.parallel import tensor_view
    v = tensor_view(_FakeTensor(5, 48), [0], "points", 48, False, "t", compressed=True)
    assert (v["n"], v["width"], v["stride"]) == (5, 48, 48)
    with pytest.raises(ValueError):
        tensor_view(_FakeTensor(5, 96), [0], "points", 48, False, "t", compressed=True)
    with pytest.raises(ValueError):
        tensor_view(_FakeTensor(5, 48), [0], "points", 48, False, "t")
    assert tensor_view(_FakeTensor(5, 96), [0], "points", 48, False, "t")["width"] == 96   # (unchanged)


@pytest.mark.parametrize("label", U.ALL)
def test_compress_point_is_the_record(label):
    """the pure-Python compressPoint == the records the tests build, and decompresses back (Python reference)"""
    from msm_zprize_amd.parallel import compress_point
    params = P.CURVES[label]
    p = params["modulus"]
    rng = random.Random(4)
    for q in [U.generator(params)] + Z.on_curve_named(label) + [U.raw_point(params, rng) for _ in range(6)]:
        for sign in Z.SIGNS:
            rec, inf = compress_point(params, q, sign)
            assert rec == Z.record(params, q, sign) and inf is False
            v = int.from_bytes(rec, "little")
            assert Z.decompress(params, v & ((1 << (8 * len(rec) - 1)) - 1), v >> (8 * len(rec) - 1), sign) == q
    if params["kind"] == "weierstrass":
        assert compress_point(params, U.pt(0, 1, True), "largest") == (bytes(params["fe_bytes"]), True)
    for bad in (U.pt(p, 1), U.pt(1, -1), U.pt(1.0, 2)):
        with pytest.raises(ValueError):
            compress_point(params, bad, "largest")
    with pytest.raises(ValueError):
        compress_point(params, U.generator(params), "odd")


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_point_is_exported(lib):
    from msm_zprize_amd import _native
    assert "msmz_download_points_compressed" in _native.EXPORTS
    assert lib.msmz_download_points_compressed is not None
    assert (_native.MSMZ_SRC_COMPRESSED, _native.MSMZ_SRC_SIGN_PARITY, _native.MSMZ_ERR_POINT) == (8, 16, 7)
    header = open(os.path.join(ROOT, "include", "msmz.h")).read()
    for text in ("MSMZ_SRC_COMPRESSED = 8", "MSMZ_SRC_SIGN_PARITY = 16", "MSMZ_ERR_POINT = 7"):
        assert text in header


def test_null_context_is_a_bad_argument(lib):
    from msm_zprize_amd import _native
    buf = C.create_string_buffer(48)
    assert lib.msmz_download_points_compressed(None, 1, 0, 1, buf, None, 0) == 1
    src = _native.MsmzSrc(C.cast(buf, C.c_void_p), 0, 48, _native.MSMZ_SRC_COMPRESSED, None, None)
    h = C.c_uint64(0)
    assert lib.msmz_import_points(None, C.byref(src), 1, C.byref(h)) == 1 and h.value == 0


def test_status_text(lib):
    assert lib.msmz_strerror(7) == b"a compressed record is not a point of the curve"
    assert lib.msmz_strerror(6) == b"scalar >= group order or coordinate >= field modulus"
    assert lib.msmz_strerror(8) == b"unknown status"
