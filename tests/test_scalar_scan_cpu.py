"""Recurrences and inversion over scalar sets without a GPU: fr_inv, the affine maps of csrc/fr.h and the per-thread
bodies of csrc/scan_kernels.h compiled for the host (tests/native/scalar_scan_test.cpp, the same templates the kernels
instantiate) against Python integers; the same program once more under the address and undefined-behaviour
sanitizers; the Python argument checks; the exports and the behaviour without a device.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import scalar_ops_util as S
import scalar_scan_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "scalar_scan_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "scalar_scan_test")
EXE_ASAN = EXE + "_asan"
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "scan_kernels.h", "scalar_kernels.h", "fp.h", "constants_gen.h")]


def _build(exe, extra):
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + extra + ["-o", exe, SRC])


def _run(exe, lines):
    """request lines -> one list of ints per answer line"""
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-3000:]
    out = res.stdout.split("\n")
    assert len(out) >= len(lines)
    return [[int(v, 16) for v in line.split()] for line in out[:len(lines)]]


@pytest.fixture(scope="module")
def driver():
    _build(EXE, [])
    return lambda lines: _run(EXE, lines)


@pytest.fixture(scope="module")
def geometry(driver):
    out = subprocess.run([EXE], input="geometry\n", capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(("rec_tile", "rec_pass", "inv_chunk", "rec_run", "inv_run"), (int(v) for v in out)))


def inv_operands(label):
    q = S.order(label)
    rng = random.Random(77 + S.ALL.index(label))
    return [1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, (1 << 32) - 1, 1 << 32, pow(2, 255, q), S.low_words_full(q)] + \
        [rng.randrange(1, q) for _ in range(64)]


@pytest.mark.parametrize("label", S.ALL)
def test_fr_inv_matches_python(driver, label):
    """fr_inv against pow(x, -1, q) on the edge operands and 64 random values, x * fr_inv(x) == 1 for each; 0 -> 0"""
    q = S.order(label)
    ops = inv_operands(label)
    got = driver([f"{label} inv {x:x}" for x in ops + [0]])
    bad = [(hex(x), g) for x, g in zip(ops, got) if g != [pow(x, -1, q), 1]]
    assert not bad, bad[:3]
    assert got[-1] == [0, 0]


def map_operands(label):
    q = S.order(label)
    rng = random.Random(5 + S.ALL.index(label))
    return [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, (1 << 32) - 1, 1 << 224, S.low_words_full(q), rng.randrange(q),
            rng.randrange(q)]


@pytest.mark.parametrize("label", S.ALL)
def test_map_composition_matches_integers(driver, label):
    """(a2, b2) o (a1, b1) = (a2 a1, a2 b1 + b2) over ALL pairs of maps drawn from a 12-value operand set (a map takes
    its a and its b from neighbouring operands, so every value appears in both places)"""
    q = S.order(label)
    ops = map_operands(label)
    assert len(ops) == 12
    maps = [(ops[i], ops[(i + 5) % 12]) for i in range(12)]
    pairs = [(g, f) for g in maps for f in maps]
    got = driver([f"{label} map {g[0]:x} {g[1]:x} {f[0]:x} {f[1]:x}" for g, f in pairs])
    bad = [(g, f, r) for (g, f), r in zip(pairs, got) if r != [g[0] * f[0] % q, (g[0] * f[1] + g[1]) % q]]
    assert not bad, bad[:2]


@pytest.mark.parametrize("label", S.ALL)
def test_map_composition_is_associative(driver, label):
    q = S.order(label)
    rng = random.Random(11 + S.ALL.index(label))
    triples = [[rng.randrange(q) for _ in range(6)] for _ in range(32)]
    got = driver([f"{label} map3 " + " ".join(f"{v:x}" for v in t) for t in triples])
    for (a3, b3, a2, b2, a1, b1), r in zip(triples, got):
        want = [a3 * a2 * a1 % q, (a3 * (a2 * b1 + b2) + b3) % q]
        assert r == want + want


def rec_line(label, mode, flags, n, init, a, b):
    _, mult, addend = U.MODE[mode]
    am = {None: 0, "broadcast": 1, "resident": 2}[mult]
    vals = (a if am == 2 else []) + (b if addend else [])
    return (f"{label} rec {am} {int(addend)} {flags} {n} {init:x} {(a if am == 1 else 0):x} " +
            " ".join(f"{v:x}" for v in vals)).strip()


@pytest.mark.parametrize("label", S.ALL)
def test_thread_bodies_chain_to_the_sequential_recurrence(driver, geometry, label):
    """compose a run, combine runs, apply to the incoming value, walk the run -- what the three kernels chain -- for n in
    {1, 2, run - 1, run, run + 1, 3 run + 2}, every mode, both directions, inclusive and exclusive, with a random
    and the default init, against the plain loop"""
    q = S.order(label)
    run = geometry["rec_run"]
    lines, want = [], []
    for n in sorted({1, 2, run - 1, run, run + 1, 3 * run + 2}):
        for mode, _, addend in U.MODES:
            a, b = U.mode_operands(label, mode, n, 3)
            for flags in range(4):
                for init in (None, q - 1, random.Random(n + flags).randrange(q)):
                    start = (0 if addend else 1) if init is None else init
                    lines.append(rec_line(label, mode, flags, n, start, a, b))
                    out, last = U.recurrence(q, n, a, b, init, bool(flags & 1), bool(flags & 2))
                    want.append(out + [last])
    got = driver(lines)
    bad = [(line[:60], g[:3], w[:3]) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]


@pytest.mark.parametrize("label", S.ALL)
def test_inverse_thread_body(driver, geometry, label):
    """one thread of k_scalars_inverse over a whole and a partial run, with zeros at the first, the last, every and no
    position"""
    q = S.order(label)
    run = geometry["inv_run"]
    rng = random.Random(21 + S.ALL.index(label))
    lines, want = [], []
    for count in (1, 2, run - 1, run):
        base = [rng.randrange(1, q) for _ in range(count)]
        base[0] = q - 1
        for zeros in ([], [0], [count - 1], [0, count - 1], list(range(count))):
            xs = [0 if i in zeros else v for i, v in enumerate(base)]
            lines.append(f"{label} sinv {count} " + " ".join(f"{v:x}" for v in xs))
            want.append(U.inverse(q, xs)[0] + [sum(1 << i for i in set(zeros))])
    got = driver(lines)
    bad = [(line[:50], g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]


def test_sanitizer_build_runs_clean(driver):
    """the same stand-alone program built with -fsanitize=address,undefined, run as a process of its own on requests of
    every kind: it exits 0, writes nothing to stderr, and answers as the plain build does"""
    _build(EXE_ASAN, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    lines = []
    for label in S.ALL:
        q = S.order(label)
        lines += [f"{label} inv {q - 2:x}", f"{label} inv 0", f"{label} map {q - 1:x} 1 2 {q - 1:x}",
                  f"{label} map3 1 2 3 4 5 6", f"{label} sinv 3 0 5 {q - 1:x}", f"{label} sinv 8 1 2 3 0 5 6 7 0"]
        for mode, _, _ in U.MODES:
            for n in (1, 9, 26):
                a, b = U.mode_operands(label, mode, n, 4)
                for flags in (0, 3):
                    lines.append(rec_line(label, mode, flags, n, 5, a, b))
    assert _run(EXE_ASAN, lines) == driver(lines)


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=100, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


def _rec(a, b, N=None, init=None, reverse=False, exclusive=False, firstA=0, firstB=0, out=None, firstOut=0, q=1009):
    from msm_zprize_amd.parallel import scalar_recurrence_args
    return scalar_recurrence_args(a, b, N, init, reverse, exclusive, firstA, firstB, out, firstOut, q)


def _inv(x, N=None, first=0, out=None, firstOut=0):
    from msm_zprize_amd.parallel import invert_scalars_args
    return invert_scalars_args(x, N, first, out, firstOut)


def test_scalar_recurrence_args_accepts():
    x, y = _arr(100, 1), _arr(80, 2)
    t = _rec(None, x)
    assert (t["N"], t["aHandle"], t["a"], t["bHandle"], t["init"], t["flags"]) == (100, 0, None, 1, None, 0)
    t = _rec(x, None, exclusive=True)
    assert (t["N"], t["aHandle"], t["bHandle"], t["flags"]) == (100, 1, 0, 2)
    t = _rec(7, y, reverse=True, exclusive=True, init=0)
    assert (t["N"], t["a"], t["init"], t["flags"]) == (80, (7).to_bytes(32, "little"), bytes(32), 3)
    assert _rec(x, y, firstA=30, firstB=20)["N"] == 60
    assert _rec(5, None, N=10)["N"] == 10 and _rec(0, None, N=10)["a"] == bytes(32)
    assert _rec(x, y, 50, out=x)["firstOut"] == 0                    # in place over the a range
    assert _rec(x, x, 40, firstA=0, firstB=50, out=x, firstOut=50)["firstOut"] == 50   # ... over the b range
    assert _rec(x, None, 10, out=x, firstOut=80)["N"] == 10          # apart inside the same handle
    assert _rec(1008, y, init=1008, reverse=True)["flags"] == 1


def test_scalar_recurrence_args_refuses():
    x, y = _arr(100, 1), _arr(80, 2)
    with pytest.raises(TypeError):
        _rec(None, None, N=5)
    for bad in (_arr(100, 4, "points"), b"x" * 32, 1.5, True):
        with pytest.raises(TypeError):
            _rec(bad, y)
        with pytest.raises(TypeError):
            _rec(x, bad)
        with pytest.raises(TypeError):
            _rec(x, y, out=bad)
    with pytest.raises(TypeError):
        _rec(x, 7)                                   # an int addend
    for bad in (1.0, "1", True, b"\x01"):
        with pytest.raises(TypeError):
            _rec(x, y, init=bad)
    for name in ("reverse", "exclusive"):
        with pytest.raises(TypeError):
            _rec(x, y, **{name: 1})
    for v in (1009, -1, 1 << 256):
        with pytest.raises(ValueError):
            _rec(v, y)
        with pytest.raises(ValueError):
            _rec(x, y, init=v)
    for name in ("N", "firstA", "firstB", "firstOut"):
        for bad in (-1, True, 1.0, "1"):
            with pytest.raises(ValueError):
                _rec(x, x, **{"N": 10, "out": x, name: bad})
    for kw in (dict(N=0), dict(N=101), dict(N=1 << 32), dict(N=51, firstA=50), dict(N=1, firstA=100), dict(N=10, firstB=71),
               dict(N=10, out=y, firstOut=71)):
        with pytest.raises(ValueError):
            _rec(x, y, **kw)
    with pytest.raises(ValueError):
        _rec(3, y, firstA=2)                         # firstA without a multiplier array
    with pytest.raises(ValueError):
        _rec(x, None, firstB=2)                      # firstB without an addend
    with pytest.raises(ValueError):
        _rec(x, None, firstOut=2)                    # firstOut without out
    with pytest.raises(ValueError):
        _rec(3, None)                                # no array gives the length
    for first_out in (1, 25, 49):
        with pytest.raises(ValueError):
            _rec(x, None, 50, out=x, firstOut=first_out)
        with pytest.raises(ValueError):
            _rec(None, x, 50, out=_arr(100, 1), firstOut=first_out)   # another object for the same handle


def test_invert_scalars_args():
    x, y = _arr(100, 1), _arr(80, 2)
    assert _inv(x) == {"N": 100, "first": 0, "firstOut": 0}
    assert _inv(x, None, 30, y, 20) == {"N": 60, "first": 30, "firstOut": 20}
    assert _inv(x, 50, 0, x, 0)["N"] == 50 and _inv(x, 50, 0, x, 50)["firstOut"] == 50
    for bad in (_arr(100, 4, "points"), None, 7, b"x"):
        with pytest.raises(TypeError):
            _inv(bad)
        if bad is not None:
            with pytest.raises(TypeError):
                _inv(x, out=bad)
    for kw in (dict(N=0), dict(N=101), dict(N=True), dict(first=-1), dict(first=100), dict(N=2, first=99), dict(firstOut=1),
               dict(N=10, out=y, firstOut=71), dict(N=50, out=x, firstOut=25), dict(N=50, first=10, out=_arr(100, 1), firstOut=0)):
        with pytest.raises(ValueError):
            _inv(x, **kw)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in ("msmz_scalars_recurrence", "msmz_scalars_inverse", "msmz_test_scalar_scan_geometry"):
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    from msm_zprize_amd.parallel import _Parallel
    for name in ("scalarRecurrence", "prefixProducts", "prefixSums", "divideByLinear", "invertScalars"):
        assert callable(getattr(_Parallel, name))
    assert C.sizeof(_native.MsmzScalarRec) == 56


def test_scan_geometry_accessor(lib, geometry):
    """msmz_test_scalar_scan_geometry == the constants the host driver was compiled with; needs no context"""
    t, p, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lib.msmz_test_scalar_scan_geometry(C.byref(t), C.byref(p), C.byref(c))
    assert [t.value, p.value, c.value] == [geometry["rec_tile"], geometry["rec_pass"], geometry["inv_chunk"]]
    assert t.value == 256 * geometry["rec_run"] and c.value == 64 * geometry["inv_run"] and p.value >= 64
    lib.msmz_test_scalar_scan_geometry(None, None, None)


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG and the outputs untouched, for both entry points"""
    from msm_zprize_amd import _native
    one = (1).to_bytes(32, "little")
    rec = _native.MsmzScalarRec(1, 0, None, 0, 0, one, 0)
    h = C.c_uint64(0)
    last = C.create_string_buffer(b"\xaa" * 32, 32)
    assert lib.msmz_scalars_recurrence(None, C.byref(rec), 1, 0, C.byref(h), last) == 1
    assert h.value == 0 and last.raw == b"\xaa" * 32
    zeros = C.c_uint64(99)
    h = C.c_uint64(77)
    assert lib.msmz_scalars_inverse(None, 1, 0, 1, 0, C.byref(h), C.byref(zeros)) == 1
    assert h.value == 77 and zeros.value == 99
