"""The number-theoretic transform without a GPU: the constants of the four scalar fields, the planner
(csrc/ntt_plan.h) at every length, and a host model that chains the per-thread bodies of csrc/ntt_kernels.h exactly
as the kernel does (tests/native/ntt_test.cpp, the same templates) against a transform over Python integers; the same
program once more under the address and undefined-behaviour sanitizers; the Python argument checks; the exports and
the calls that need no device.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import ntt_util as N
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ntt_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "ntt_test")
EXE_ASAN = EXE + "_asan"
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "ntt_kernels.h", "ntt_plan.h", "scalar_kernels.h", "fp.h", "constants_gen.h")]
RUN_BYTES = 128   # the shortest run of a strided pass


def _build(exe, extra):
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + extra + ["-o", exe, SRC])


def _run(exe, lines):
    """request lines -> the answer lines"""
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-3000:]
    out = res.stdout.split("\n")
    assert len(out) >= len(lines)
    return out[:len(lines)]


def _hex(line):
    return [int(v, 16) for v in line.split()]


@pytest.fixture(scope="module")
def driver():
    _build(EXE, [])
    return lambda lines: _run(EXE, lines)


@pytest.fixture(scope="module")
def geometry(driver):
    return dict(zip(("pass_log", "run_log", "threads", "lds_words", "max_passes"), (int(v) for v in driver(["geometry"])[0].split())))


def _plan(driver, log_n):
    v = [int(x) for x in driver([f"plan {log_n}"])[0].split()]
    keys = ("s", "log_c", "log_t", "s_next", "first", "last")
    return {"n_passes": v[0], "tile_log": v[1], "split": v[2],
            "passes": [dict(zip(keys, v[3 + 6 * j:9 + 6 * j])) for j in range(v[0])]}


# ------------------------------------------------------------------------------------------------ constants
def test_two_adicities(driver):
    """Fr::TWO_ADICITY of the four fields is 47, 32, 32 and 1; each generator is a quadratic non-residue, which is what
    makes Fr::ROOT_MAX a root of order exactly 2^TWO_ADICITY"""
    consts = [_hex(line) for line in driver([f"{label} consts" for label in S.ALL])]
    assert [c[0] for c in consts] == [47, 32, 32, 1] == [N.two_adicity(label) for label in S.ALL]
    for label, (s, w) in zip(S.ALL, consts):
        q = S.order(label)
        assert pow(N.GENERATOR[label], (q - 1) // 2, q) == q - 1
        assert pow(w, 1 << (s - 1), q) == q - 1 and w == N.root_max(label)


@pytest.mark.parametrize("label", S.ALL)
def test_constants_match_python(driver, label):
    """Fr::TWO_ADICITY and Fr::ROOT_MAX; the default root at every legal log_n, by the host function the library uses; a
    longer transform is refused; fr_is_primitive_root accepts them and refuses their squares and 1"""
    q, s = S.order(label), N.two_adicity(label)
    assert _hex(driver([f"{label} consts"])[0]) == [s, N.root_max(label)]
    got = driver([f"{label} root {k}" for k in range(s + 2)])
    assert [int(v, 16) for v in got[:s + 1]] == [N.root(label, k) for k in range(s + 1)]
    assert got[s + 1] == "unsupported"
    logs = [k for k in (0, 1, 2, 5, 16, 31) if k <= s]
    roots = [N.root(label, k) for k in logs]
    assert driver([f"{label} primitive {k} {w:x}" for k, w in zip(logs, roots)]) == ["1"] * len(logs)
    bad = [(k, v) for k, w in zip(logs, roots) for v in ({1, w * w % q, 0, q - 1, 5} - ({w}))]
    bad = [(k, v) for k, v in bad if not (k and pow(v, 1 << (k - 1), q) == q - 1) and not (k == 0 and v == 1)]
    assert driver([f"{label} primitive {k} {v:x}" for k, v in bad]) == ["0"] * len(bad)


@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


@pytest.mark.parametrize("label", S.ALL)
def test_root_of_unity_entry_point(lib, label):
    """msmz_scalars_root_of_unity at every legal log_n, without a context; log_n > S is MSMZ_ERR_UNSUPPORTED and leaves
    the buffer alone"""
    s, cid = N.two_adicity(label), N.curve_id(label)
    for k in range(s + 1):
        buf = C.create_string_buffer(32)
        assert lib.msmz_scalars_root_of_unity(cid, k, buf) == 0
        assert int.from_bytes(buf.raw, "little") == N.root(label, k), k
    for k in (s + 1, 64, (1 << 32) - 1):
        buf = C.create_string_buffer(b"\xaa" * 32, 32)
        assert lib.msmz_scalars_root_of_unity(cid, k, buf) == 4
        assert buf.raw == b"\xaa" * 32
    assert lib.msmz_scalars_root_of_unity(cid, 0, None) == 1
    assert lib.msmz_scalars_root_of_unity(17, 0, C.create_string_buffer(32)) == 1


# ------------------------------------------------------------------------------------------------ the planner
def test_plan_at_every_length(driver, geometry):
    """log_n = 0 .. 32: the stages sum to log_n; a one-pass plan is within NTT_PASS_LOG and contiguous; every pass of a
    longer plan is strided, fills no more than a tile, has at least two stages and moves runs of at least 128 bytes on
    both sides; the pass count is the least the limits allow; the digits chain (log_t, s_next, first, last); the
    two-level split covers every exponent below n with O(sqrt n) entries"""
    limit, run_log = geometry["pass_log"], geometry["run_log"]
    assert 32 << run_log >= RUN_BYTES
    strided = limit - run_log
    for log_n in range(33):
        p = _plan(driver, log_n)
        ps = p["passes"]
        assert sum(x["s"] for x in ps) == log_n
        assert p["n_passes"] == (1 if log_n <= limit else -(-log_n // strided)) <= geometry["max_passes"]
        assert p["tile_log"] == max(x["s"] for x in ps)
        done = 0
        for j, x in enumerate(ps):
            assert x["log_t"] == done and x["first"] == (j == 0) and x["last"] == (j == len(ps) - 1)
            assert x["s_next"] == (ps[j + 1]["s"] if j + 1 < len(ps) else 0)
            assert x["s"] + x["log_c"] <= limit
            if len(ps) == 1:
                assert x["log_c"] == 0 and x["s"] <= limit
            else:
                assert 2 <= x["s"] <= strided
                assert 32 << x["log_c"] >= RUN_BYTES                 # runs of C entries on the reading side ...
                columns = log_n - x["s"] if j == 0 else done          # ... that are neighbours on the writing side too
                assert x["log_c"] <= columns
                assert x["s"] + x["log_c"] == limit                   # a full tile
            done += x["s"]
        assert p["split"] <= log_n and (1 << p["split"]) + (1 << (log_n - p["split"])) <= 3 << (log_n // 2)


def test_plan_entry_point(lib, driver, geometry):
    """msmz_test_ntt_plan and msmz_test_ntt_geometry == the planner the host driver was compiled with; no context"""
    v = C.c_uint32(0)
    lib.msmz_test_ntt_geometry(C.byref(v))
    assert v.value == geometry["pass_log"]
    lib.msmz_test_ntt_geometry(None)
    for log_n in range(33):
        st, stages = N.plan(lib, 0, log_n)
        assert st == 0 and stages == [x["s"] for x in _plan(driver, log_n)["passes"]]
    assert N.plan(lib, 0, 33)[0] == 1 and N.plan(lib, 9, 3)[0] == 1
    assert N.plan(lib, 1, 32)[0] == 0 and N.plan(lib, 3, 1) == (0, [1]) and N.plan(lib, 3, 2)[0] == 4
    n = C.c_uint32(0)
    assert lib.msmz_test_ntt_plan(0, 3, None, (C.c_uint32 * 8)()) == 1 and lib.msmz_test_ntt_plan(0, 3, C.byref(n), None) == 1


def test_ranges_clash(driver):
    """ranges of different lengths: one range exactly is no clash, apart is none, anything between is one"""
    cases = [((5, 4, 5, 4), 0), ((5, 4, 9, 4), 0), ((9, 4, 5, 4), 0), ((5, 4, 8, 4), 1), ((8, 4, 5, 4), 1), ((5, 4, 5, 8), 1),
             ((5, 8, 5, 4), 1), ((5, 2, 6, 8), 1), ((6, 8, 5, 2), 1), ((5, 1, 6, 8), 0), ((6, 8, 5, 1), 0), ((0, 1, 0, 1), 0),
             ((2 ** 64 - 2, 1, 0, 5), 0), ((0, 5, 2 ** 64 - 2, 1), 0), ((2 ** 63, 2 ** 63 - 1, 2 ** 63 + 5, 1), 1)]
    got = driver([f"clash {a} {na} {b} {nb}" for (a, na, b, nb), _ in cases])
    assert [int(v) for v in got] == [want for _, want in cases]


def test_lds_bank_conflicts_of_every_plan(driver, geometry):
    """For every pass shape of every plan, log_n = 0 .. 32: the LDS slots that the kernel's own thread bodies touch,
    instruction by instruction, put at most 2 distinct slots of a group of 32 lanes on one of the 32 banks (the bound
    DESIGN.md section 20 states); and tools/ntt_lds_model.py, which derives that table, replays exactly these slots"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ntt_lds_model", os.path.join(ROOT, "tools", "ntt_lds_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    pad = (geometry["lds_words"] - (1 << geometry["pass_log"])) * 32 >> geometry["pass_log"]
    slot = lambda p: p + (p >> 5) * pad
    assert slot((1 << geometry["pass_log"]) - 1) < geometry["lds_words"] and model.THREADS == geometry["threads"]
    shapes = sorted({(x["s"], x["log_c"], min(x["log_t"], 1)) for k in range(33) for x in _plan(driver, k)["passes"]})
    assert len(shapes) >= 15
    traces = driver([f"lds {s} {c} {t}" for s, c, t in shapes])
    for shape, line in zip(shapes, traces):
        groups = [[int(v) for v in g.split()] for g in line.split("|")]
        assert all(len(g) == geometry["threads"] for g in groups)
        for g in groups:
            for lane0 in range(0, len(g), 32):
                banks = {}
                for sl in {v for v in g[lane0:lane0 + 32] if v >= 0}:
                    banks[sl % 32] = banks.get(sl % 32, 0) + 1
                assert max(banks.values(), default=0) <= 2, (shape, lane0)
        replay = {tuple(-1 if p is None else slot(p) for p in pos) for _, pos in model.instructions(*shape)}
        assert replay == {tuple(g) for g in groups}, shape
    assert max(model.worst(slot, shapes).values()) <= 2


@pytest.mark.parametrize("label,log_n", [("bls12-377", 0), ("bls12-377", 7), ("bls12-377", 12), ("bls12-377", 25), ("pallas", 32),
                                         ("bls12-381", 19), ("ed-on-bls12-377", 1)])
def test_two_level_split_reproduces_the_powers(driver, label, log_n):
    """w^e = low[e mod 2^h] * high[e div 2^h] for e = 0, 1, the edges of the split, n - 1 and random exponents"""
    q, n = S.order(label), 1 << log_n
    w = N.root(label, log_n)
    h = _plan(driver, log_n)["split"]
    rng = random.Random(log_n)
    es = sorted({e for e in (0, 1, (1 << h) - 1, 1 << h, (1 << h) + 1, n // 2, n - 1) if e < n} | {rng.randrange(n) for _ in range(8)})
    got = _hex(driver([f"{label} tw {log_n} {len(es)} " + " ".join(f"{e:x}" for e in es)])[0])
    assert got == [pow(w, e, q) for e in es]


# ------------------------------------------------------------------------------------------------ the host model
def _line(label, log_n, flags, count, n_in, shift, xs):
    return f"{label} ntt {log_n} {flags} {count} {n_in} {shift:x} " + " ".join(f"{v:x}" for v in xs)


def _cases(label, log_n, seed):
    """(flags, count, n_in, shift): forward, inverse, both on a coset, a batch, and short inputs"""
    q, n = S.order(label), 1 << log_n
    g = random.Random(seed).randrange(2, q)
    cases = [(0, 1, n, 0), (N.INVERSE, 1, n, 0), (N.COSET, 2, n, g), (N.INVERSE | N.COSET, 1, n, g)]
    if n > 1:
        cases += [(0, 2, max(1, n // 4), 0), (N.COSET, 1, n // 2 + 1, q - 1)]
    return cases


def _model_matches(driver, label, log_ns):
    q = S.order(label)
    lines, want = [], []
    for log_n in log_ns:
        n, w = 1 << log_n, N.root(label, log_n)
        for flags, count, n_in, shift in _cases(label, log_n, log_n):
            xs = N.inputs(label, count * n_in, 7 * log_n + flags)
            lines.append(_line(label, log_n, flags, count, n_in, shift, xs))
            out = []
            for k in range(count):
                out += N.transform(q, xs[k * n_in:(k + 1) * n_in], n, w, bool(flags & N.INVERSE), shift if flags & N.COSET else None)
            want.append(out)
    got = [_hex(line) for line in driver(lines)]
    bad = [(line[:40], g[:2], v[:2]) for line, g, v in zip(lines, got, want) if g != v]
    assert not bad, bad[:3]


def test_host_model_every_size_up_to_4096(driver):
    """BLS12-377, log_n = 0 .. 12: the chained pass bodies give the Python-integer transform -- forward, inverse, coset,
    batches and n_in < n; from 2^11 on the plan has two passes"""
    _model_matches(driver, "bls12-377", range(13))
    assert _plan(driver, 12)["n_passes"] == 2


@pytest.mark.parametrize("label", ["pallas", "bls12-381"])
def test_host_model_other_fields(driver, geometry, label):
    """0, 1 and the first two-pass size"""
    _model_matches(driver, label, [0, 1, geometry["pass_log"] + 1])


def test_host_model_twisted_edwards_field(driver):
    """ed-on-bls12-377 has transforms of length 1 and 2 and no other"""
    label = "ed-on-bls12-377"
    _model_matches(driver, label, [0, 1])
    assert driver([_line(label, 2, 0, 1, 4, 0, [1, 2, 3, 4])]) == ["unsupported"]


def test_host_model_three_passes(driver, geometry):
    """the smallest three-pass size, forward on a coset and back: the round trip is exact and entry k is <x, (g w^k)^i>
    at a few k"""
    label = "bls12-377"
    q = S.order(label)
    log_n = next(k for k in range(33) if _plan(driver, k)["n_passes"] == 3)
    assert log_n <= 22
    n, w, g = 1 << log_n, N.root(label, log_n), 3
    xs = S.random_below_2_250(n, random.Random(3))
    ys = _hex(driver([_line(label, log_n, N.COSET, 1, n, g, xs)])[0])
    for k in (0, 1, n // 2 + 1, n - 1):
        b, acc = g * pow(w, k, q) % q, 0
        for v in reversed(xs):
            acc = (acc * b + v) % q
        assert ys[k] == acc, k
    assert _hex(driver([_line(label, log_n, N.INVERSE | N.COSET, 1, n, g, ys)])[0]) == xs


def test_model_flags_a_record_out_of_range(driver):
    """the first pass flags a record >= q; behind n_in nothing is read"""
    label = "bls12-377"
    q = S.order(label)
    assert driver([_line(label, 3, 0, 1, 8, 0, [1, 2, q, 4, 5, 6, 7, 8])]) == ["range"]
    assert driver([_line(label, 3, 0, 1, 8, 0, [1, 2, (1 << 256) - 1, 4, 5, 6, 7, 8])]) == ["range"]


def test_sanitizer_build_runs_clean(driver, geometry):
    """the same stand-alone program built with -fsanitize=address,undefined, run as a process of its own on requests of
    every kind: it exits 0, writes nothing to stderr, and answers as the plain build does"""
    _build(EXE_ASAN, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    lines = ["geometry", "clash 5 4 8 4", "lds 5 5 1", "lds 3 0 0"] + [f"plan {k}" for k in (0, 10, 11, 32)]
    for label in S.ALL:
        q = S.order(label)
        lines += [f"{label} consts", f"{label} root 1", f"{label} root 40", f"{label} primitive 1 {q - 1:x}", f"{label} tw 1 2 0 1"]
        for log_n in (0, 1):
            for flags, count, n_in, shift in _cases(label, log_n, 1):
                lines.append(_line(label, log_n, flags, count, n_in, shift, N.inputs(label, count * n_in, 1)))
    for log_n in (2, 5, geometry["pass_log"], geometry["pass_log"] + 1, geometry["pass_log"] + 3):
        for flags, count, n_in, shift in _cases("pallas", log_n, 2):
            lines.append(_line("pallas", log_n, flags, count, n_in, shift, N.inputs("pallas", count * n_in, 2)))
    lines.append(f"bls12-381 tw 20 3 0 fffff 12345")
    assert _run(EXE_ASAN, lines) == driver(lines)


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=4096, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


def _args(x, logN, inverse=False, shift=None, root=None, nIn=None, count=1, first=0, out=None, firstOut=0, q=1009):
    from msm_zprize_amd.parallel import ntt_args
    return ntt_args(x, logN, inverse, shift, root, nIn, count, first, out, firstOut, q)


def test_ntt_args_accepts():
    x, y = _arr(4096, 1), _arr(5000, 2)
    t = _args(x, 12)
    assert t == {"logN": 12, "flags": 0, "nIn": 4096, "count": 1, "first": 0, "firstOut": 0, "root": None, "shift": None}
    t = _args(x, 10, inverse=True, shift=5, root=7, count=4)
    assert (t["flags"], t["count"], t["root"], t["shift"]) == (3, 4, (7).to_bytes(32, "little"), (5).to_bytes(32, "little"))
    assert _args(x, 10, nIn=100, count=40, first=96)["nIn"] == 100
    assert _args(x, 11, first=0, out=x, firstOut=0)["firstOut"] == 0            # in place
    assert _args(x, 11, first=0, out=x, firstOut=2048)["firstOut"] == 2048      # apart in one handle
    assert _args(x, 11, nIn=1024, first=0, out=x, firstOut=1024)["nIn"] == 1024
    assert _args(x, 12, out=y, firstOut=904)["firstOut"] == 904
    assert _args(x, 0, count=4096)["count"] == 4096 and _args(_arr((1 << 32) - 1), 31)["logN"] == 31


def test_ntt_args_refuses():
    x, y = _arr(4096, 1), _arr(5000, 2)
    for bad in (_arr(100, 4, "points"), None, 7, b"x"):
        with pytest.raises(TypeError):
            _args(bad, 3)
        if bad is not None:
            with pytest.raises(TypeError):
                _args(x, 3, out=bad)
    for name in ("shift", "root"):
        for bad in (1.0, "1", True, b"\x01"):
            with pytest.raises(TypeError):
                _args(x, 3, **{name: bad})
        for bad in (1009, -1, 1 << 256):
            with pytest.raises(ValueError):
                _args(x, 3, **{name: bad})
    with pytest.raises(TypeError):
        _args(x, 3, inverse=1)
    for kw in (dict(shift=0), dict(logN=-1), dict(logN=32), dict(logN=True), dict(logN=1.0), dict(logN=13), dict(count=0),
               dict(count=True), dict(logN=12, count=2), dict(logN=20, count=1 << 12), dict(nIn=0), dict(nIn=9), dict(nIn=-1),
               dict(nIn=4, inverse=True), dict(first=-1), dict(first=4089), dict(first=True), dict(firstOut=1),
               dict(out=y, firstOut=4993), dict(out=y, firstOut=-1), dict(logN=11, out=x, firstOut=1), dict(logN=11, first=1, out=x),
               dict(logN=11, out=x, firstOut=2047), dict(logN=11, nIn=1024, out=x), dict(logN=11, nIn=1024, first=5, out=x),
               dict(logN=11, nIn=1024, out=_arr(4096, 1), firstOut=1023)):
        args = dict(logN=3)
        args.update(kw)
        with pytest.raises(ValueError):
            _args(x, **args)


# ------------------------------------------------------------------------------------------------ the library
def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in ("msmz_scalars_ntt", "msmz_scalars_root_of_unity", "msmz_test_ntt_plan", "msmz_test_ntt_geometry"):
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    from msm_zprize_amd.parallel import _Parallel
    for name in ("ntt", "rootOfUnity"):
        assert callable(getattr(_Parallel, name))
    assert C.sizeof(_native.MsmzNtt) == 56
    assert (_native.MSMZ_NTT_INVERSE, _native.MSMZ_NTT_COSET) == (1, 2)


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG and the handle untouched"""
    from msm_zprize_amd import _native
    t = _native.MsmzNtt(1, 0, 3, 0, 0, 1, None, None)
    h = C.c_uint64(77)
    assert lib.msmz_scalars_ntt(None, C.byref(t), 0, C.byref(h)) == 1
    assert h.value == 77


def test_cache_hooks_need_no_device(lib):
    """msmz_test_cache_geometry answers without a context, every pointer nullable; msmz_test_ntt_tables without a context
    or a counter is MSMZ_ERR_ARG and writes nothing.  (What the values mean is held by the GPU tests that fill the caches
    and the grid past them.)"""
    from msm_zprize_amd import _native
    for name in ("msmz_test_cache_geometry", "msmz_test_ntt_tables"):
        assert name in _native.EXPORTS and getattr(lib, name) is not None
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lib.msmz_test_cache_geometry(C.byref(a), C.byref(b), C.byref(c))
    lib.msmz_test_cache_geometry(None, None, None)
    assert a.value >= 2 and b.value >= 3 and 1 <= c.value <= 65535   # (grid.y of a launch has 16 bits)
    built = C.c_uint64(5)
    assert lib.msmz_test_ntt_tables(None, C.byref(built)) == 1 and built.value == 5
    assert lib.msmz_test_ntt_tables(None, None) == 1
