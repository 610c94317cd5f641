"""The sumcheck step without a GPU: the step bodies of csrc/mle_kernels.h compiled for the CPU
(tests/native/sumcheck_step_test.cpp: fr_sc_step, one thread's work for one new pair index, and fr_sc_last, the step of
one-variable tables) against Python integers (tests/sumcheck_step_util.py), the same program under
-fsanitize=address,undefined over the same requests; the Python argument checks of sumcheckStep and the host loop of
sumcheckProve on a library that is a Python model; the export, the descriptor's layout and the null context.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import mle_util as M
import scalar_ops_util as S
import sumcheck_step_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sumcheck_step_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "sumcheck_step_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")


def _build(exe, flags=("-O2",)):
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "mle_kernels.h", "scalar_kernels.h", "sqrt.h", "fp.h", "constants_gen.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", *flags, "-std=c++17", "-o", exe, SRC])


def _run(exe, lines):
    """request lines -> one list of ints per answer line"""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(lines)
    return [[int(v, 16) for v in line.split()] for line in out[:len(lines)]]


def _geometry():
    _build(EXE)
    return [int(v) for v in subprocess.run([EXE], input="geometry\n", capture_output=True, text=True, check=True).stdout.split()]


def _terms_words(terms):
    return " ".join(f"{m:x} " + ("-" if c is None else f"{c:x}") for c, m in terms)


def _requests(label):
    """(request line, wanted answer) for one curve: every table count, the mask sets of the round test, coefficients over
    {NULL, 0, q - 1, random}, both orders, r over {0, 1, q - 1, random}: tables of 8 entries (two new pair indices) for
    the step, of 2 entries for the last step"""
    q = S.order(label)
    rng = random.Random(S.ALL.index(label) + 3000)
    rows = S.planted_pairs(q, rng)
    case = 0
    for nt in range(1, 7):
        for masks in M.mask_sets(nt, 4):
            for coeffs in ([None] * 2, [0, q - 1], [q - 1, rng.randrange(2, q)], [rng.randrange(2, q), None]):
                terms = list(zip(coeffs, masks))
                for low in (False, True):
                    case += 1
                    r = (0, 1, q - 1, rng.randrange(2, q))[case % 4]
                    tables = []
                    for j in range(nt):   # planted rows where the order puts a bound pair, random values elsewhere
                        t = [rng.randrange(q) for _ in range(8)]
                        if (j + case) % 2:
                            lo, hi = rows[(7 * j + case) % len(rows)]
                            t[1 if low else 0], t[(1 if low else 0) + (1 if low else 4)] = lo, hi
                        tables.append(t)
                    at = (lambda i: (4 * i, 4 * i + 1, 4 * i + 2, 4 * i + 3)) if low else (lambda i: (i, i + 4, i + 2, i + 6))
                    to = (lambda i: (2 * i, 2 * i + 1)) if low else (lambda i: (i, i + 2))
                    bound, degree, values = U.step(tables, terms, r, q, low)
                    words = " ".join(f"{tables[j][k]:x}" for i in range(2) for j in range(nt) for k in at(i))
                    want = values + [bound[j][k] for i in range(2) for j in range(nt) for k in to(i)]
                    assert degree == max(bin(m).count("1") for m in masks)
                    yield f"{label} step {nt} 2 {len(terms)} {r:x} {words} {_terms_words(terms)}", want
                    # the last step: tables of one variable
                    ones = [t[:2] for t in tables]
                    bound, degree, values = U.step(ones, terms, r, q, low)
                    assert degree == 0 and len(values) == 1
                    words = " ".join(f"{t[0]:x} {t[1]:x}" for t in ones)
                    yield f"{label} last {nt} {len(terms)} {r:x} {words} {_terms_words(terms)}", values * 2 + [b[0] for b in bound]


@pytest.mark.parametrize("label", S.ALL)
def test_step_bodies(label):
    """fr_sc_step over two new pair indices == bind then round of the model, values and stored entries, for every table
    count 1 .. 6, both orders, the mask sets of the round test and coefficients NULL, 0, q - 1, random; with tables of one
    variable fr_sc_step on hi = lo at degree 0 == fr_sc_last == the terms over the bound entries"""
    _build(EXE)
    lines, want = zip(*_requests(label))
    got = _run(EXE, lines)
    bad = [(line[:70], g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:2]
    assert len(lines) > 200 and any(" last 6 " in l for l in lines) and any(" step 6 " in l for l in lines)


def test_sanitized_driver_runs_clean():
    """sumcheck_step_test.cpp as a stand-alone program with -fsanitize=address,undefined over the requests of the test
    above on two curves, and the malformed ones: exit 0, nothing on stderr, the same answers"""
    _build(EXE)
    exe = EXE + "_asan"
    _build(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    lines = ["geometry", "nocurve step", "pallas what", "pallas step 7 1 1 0", "pallas step 1 1 9 0 1 2 3 4"]
    lines += [l for label in ("bls12-377", "pallas") for l, _ in _requests(label)]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout


def test_model_is_consistent():
    """the Python model against itself: every g_k(0) + g_k(1) is g_(k-1)(r_(k-1)), the first is the sum, and the claim is
    the terms over the tables evaluated at the challenges, in both orders"""
    q = S.order("pallas")
    rng = random.Random(7)
    v = 4
    tables = [[rng.randrange(q) for _ in range(1 << v)] for _ in range(3)]
    terms = U.mixed_terms(3, q, rng)
    for low in (False, True):
        polys, rs, claim, final = U.prove(tables, terms, q, lambda vals: rng.randrange(q), low)
        assert len(polys) == len(rs) == v and [len(f) for f in final] == [1, 1, 1]
        assert (polys[0][0] + polys[0][1]) % q == sum(U.claim([[f[i]] for f in tables], terms, q) for i in range(1 << v)) % q
        for k in range(1, v):
            assert (polys[k][0] + polys[k][1]) % q == M.interpolate(polys[k - 1], rs[k - 1], q)
        assert claim == M.interpolate(polys[-1], rs[-1], q) == U.claim(final, terms, q)
        point = rs if low else rs[::-1]   # variable 0 first
        assert [f[0] for f in final] == [M.mle_eval(f, point, q) for f in tables]


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=64, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


Q = 1009


def _step(tables, terms=((None, 1),), nVars=None, r=5, out=None, low=False):
    from msm_zprize_amd.parallel import sumcheck_step_args
    return sumcheck_step_args(tables, list(terms), nVars, r, out, low, Q)


def test_sumcheck_step_args():
    f, g, d = _arr(64, 1), _arr(100, 2), _arr(64, 3)
    a = _step([f, (g, 36)], [(None, 0b11), (Q - 1, 0b10)], out=[d, (g, 4)])
    assert (a["nVars"], a["degree"], a["flags"], a["r"]) == (6, 2, 0, (5).to_bytes(32, "little"))
    assert a["tables"] == [(f, 0), (g, 36)] and a["out"] == [(d, 0), (g, 4)]
    assert _step([f])["out"] is None                                              # in place
    assert _step([(f, 0)], nVars=5, out=[(f, 0)])["out"] == [(f, 0)]              # the low half, said aloud
    assert _step([(f, 16)], nVars=4, out=[(f, 0)])["nVars"] == 4                  # apart, ending where the source begins
    assert _step([(f, 16)], nVars=4, out=[(f, 32)])["nVars"] == 4                 # apart, beginning where it ends
    assert _step([f, f], [(1, 3)], out=[d, (g, 0)], low=True)["flags"] == 1       # one range twice, destinations apart
    assert _step([(f, 0), (f, 32)], nVars=5)["out"] is None                       # two tables of one array, each in place
    assert _step([(f, 2)], nVars=1)["degree"] == 0 and _step([f], [(1, 1)], 1, out=[(d, 63)])["degree"] == 0
    assert _step([f] * 1, r=0)["r"] == bytes(32) and _step([f], r=Q - 1)["r"] == (Q - 1).to_bytes(32, "little")
    for kw in (dict(r=None), dict(r=1.5), dict(r=True), dict(r=b"\x01"), dict(out=7), dict(out=d), dict(out=[7]),
               dict(out=[_arr(64, 4, "points")]), dict(out=[(d, 0, 0)]), dict(low=1)):
        with pytest.raises(TypeError):
            _step([f], **kw)
    for tables, terms in ((None, [(1, 1)]), ([7], [(1, 1)]), ([f], [(1.5, 1)]), ([f], [1])):     # sumcheckRound's own
        with pytest.raises(TypeError):
            _step(tables, terms)
    for tables, kw in (([f], dict(r=Q)), ([f], dict(r=-1)), ([f], dict(out=[])), ([f], dict(out=[d, d])),
                       ([f, f], dict(out=[d])), ([f], dict(out=[(d, 33)])), ([f], dict(out=[(d, -1)])),
                       ([f], dict(out=[(g, 69)])), ([f], dict(nVars=0)), ([f], dict(nVars=7)), ([g], dict()),
                       ([f], dict(terms=[(1, 2)])), ([f], dict(terms=[(Q, 1)])), ([], dict()),
                       ([f], dict(out=[(f, 32)])),                                  # the high half
                       ([f], dict(out=[(f, 1)])), ([f], dict(out=[(f, 31)])),       # partial overlaps with the low half
                       ([(f, 16)], dict(nVars=4, out=[(f, 9)])), ([(f, 16)], dict(nVars=4, out=[(f, 24)])),
                       ([(f, 16)], dict(nVars=4, out=[(f, 31)])),
                       ([f], dict(low=True)), ([f], dict(low=True, out=[f])),       # the low order in place
                       ([(f, 16)], dict(nVars=4, low=True, out=[(f, 16)])),
                       ([f, f], dict(terms=[(1, 3)])),                              # in place on another table's source
                       ([f, d], dict(out=[(d, 0), (g, 0)])), ([f, d], dict(out=[(g, 0), (f, 0)])),
                       ([(f, 0), (f, 16)], dict(nVars=5)),                          # overlapping sources, in place
                       ([f, d], dict(out=[(g, 0), (g, 31)])), ([f, d], dict(out=[g, g])),   # two destinations overlap
                       ([f, d, g], dict(nVars=6, out=[(g, 64), (g, 0), (d, 0)]))):  # ... on a source, and each other
        with pytest.raises(ValueError):
            _step(tables, **kw)
    same = _arr(64, 1)   # another object for the same handle overlaps all the same
    with pytest.raises(ValueError):
        _step([f], out=[(same, 3)])


class _ModelLib:
    """stands in for the loaded library: resident scalar sets as Python lists, the two sumcheck calls by the integer
    model, alloc and free; counts its calls"""

    def __init__(self, q):
        self.q, self.sets, self.next, self.calls = q, {}, 1, []

    def add(self, values):
        self.sets[self.next] = list(values)
        self.next += 1
        return self.next - 1

    @staticmethod
    def _value(st, field):
        """the 32-byte value a pointer field of a descriptor points at, as an int, or None (a c_char_p read stops at a 0)"""
        addr = C.c_void_p.from_buffer(st, getattr(type(st), field).offset).value
        return None if addr is None else int.from_bytes(C.string_at(addr, 32), "little")

    def _terms(self, s):
        return [(self._value(s.terms[k], "coeff"), s.terms[k].mask) for k in range(s.n_terms)]

    def _put(self, values, degree, buf):
        degree._obj.value = len(values) - 1
        C.memmove(buf, b"".join(v.to_bytes(32, "little") for v in values), 32 * len(values))
        return 0

    def msmz_alloc_scalars(self, ctx, n, h):
        self.calls.append("alloc")
        h._obj.value = self.add([None] * n)
        return 0

    def msmz_free(self, ctx, h):
        self.calls.append("free")
        del self.sets[h]
        return 0

    def msmz_scalars_sumcheck_round(self, ctx, s, degree, buf):
        s = s._obj
        self.calls.append("round")
        tabs = [self.sets[s.tables[j].handle][s.tables[j].first:][:1 << s.n_vars] for j in range(s.n_tables)]
        return self._put(M.round_poly(tabs, self._terms(s), self.q, bool(s.flags)), degree, buf)

    def msmz_scalars_sumcheck_step(self, ctx, s, degree, buf):
        s = s._obj
        self.calls.append("step")
        tabs = [self.sets[s.tables[j].handle][s.tables[j].first:][:1 << s.n_vars] for j in range(s.n_tables)]
        assert all(v is not None for t in tabs for v in t), "a step read entries nothing had written"
        r = self._value(s, "r")
        bound, _, values = U.step(tabs, self._terms(s), r, self.q, bool(s.flags))
        dst = s.out if s.out else s.tables
        for j, b in enumerate(bound):
            self.sets[dst[j].handle][dst[j].first:dst[j].first + len(b)] = b
        return self._put(values, degree, buf)


class _Curve:
    _ctx = "ctx"

    def __init__(self, q):
        self.params = {"order": q}


@pytest.mark.parametrize("low", (False, True))
def test_sumcheck_prove_is_a_host_loop(monkeypatch, low):
    """sumcheckProve on a library that is the integer model: one round and nVars steps, in place in the high order and
    between the tables and one scratch array per table in the low order, every scratch array freed; polynomials,
    challenges and claim are those of the model's two-call prover; the challenge function sees each round's values"""
    from msm_zprize_amd import parallel
    q = S.order("bls12-381")
    rng = random.Random(11)
    lib = _ModelLib(q)
    monkeypatch.setattr(parallel, "lib", lambda: lib)
    curve = _Curve(q)
    v = 5
    data = [[rng.randrange(q) for _ in range((1 << v) + 3)] for _ in range(3)]
    arrays = [parallel.DeviceArray(curve, lib.add(d), len(d), "scalars") for d in data]
    tables = [arrays[0], (arrays[1], 3), (arrays[2], 1)]
    terms = U.mixed_terms(3, q, rng)
    seen = []

    def challenge(values):
        seen.append(values)
        return (sum(values) * 31 + len(seen)) % q

    polys, rs, claim = parallel._Parallel(curve).sumcheckProve(tables, terms, v, challenge, low=low)
    seen_by_device, seen = seen, []
    want = U.prove([data[0][:1 << v], data[1][3:3 + (1 << v)], data[2][1:1 + (1 << v)]], terms, q, challenge, low)
    assert (polys, rs, claim) == want[:3] and seen_by_device == seen == polys
    assert lib.calls.count("round") == 1 and lib.calls.count("step") == v
    assert lib.calls.count("alloc") == lib.calls.count("free") == (3 if low else 0) and len(lib.sets) == 3
    assert [len(lib.sets[a.handle]) for a in arrays] == [len(d) for d in data]
    assert lib.sets[arrays[1].handle][:3] == data[1][:3]            # entries in front of a table stay
    par = parallel._Parallel(curve)
    before = len(lib.calls)
    with pytest.raises(TypeError):
        par.sumcheckProve(tables, terms, v, None, low=low)
    with pytest.raises(TypeError):
        par.sumcheckProve(tables, terms, v, challenge, low=1)
    with pytest.raises(ValueError):
        par.sumcheckProve(tables, terms, v + 1, challenge, low=low)
    with pytest.raises(ValueError):
        par.sumcheckStep(tables, terms, v, q)
    assert len(lib.calls) == before                                   # refused before the library is reached
    with pytest.raises(ValueError):                                   # a challenge out of range: the step refuses it
        par.sumcheckProve(tables, terms, 2, lambda values: q, low=low)
    assert lib.calls.count("alloc") == lib.calls.count("free")        # ... and the scratch arrays are freed all the same


def test_sumcheck_step_reaches_the_library(monkeypatch):
    """sumcheckStep hands the library the descriptor its arguments describe and returns (degree, values)"""
    from msm_zprize_amd import parallel
    q = S.order("pallas")
    rng = random.Random(12)
    lib = _ModelLib(q)
    monkeypatch.setattr(parallel, "lib", lambda: lib)
    curve = _Curve(q)
    data = [[rng.randrange(q) for _ in range(16)] for _ in range(2)]
    f, g = (parallel.DeviceArray(curve, lib.add(d), 16, "scalars") for d in data)
    out = parallel.DeviceArray(curve, lib.add([None] * 16), 16, "scalars")
    terms = [(3, 0b11), (None, 0b10)]
    r = rng.randrange(q)
    got = parallel._Parallel(curve).sumcheckStep([f, (g, 8)], terms, 3, r, out=[out, (out, 12)], low=True)
    bound, degree, values = U.step([data[0][:8], data[1][8:]], terms, r, q, True)
    assert got == (degree, values) == (2, values)
    assert lib.sets[out.handle] == bound[0] + [None] * 8 + bound[1] and lib.sets[f.handle] == data[0]
    got = parallel._Parallel(curve).sumcheckStep([(f, 4)], [(None, 1)], 1, r)      # the last step, in place
    assert got == (0, [(data[0][4] + r * (data[0][5] - data[0][4])) % q]) and lib.sets[f.handle][4] == got[1][0]


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in ("msmz_scalars_sumcheck_step", "msmz_test_sumcheck_step_geometry"):
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    assert C.sizeof(_native.MsmzSumcheckStep) == 48
    header = open(os.path.join(ROOT, "include", "msmz.h")).read()
    assert "int msmz_scalars_sumcheck_step(msmz_ctx* ctx, const msmz_sumcheck_step* s, uint32_t* degree, uint8_t* evals_le32);" in header


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof and the offset of every field of msmz_sumcheck_step, C side == ctypes side"""
    from msm_zprize_amd import _native as N
    prints, want = ['printf("%zu ", sizeof(msmz_sumcheck_step));'], [C.sizeof(N.MsmzSumcheckStep)]
    for fname, _ in N.MsmzSumcheckStep._fields_:
        prints.append(f'printf("%zu ", offsetof(msmz_sumcheck_step, {fname}));')
        want.append(getattr(N.MsmzSumcheckStep, fname).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msmz.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()] == want
    assert want == [48, 0, 8, 16, 20, 24, 32, 36, 40]


def test_geometry_accessor(lib):
    """msmz_test_sumcheck_step_geometry == the constant the host driver was compiled with == the round's tile; needs no
    context"""
    t, rt = C.c_uint32(0), C.c_uint32(0)
    lib.msmz_test_sumcheck_step_geometry(C.byref(t))
    lib.msmz_test_mle_geometry(None, None, C.byref(rt))
    tile, max_tables, max_degree, max_terms, fused = _geometry()
    assert t.value == tile == rt.value and tile & (tile - 1) == 0
    assert (max_tables, max_degree, max_terms) == (6, 4, 8) and 1 <= fused <= max_tables
    lib.msmz_test_sumcheck_step_geometry(None)


def test_null_context_is_a_bad_argument(lib):
    """no context, no device -> MSMZ_ERR_ARG and the outputs untouched"""
    from msm_zprize_amd import _native as N
    one = (1).to_bytes(32, "little")
    tabs = (N.MsmzSumcheckTable * 1)(N.MsmzSumcheckTable(1, 0))
    terms = (N.MsmzSumcheckTerm * 1)(N.MsmzSumcheckTerm(None, 1))
    s = N.MsmzSumcheckStep(tabs, None, 1, 1, terms, 1, 0, one)
    d = C.c_uint32(9)
    ev = C.create_string_buffer(b"\xaa" * 160, 160)
    assert lib.msmz_scalars_sumcheck_step(None, C.byref(s), C.byref(d), ev) == 1
    assert d.value == 9 and ev.raw == b"\xaa" * 160
