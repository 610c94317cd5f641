"""Lookup multiplicities without a GPU: the host-callable part of csrc/lookup_kernels.h compiled for the CPU
(tests/native/lookup_test.cpp, the same templates the kernels instantiate, a sequential policy in place of the device
atomics) against Python integers (tests/lookup_util.py) -- the spread of the hash, the host hook against the driver, and
insert / count / emit with the threads of every launch in forward, reverse and shuffled order; the descriptor layouts,
the exports, null arguments and the Python argument checks.  The driver is also built with the address and
undefined-behaviour sanitizers as a stand-alone program and run over the same requests.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import pytest

import lookup_util as L
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "lookup_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "lookup_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("fr.h", "lookup_kernels.h", "fp.h", "constants_gen.h")]
CURVE_ID = {"bls12-377": 0, "pallas": 1, "bls12-381": 2, "ed-on-bls12-377": 3}
ORDERS = ("fwd", "rev", "shuf")


def _build(exe, extra=()):
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, "-o", exe, SRC])


def _ask(exe, lines):
    """request lines -> the answer lines, as lists of words"""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(lines)
    return [line.split() for line in out[:len(lines)]]


@pytest.fixture(scope="module")
def driver():
    _build(EXE)
    return lambda lines: _ask(EXE, lines)


@pytest.fixture(scope="module")
def lib():
    import msm_zprize_amd.build as b
    from msm_zprize_amd import _native
    b.build(verbose=False)
    return _native.lib()


def _slot_of(lib, label, n):
    return lambda v: lib.msmz_test_lookup_slot(CURVE_ID[label], v.to_bytes(32, "little"), n)


def _hex(values):
    return " ".join(f"{v:x}" for v in values)


# ------------------------------------------------------------------------------------------------ the hash
# The bounds are those of a uniformly random hash at load 1/2, not of this one.  Linear probing: the longest run of
# occupied slots of n keys at load a concentrates at ln n / (a - 1 - ln a) (Pittel 1987), 43 for n = 4096, a = 1/2, and
# no walk is longer than the run it lies in; 64 leaves half of that again.  First slots: the keys per slot are
# Poisson(1/2), and 8192 slots see one with 9 or more with probability below 10^-4.  Seen: walks of 12 (0 .. 4095) and
# 23 (top word only) against 17 to 21 for five tables of random values; at most 6 and 4 keys on one first slot.
WALK_BOUND, SHARED_BOUND = 64, 8


@pytest.mark.parametrize("label", S.ALL)
def test_hash_spreads_small_integers_and_top_words(driver, label):
    """0 .. 4095 (only word 0 differs) and 4096 values that differ only in word 7, into 8192 slots each"""
    low = list(range(4096))
    top = [(k << 224) + 5 for k in range(4096)]
    assert max(top) < S.order(label)
    for name, got in zip(("low", "top"), driver([f"{label} chain 4096 {_hex(low)}", f"{label} chain 4096 {_hex(top)}"])):
        s, walk, shared = (int(w) for w in got)
        print(label, name, "slots", s, "longest walk", walk, "most keys on one first slot", shared)
        assert s == 8192
        assert walk <= WALK_BOUND and shared <= SHARED_BOUND, (name, walk, shared)


@pytest.mark.parametrize("label", S.ALL)
def test_slot_hook_agrees_with_the_driver(driver, lib, label):
    """msmz_test_lookup_slot == lk_first_slot as the driver compiled it, for edge and random values at table sizes on
    both sides of every power of two up to 2^30; needs no context"""
    q = S.order(label)
    rng = random.Random(11 + S.ALL.index(label))
    values = S.edge_values(q) + [rng.randrange(q) for _ in range(40)]
    sizes = [1, 2, 3, 4, 5, 64, 65, 4096, 4097, (1 << 30) - 1, 1 << 30]
    cases = [(v, n) for v in values for n in sizes]
    got = driver([f"{label} slot {v:x} {n}" for v, n in cases])
    for (v, n), words in zip(cases, got):
        slot = _slot_of(lib, label, n)(v)
        assert slot == int(words[0]) and slot < L.slots(n), (hex(v), n)
    assert [int(w[0]) for w in driver([f"slots {n}" for n in sizes])] == [L.slots(n) for n in sizes]
    assert L.slots(1 << 30) == 1 << 31


def test_slot_hook_refuses(lib):
    one = (1).to_bytes(32, "little")
    assert lib.msmz_test_lookup_slot(0, one, 5) < 16
    for curve, value, n in ((4, one, 5), (-1, one, 5), (0, None, 5), (0, one, 0), (0, one, (1 << 30) + 1),
                            (1, S.order("pallas").to_bytes(32, "little"), 5), (2, b"\xff" * 32, 5)):
        assert lib.msmz_test_lookup_slot(curve, value, n) == L.NONE, (curve, n)


def test_geometry(driver, lib):
    """msmz_test_lookup_geometry == the constants the driver was compiled with; needs no context"""
    s, w = C.c_uint32(0), C.c_uint32(0)
    lib.msmz_test_lookup_geometry(C.byref(s), C.byref(w))
    assert [[str(s.value), str(w.value)]] == driver(["geometry"])
    assert s.value == 2 and w.value % 64 == 0 and w.value >= 64
    lib.msmz_test_lookup_geometry(None, None)


def test_small_table_geometry(driver, lib):
    """msmz_test_lookup_small_table == the constants of the driver; a workgroup of k_lookup_count_small takes `passes`
    passes of W column entries until that would need more than `groups` workgroups"""
    p, g = C.c_uint32(0), C.c_uint32(0)
    small = lib.msmz_test_lookup_small_table(C.byref(p), C.byref(g))
    assert [[str(small), str(p.value), str(g.value)]] == driver(["small"])
    assert lib.msmz_test_lookup_small_table(None, None) == small
    W = int(driver(["geometry"])[0][1])
    assert 4 * small <= 64 * 1024            # the counts of a workgroup fit its LDS
    per = W * p.value
    sizes = [1, per - 1, per, per + 1, 7 * per, per * g.value - 1, per * g.value, per * g.value + 1, (1 << 32) - 1]
    got = [int(w[0]) for w in driver([f"groups {n}" for n in sizes])]
    assert got == [min(-(-n // per), g.value) for n in sizes] and got[0] == 1 and got[-1] == g.value


# ------------------------------------------------------------------------------------------------ the three kernels
def _run_line(label, order, seed, table, column, want_pos=True):
    return f"{label} run {order} {seed} {1 if want_pos else 0} {len(table)} {len(column)} {_hex(table)} {_hex(column)}"


def _parse(words, tn, cn, want_pos=True):
    m = [int(w, 16) for w in words[:tn]]
    pos = [int(w) for w in words[tn:tn + cn]] if want_pos else None
    err, missing, first, distinct = (int(w) for w in words[-4:])
    assert len(words) == tn + (cn if want_pos else 0) + 4
    return m, pos, err, {"missing": missing, "firstMissing": None if first == L.NONE else first, "distinct": distinct}


def _emulation_cases(lib, label, seed):
    q = S.order(label)
    rng = random.Random(seed)
    W = 256
    for n in (1, 2, 3, 64, 65):
        for tname, table in L.tables(n, q, rng, _slot_of(lib, label, n)).items():
            for cn in (1, 65, 2 * W + 9):
                for cname, column in L.columns(cn, table, q, rng, W).items():
                    yield (tname, n, cname, cn), table, column


@pytest.mark.parametrize("label", S.ALL)
def test_every_thread_order_gives_the_model(driver, lib, label):
    """tables: all distinct, 0 .. n - 1, all equal, every value twice, each value three times, the edge values as keys, all
    keys starting at one slot and at the last slot (wrap-around); sizes 1, 2, 3, 64, 65; columns: all present (uniform,
    constant, 63 of 64, runs), all missing, one and two missing -- insert, count and emit with the threads of each
    launch forward, reversed and shuffled: identical multiplicities, positions and result words, those of the model"""
    cases = list(_emulation_cases(lib, label, 70 + S.ALL.index(label)))
    if label not in ("bls12-377", "pallas"):
        cases = [c for c in cases if c[0][3] == 65]
    lines = [_run_line(label, order, 5 + k, t, c) for k, (_, t, c) in enumerate(cases) for order in ORDERS]
    got = driver(lines)
    for k, (ident, table, column) in enumerate(cases):
        want = L.model(table, column)
        for o, order in enumerate(ORDERS):
            m, pos, err, info = _parse(got[3 * k + o], len(table), len(column))
            assert (m, pos, err, info) == (want[0], want[1], 0, want[2]), (ident, order)


def test_without_positions_nothing_is_written(driver):
    q = S.order("pallas")
    rng = random.Random(3)
    table = L.distinct(65, q, rng)
    column = L.columns(300, table, q, rng)["missing_two"]
    words = driver([_run_line("pallas", "shuf", 9, table, column, want_pos=False)])[0]
    m, pos, err, info = _parse(words, 65, 300, want_pos=False)
    assert (m, err, info) == (L.model(table, column)[0], 0, L.model(table, column)[2])


@pytest.mark.parametrize("label", S.ALL)
def test_values_not_below_q_are_flagged(driver, label):
    """q and 2^256 - 1 as a table entry and as a column entry raise the error word; q - 1 and 0 are ordinary keys"""
    q = S.order(label)
    good = [5, q - 1, 0, 7]
    lines, want_err = [], []
    for bad in (q, (1 << 256) - 1):
        for order in ORDERS:
            lines += [_run_line(label, order, 1, [5, bad, 0, 7], [5, 0, 7]), _run_line(label, order, 1, good, [5, bad, 0]),
                      _run_line(label, order, 1, good, [q - 1, 0, 0, q - 1, 5])]
            want_err += [1, 1, 0]
    got = driver(lines)
    assert [int(w[-4]) for w in got] == want_err
    m, pos, err, info = _parse(got[2], 4, 5)
    assert (m, pos, info) == L.model(good, [q - 1, 0, 0, q - 1, 5]) and m == [1, 2, 2, 0]


def test_sanitized_driver_runs_clean(lib):
    """lookup_test.cpp as a stand-alone program with -fsanitize=address,undefined over requests of every kind: exit 0,
    nothing on stderr, the same answers"""
    _build(EXE)
    exe = EXE + "_asan"
    _build(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    label, q = "bls12-377", S.order("bls12-377")
    cases = [c for c in _emulation_cases(lib, label, 4) if c[0][1] in (1, 2, 65) and c[0][3] in (1, 65)]
    lines = ["geometry", "slots 3", "small", "groups 5000", f"{label} slot {q - 1:x} 65", f"{label} chain 300 {_hex(range(300))}",
             _run_line(label, "fwd", 1, [5, q, 0], [5, (1 << 256) - 1])]
    lines += [_run_line(label, ORDERS[k % 3], k, t, c, want_pos=k % 2 == 0) for k, (_, t, c) in enumerate(cases)]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout


# ------------------------------------------------------------------------------------------------ Python arguments
def _arr(n=64, handle=1, kind="scalars"):
    from msm_zprize_amd.parallel import DeviceArray
    return DeviceArray(None, handle, n, kind)


def _args(column, table, firstColumn=0, N=None, firstTable=0, tableN=None, out=None, firstOut=0, positions=False):
    from msm_zprize_amd.parallel import lookup_args
    return lookup_args(column, table, firstColumn, N, firstTable, tableN, out, firstOut, positions)


def test_lookup_args():
    f, t, o = _arr(64, 1), _arr(16, 2), _arr(40, 3)
    assert _args(f, t) == {"N": 64, "tableN": 16}
    assert _args(f, t, firstColumn=60, firstTable=15) == {"N": 4, "tableN": 1}
    assert _args(f, t, N=10, tableN=4, out=o, firstOut=36, positions=True) == {"N": 10, "tableN": 4}
    assert _args(f, f, firstColumn=8, N=20, firstTable=0, tableN=16) == {"N": 20, "tableN": 16}     # table and column overlap
    assert _args(f, f, firstColumn=8, N=8, firstTable=16, tableN=8, out=f, firstOut=0)["tableN"] == 8   # ends where f begins
    assert _args(f, f, firstColumn=8, N=8, firstTable=16, tableN=8, out=f, firstOut=24)["tableN"] == 8  # begins where t ends
    for args, kw in (((None, t), {}), ((f, None), {}), ((7, t), {}), ((_arr(64, 4, "points"), t), {}), ((f, _arr(64, 4, "points")), {}),
                     ((f, t), dict(out=7)), ((f, t), dict(out=_arr(64, 4, "points"))), ((f, t), dict(positions=1)),
                     ((f, t), dict(positions=None))):
        with pytest.raises(TypeError):
            _args(*args, **kw)
    same = _arr(64, 1)   # another object for the same handle overlaps all the same
    for kw in (dict(N=0), dict(tableN=0), dict(N=65), dict(tableN=17), dict(N=-1), dict(N=True), dict(N=1.0), dict(firstColumn=64),
               dict(firstColumn=-1), dict(firstColumn=True), dict(firstTable=16), dict(firstTable=10, tableN=7), dict(firstOut=1),
               dict(out=o, firstOut=25), dict(out=o, firstOut=-1), dict(N=1 << 32), dict(tableN=(1 << 30) + 1),
               dict(out=t), dict(out=f), dict(out=same, firstOut=48),                          # the exact ranges, and
               dict(firstTable=4, tableN=4, out=t, firstOut=1), dict(firstTable=4, tableN=4, out=t, firstOut=7),   # every partial one
               dict(firstColumn=20, N=10, tableN=4, out=f, firstOut=17), dict(firstColumn=20, N=10, tableN=4, out=same, firstOut=29)):
        with pytest.raises(ValueError):
            _args(f, t, **kw)
    assert _args(f, t, firstColumn=20, N=10, tableN=4, out=f, firstOut=16)["N"] == 10
    assert _args(f, t, firstColumn=20, N=10, tableN=4, out=f, firstOut=30)["N"] == 10
    assert _args(f, t, firstTable=4, tableN=4, out=t, firstOut=0)["tableN"] == 4
    assert _args(f, t, firstTable=4, tableN=4, out=t, firstOut=8)["tableN"] == 4


# ------------------------------------------------------------------------------------------------ the library
NAMES = ("msmz_scalars_lookup", "msmz_test_lookup_geometry", "msmz_test_lookup_slot", "msmz_test_lookup_small_table")


def test_entry_points_are_exported(lib):
    from msm_zprize_amd import _native
    for name in NAMES:
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    assert C.sizeof(_native.MsmzLookup) == 64 and C.sizeof(_native.MsmzLookupResult) == 24
    assert _native.LOOKUP_NONE == L.NONE
    from msm_zprize_amd.parallel import _Parallel
    assert callable(_Parallel.lookupMultiplicities)


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof and the offsets of every field of the two descriptors, C side == ctypes side"""
    from msm_zprize_amd import _native as N
    src = tmp_path / "layout.c"
    prints, want = [], []
    for cname, T in (("msmz_lookup", N.MsmzLookup), ("msmz_lookup_result", N.MsmzLookupResult)):
        prints.append(f'printf("%zu ", sizeof({cname}));')
        want.append(C.sizeof(T))
        for fname, _ in T._fields_:
            prints.append(f'printf("%zu ", offsetof({cname}, {fname}));')
            want.append(getattr(T, fname).offset)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msmz.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()] == want
    assert want[0] == 64 and want[len(N.MsmzLookup._fields_) + 1] == 24
    header = open(os.path.join(ROOT, "include", "msmz.h")).read()
    assert "} msmz_lookup;           /* 64 bytes */" in header and "} msmz_lookup_result;      /* 24 bytes */" in header


def test_null_arguments_are_bad_arguments(lib):
    """no context, no device -> MSMZ_ERR_ARG and the outputs untouched"""
    from msm_zprize_amd import _native as N
    pos = (C.c_uint32 * 2)(77, 78)
    l = N.MsmzLookup(1, 0, 1, 2, 0, 2, pos, 0)
    h = C.c_uint64(77)
    res = N.MsmzLookupResult(5, 6, 7)
    assert lib.msmz_scalars_lookup(None, C.byref(l), 0, C.byref(h), C.byref(res)) == 1
    assert lib.msmz_scalars_lookup(None, C.byref(l), 0, C.byref(h), None) == 1
    assert lib.msmz_scalars_lookup(None, None, 0, C.byref(h), C.byref(res)) == 1
    assert lib.msmz_scalars_lookup(None, C.byref(l), 0, None, C.byref(res)) == 1
    assert h.value == 77 and (res.n_missing, res.first_missing, res.n_distinct) == (5, 6, 7) and list(pos) == [77, 78]
