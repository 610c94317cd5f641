"""in_range and partial_overlap (csrc/ranges.h), the two predicates every first / n argument check goes through,
compiled for the host (tests/native/ranges_test.cpp) against Python integers, which do not wrap; the same program once
more under the address and undefined-behaviour sanitizers.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ranges_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "ranges_test")
EXE_ASAN = EXE + "_asan"
DEPS = [SRC, os.path.join(ROOT, "msm_zprize_amd", "csrc", "ranges.h")]
TOP = (1 << 64) - 1


def _build(exe, extra):
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + extra + ["-o", exe, SRC])


def _run(exe, lines):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-3000:]
    out = res.stdout.split()
    assert len(out) == len(lines)
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def driver():
    _build(EXE, [])
    return lambda lines: _run(EXE, lines)


def in_range_cases():
    """(first, n, len): the edges of the issue for lengths 0, 1, 8, 2^32 - 1, 2^32, 2^32 + 8 and 2^64 - 1"""
    cases = []
    for ln in (0, 1, 8, (1 << 32) - 1, 1 << 32, (1 << 32) + 8, TOP):
        firsts = {0, 1, 8, 9, ln // 2, max(ln - 1, 0), ln, min(ln + 1, TOP), (1 << 32) - 1, 1 << 32, TOP - 1, TOP}
        for first in sorted(firsts):
            rest = ln - first if first <= ln else 0
            ns = {0, 1, 2, rest, max(rest - 1, 0), min(rest + 1, TOP), (1 << 32) - 1, 1 << 32, TOP - first, TOP - first + 1,
                  TOP - first + 2, TOP - 1, TOP}
            cases += [(first, n, ln) for n in sorted(v for v in ns if 0 <= v <= TOP)]
    return cases


def test_in_range_matches_integers(driver):
    cases = in_range_cases()
    for must in ((8, 0, 8), (8, 1, 8), (9, 0, 8), (TOP, 2, 8), (0, TOP, 8), (0, TOP, TOP), (0, 0, 0), (0, 1, 0), (1, 0, 0),
                 (8, 1 << 32, (1 << 32) + 8), (9, 1 << 32, (1 << 32) + 8), (0, 1 << 32, 1 << 32), (1, 1 << 32, 1 << 32)):
        assert must in cases, must
    got = driver([f"in {f:x} {n:x} {ln:x}" for f, n, ln in cases])
    bad = [(c, g) for c, g in zip(cases, got) if g != int(c[0] + c[1] <= c[2])]
    assert not bad, bad[:3]
    assert got[cases.index((TOP, 2, 8))] == 0        # first + n wraps to 1
    assert got[cases.index((8, 0, 8))] == 1 and got[cases.index((8, 1, 8))] == 0


def overlap_cases():
    """(a, b, n): distances 0, 1, n - 1, n, n + 1 in both orders, from starts at 0, in the middle and near 2^64 - 1"""
    cases = []
    for n in (0, 1, 2, 3, 8, 1 << 32, TOP):
        for d in sorted({0, 1, max(n - 1, 0), n, min(n + 1, TOP), TOP}):
            for base in (0, 5, 1 << 32, TOP - d):
                if base + d <= TOP:
                    cases += [(base, base + d, n), (base + d, base, n)]
    return cases


def test_partial_overlap_matches_integers(driver):
    cases = overlap_cases()
    for must in ((5, 5, 8), (5, 6, 8), (5, 12, 8), (12, 5, 8), (5, 13, 8), (13, 5, 8), (5, 14, 8), (5, 5, 1), (5, 6, 1), (6, 5, 1),
                 (TOP, TOP, 8), (TOP - 1, TOP, 8), (TOP, TOP - 7, 8), (TOP - 8, TOP, 8), (0, TOP, TOP), (TOP, 0, TOP)):
        assert must in cases, must
    got = driver([f"ov {a:x} {b:x} {n:x}" for a, b, n in cases])
    bad = [(c, g) for c, g in zip(cases, got) if g != int(c[0] != c[1] and abs(c[0] - c[1]) < c[2])]
    assert not bad, bad[:3]


def test_sanitizer_build_runs_clean(driver):
    """the same stand-alone program built with -fsanitize=address,undefined, run as a process of its own on every case:
    it exits 0, writes nothing to stderr, and answers as the plain build does"""
    _build(EXE_ASAN, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    lines = [f"in {f:x} {n:x} {ln:x}" for f, n, ln in in_range_cases()] + [f"ov {a:x} {b:x} {n:x}" for a, b, n in overlap_cases()]
    assert _run(EXE_ASAN, lines) == driver(lines)
