"""MultiEngine (csrc/multi.h) over mock engines on a toy group, 1 to 8 of them, without a GPU: the self-checking program
tests/native/multi_engine_test.cpp built three ways -- plain, under the thread sanitizer, and under the address and
undefined-behaviour sanitizers -- each run as a process of its own.  Every build exits 0, writes nothing to stderr (a
sanitizer reports there) and runs the same number of cases, so an empty run cannot pass.  Nothing is loaded into Python.
CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "multi_engine_test.cpp")
EXE = os.path.join(ROOT, "tests", "native", "multi_engine_test")
CSRC = os.path.join(ROOT, "msm_zprize_amd", "csrc")
DEPS = [SRC, os.path.join(ROOT, "include", "msmz.h")] + \
    [os.path.join(CSRC, h) for h in ("multi.h", "iengine.h", "ranges.h", "fr.h", "fp.h", "constants_gen.h")]
BUILDS = {
    "plain": (EXE, ["-O2"]),
    "tsan": (EXE + "_tsan", ["-O1", "-g", "-fsanitize=thread"]),
    "asan": (EXE + "_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
}
_results = {}


def _run(variant):
    """build (when stale) and run one variant, once per session -> (status, stdout, stderr, cases)"""
    if variant in _results:
        return _results[variant]
    exe, flags = BUILDS[variant]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        cc = subprocess.run(["g++", "-std=c++17", "-pthread"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
        if cc.returncode != 0:
            missing = [ln for ln in cc.stderr.splitlines() if re.search(r"cannot find .*(tsan|asan|ubsan)", ln)]
            if variant != "plain" and missing:
                pytest.skip("the sanitizer runtime does not link here: " + missing[0].strip())
            pytest.fail("g++ failed:\n" + cc.stderr[-3000:])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    m = re.search(r"^cases (\d+)$", res.stdout, re.M)
    _results[variant] = (res.returncode, res.stdout, res.stderr, int(m.group(1)) if m else 0)
    return _results[variant]


@pytest.mark.parametrize("variant", list(BUILDS))
def test_multi_engine_over_mock_engines(variant):
    status, out, err, cases = _run(variant)
    assert status == 0 and err == "", (status, out[-3000:], err[-3000:])
    assert cases > 0
    assert cases == _run("plain")[3], "the builds ran different numbers of cases"
