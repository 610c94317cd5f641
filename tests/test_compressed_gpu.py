"""Compressed point sets on the GPU (msmz_import_points with MSMZ_SRC_COMPRESSED, msmz_download_points_compressed).  The
cases are in tests/compressed_gpu_cases.py; each test here runs one of its test functions, with all its parameters, in
a fresh child process that imports torch BEFORE libmsmz.so is loaded, as tests/test_scalar_import_gpu.py does and for
its reason: the device-memory sources are torch tensors, and a process drives the GPU through one HIP runtime only."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "compressed_gpu_cases.py")


def _run(name, timeout):
    code = ("import sys, torch, pytest; "
            "sys.exit(pytest.main([%r, '-x', '-q', '-p', 'no:cacheprovider', '--durations=5']))" % (CASES + "::" + name))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       stdin=subprocess.DEVNULL)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("name,timeout", [
    ("test_round_trip", 300), ("test_generated_set_survives_compression", 300), ("test_the_set_is_ordinary", 300),
    ("test_refusals", 300), ("test_two_engines_on_one_gpu", 300)])
def test_compressed_gpu(name, timeout):
    _run(name, timeout)
