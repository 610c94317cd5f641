"""Exports on the GPU (msmz_export_scalars / msmz_export_points; scalarsToTensor, pointsToTensor, scalarsToBytes,
pointsToBytes).  The cases are in tests/export_gpu_cases.py; each test here runs one of its test functions, with all its
parameters, in a fresh child process that imports torch BEFORE libmsmz.so is loaded, exactly as
tests/test_scalar_import_gpu.py does and for the reason given there."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "export_gpu_cases.py")


def _run(name, timeout):
    code = ("import sys, torch, pytest; "
            "sys.exit(pytest.main([%r, '-x', '-q', '-p', 'no:cacheprovider', '--durations=5']))" % (CASES + "::" + name))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       stdin=subprocess.DEVNULL)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("name,timeout", [
    ("test_scalar_forms", 300), ("test_round_trips", 300), ("test_overflow_and_range", 300), ("test_point_forms", 300),
    ("test_result_is_usable_where_it_lies", 300), ("test_argument_errors", 120),
    ("test_pinned_host_memory_as_a_device_destination", 120), ("test_export_behind_a_torch_stream", 120),
    ("test_two_engines_on_one_gpu", 300)])
def test_export_gpu(name, timeout):
    _run(name, timeout)
