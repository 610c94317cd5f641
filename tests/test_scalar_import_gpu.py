"""Imports on the GPU (msmz_import_scalars / _into / msmz_import_points; scalarsFromTensor, pointsFromTensor, scalarsInto).
The cases are in tests/import_gpu_cases.py; each test here runs one of its test functions, with all its parameters, in a
fresh child process that imports torch BEFORE libmsmz.so is loaded.  torch brings its own copy of the HIP runtime and a
process can drive the GPU through one copy only: the copy loaded first serves both (that is the order bench.py uses).
This process has usually loaded libmsmz.so on the system's runtime already, for the other GPU tests, so torch could not
see the GPU from here."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "import_gpu_cases.py")


def _run(name, timeout):
    code = ("import sys, torch, pytest; "
            "sys.exit(pytest.main([%r, '-x', '-q', '-p', 'no:cacheprovider', '--durations=5']))" % (CASES + "::" + name))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       stdin=subprocess.DEVNULL)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("name,timeout", [
    ("test_scalar_conversion", 600), ("test_point_conversion", 600), ("test_pinned_host_memory_as_a_device_source", 300),
    ("test_msm_over_imported_handles", 900), ("test_precomputed_set_from_imported_points", 600),
    ("test_msm_batch_over_a_list_of_device_tensors", 600), ("test_range_errors_leave_the_context_usable", 600),
    ("test_argument_errors", 300), ("test_three_engines_on_one_gpu", 600), ("test_import_behind_a_torch_stream", 300)])
def test_import_gpu(name, timeout):
    _run(name, timeout)
