"""Recurrences and inversion over resident scalar arrays through the JavaScript host (js/parallel.mjs scalarRecurrence /
prefixProducts / prefixSums / divideByLinear / invertScalars over napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

import scalar_ops_util as S
import scalar_scan_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-scalar-scan.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "scalar_scan_js_fixture.json")
MODES = ("sums", "products", "grand", "quotient", "value", "general", "inverse", "zeros", "inplace")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_scalar_scan_script_parses(addon):
    """CPU: the addon exports the two calls, they refuse bad arguments without a device, and the script parses"""
    js = ("const a=require(%r); const t=[a.scalarsRecurrence,a.scalarsInverse].map((f)=>typeof f); let refused=0;"
          "for (const f of [()=>a.scalarsRecurrence(), ()=>a.scalarsRecurrence(null,1,0,0,0,null,0,1,0,0),"
          "()=>a.scalarsInverse(null,1,0,1,0,0)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused]))" % addon)
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == [["function"] * 2, 3]
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_fixture_is_self_consistent():
    """CPU: the committed fixture holds the planted values and what Python integers say today"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_scalar_scan_fixture",
                                                  os.path.join(ROOT, "tests", "golden", "make_scalar_scan_fixture.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    fx = json.load(open(FIXTURE))
    assert fx == maker.build()
    q = S.order(fx["curve"])
    n = fx["n"]
    x, y = ([int(v) for v in fx[k]] for k in ("x", "y"))
    assert n == 65 and len(x) == len(y) == n and {0, 1, q - 1, S.low_words_full(q)} <= set(x)
    assert fx["zeros"] == x.count(0) >= 1
    assert fx["grand"][0][0] == "1" and fx["quotient"][-1] == "0"
    z = int(fx["z"])
    assert int(fx["value"]) == sum(c * pow(z, i, q) for i, c in enumerate(y)) % q
    assert [int(v) for v in fx["sums"][0]] == [sum(y[:i + 1]) % q for i in range(n)]
    assert all(u * int(w) % q == (1 if u else 0) for u, w in zip(x, fx["inverse"]))
    assert U.recurrence(q, n, x, None)[1] == int(fx["products"][1]) == int(fx["grand"][1])


@pytest.mark.gpu
def test_js_scalar_scan(addon):
    """GPU: node runs the calls on the fixture's 65 scalars, one inversion in place; every value is the fixture's"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert got[mode] == fx[mode], mode
    assert got["refused"]
