"""Arithmetic over resident scalar arrays through the JavaScript host (js/parallel.mjs combineScalars / innerProduct /
scalarPowers over napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-scalar-ops.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "scalar_ops_js_fixture.json")
MODES = ("scaled", "hadamard", "combined", "fold", "dot", "sum", "cross", "powers")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_scalar_ops_script_parses(addon):
    """CPU: the addon exports the three calls, they refuse bad arguments without a device, and the script parses"""
    js = ("const a=require(%r); const t=[a.scalarsCombine,a.scalarsDot,a.scalarsPowers].map((f)=>typeof f); let refused=0;"
          "for (const f of [()=>a.scalarsCombine(), ()=>a.scalarsDot(null,1,0,0,0,1), ()=>a.scalarsPowers(null,null,null,1)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused]))" % addon)
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == [["function"] * 3, 3]
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_fixture_is_self_consistent():
    """CPU: the committed fixture holds the planted values and what Python integers say today"""
    fx = json.load(open(FIXTURE))
    q = S.order(fx["curve"])
    n, half = fx["n"], fx["n"] // 2
    assert n == 65 and all(len(fx[k]) == n for k in ("x", "y", "c", "scaled", "hadamard", "combined", "fold", "powers"))
    x, y, c = ([int(v) for v in fx[k]] for k in ("x", "y", "c"))
    a, b, z = int(fx["a"]), int(fx["b"]), int(fx["z"])
    assert all(0 <= v < q for v in x + y + c + [a, b, z])
    assert {0, 1, q - 1, S.low_words_full(q)} <= set(x) and any(u + v == q for u, v in zip(x, y))
    assert [int(v) for v in fx["scaled"]] == [a * v % q for v in x]
    assert [int(v) for v in fx["hadamard"]] == [w * v % q for w, v in zip(c, x)]
    assert [int(v) for v in fx["combined"]] == [(w * u + b * v) % q for w, u, v in zip(c, x, y)]
    assert [int(v) for v in fx["fold"]] == [(x[i] + a * x[half + i]) % q for i in range(half)] + x[half:]
    assert int(fx["dot"]) == sum(u * v for u, v in zip(x, y)) % q and int(fx["sum"]) == sum(x) % q
    assert int(fx["cross"]) == sum(x[i] * y[half + i] for i in range(half)) % q
    assert [int(v) for v in fx["powers"]] == [b * pow(z, i, q) % q for i in range(n)]


@pytest.mark.gpu
def test_js_scalar_ops(addon):
    """GPU: node runs the three calls on the fixture's 65 scalars, the fold in place; every value is the fixture's"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert got[mode] == fx[mode], mode
    assert got["refused"]
