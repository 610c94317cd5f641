"""The batched inner products through the JavaScript host (js/parallel.mjs innerProducts / evaluatePolynomials over
napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

import dot_many_util as U
import scalar_ops_util as S
from test_dot_many_cpu import BAD_TYPE, BAD_VALUE, GOOD, _args, _arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-dot-many.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "dot_many_js_fixture.json")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_script_parses(addon):
    """CPU: the addon exports the call, it refuses bad arguments without a device, the descriptor sizes and limits are the
    header's and the call without a family answers what it did, and the script parses"""
    js = ("const a=require(%r); const t=typeof a.scalarsDotMany; let refused=0; const b=Buffer.alloc(16);"
          "for (const f of [()=>a.scalarsDotMany(), ()=>a.scalarsDotMany(null,b,1,b,1,4,0,0,0), ()=>a.scalarsDotMany(null,b,2,b,1,4,0,0,0),"
          "()=>a.scalarsDotMany(null,b,1,b,9,4,0,0,0), ()=>a.scalarsDotMany(null,b,1,null,1,4,0,0,0)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused, a.descriptorSizes('dotMany'),"
          " a.descriptorSizes()]))" % addon)
    t, refused, sizes, plain = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert (t, refused) == ("function", 5)
    from msm_zprize_amd import _native as N
    import ctypes as C
    assert sizes == {"dotMany": C.sizeof(N.MsmzDotMany), "scalarVec": C.sizeof(N.MsmzScalarVec), "maxRows": N.MSMZ_DOT_MANY_MAX_ROWS,
                     "maxCols": N.MSMZ_DOT_MANY_MAX_COLS} == {"dotMany": 48, "scalarVec": 16, "maxRows": 128, "maxCols": 8}
    assert plain == {"mleBind": 40, "sumcheck": 32, "sumcheckTable": 16, "sumcheckTerm": 16, "maxTables": 6, "maxDegree": 4,
                     "maxTerms": 8}
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def _js(case):
    """a case of tests/test_dot_many_cpu.py in JavaScript's notation"""
    f, g, d, pts = "F", "G", "D", "P"
    names = {1: f, 2: g, 3: d, 4: pts}

    def val(v):
        if v is None:
            return "null"
        if isinstance(v, (list, tuple)):
            return "[" + ",".join(val(e) for e in v) + "]"
        if hasattr(v, "handle"):
            return names[v.handle]
        return repr(v)

    rows, cols, n, out, first_out = case(_arr(64, 1), _arr(100, 2), _arr(64, 3))
    return "[%s,%s,%s,{out:%s,firstOut:%s}]" % (val(rows), val(cols), val(n), val(out), val(first_out))


def test_js_host_args():
    """CPU: dotManyArgs accepts and refuses what the Python twin does in tests/test_dot_many_cpu.py, case for case, with a
    TypeError where Python raises one, and returns the same n and firstOut"""
    cases = GOOD + BAD_TYPE + BAD_VALUE
    js = ("import('%s').then((m)=>{ const F={handle:1,n:64,kind:'scalars'}, G={handle:2,n:100,kind:'scalars'},"
          "D={handle:3,n:64,kind:'scalars'}, P={handle:4,n:64,kind:'points'};"
          "const run=(a)=>{ try { const t=m.dotManyArgs(a[0],a[1],a[2],a[3]); return ['ok',t.n,t.firstOut,t.rows.length,t.cols.length]; }"
          " catch (e) { return [e instanceof TypeError ? 'type' : 'value']; } };"
          "console.log(JSON.stringify([%s].map(run))); })"
          % (os.path.join(ROOT, "js", "parallel.mjs"), ",".join(_js(c) for c in cases)))
    got = json.loads(subprocess.check_output([NODE, "-e", js], text=True, cwd=ROOT))
    f, g, d = _arr(64, 1), _arr(100, 2), _arr(64, 3)
    for k, case in enumerate(GOOD):
        want = _args(*case(f, g, d))
        assert got[k] == ["ok", want["N"], want["firstOut"], len(want["rows"]), len(want["cols"])], (k, got[k])
    kinds = [r[0] for r in got[len(GOOD):]]
    assert kinds == ["type"] * len(BAD_TYPE) + ["value"] * len(BAD_VALUE), list(enumerate(kinds))


def test_fixture_is_self_consistent():
    """CPU: the committed fixture holds the planted values and what Python integers say today"""
    fx = json.load(open(FIXTURE))
    q = S.order(fx["curve"])
    rows = [[int(e) for e in r] for r in fx["rows"]]
    cols = [[int(e) for e in c] for c in fx["cols"]]
    assert (fx["curve"], len(rows), len(cols), fx["n"]) == ("bls12-377", 6, 3, 70)
    assert all(len(v) == 70 and all(0 <= e < q for e in v) for v in rows + cols)
    assert {0, q - 1} <= set(rows[0]) and q - 1 in cols[0]
    assert [[int(e) for e in r] for r in fx["values"]] == U.products(rows, cols, q)
    points = [int(z) for z in fx["points"]]
    assert q - 1 in points and [[int(e) for e in r] for r in fx["evals"]] == [[U.horner(r, z, q) for z in points] for r in rows]


@pytest.mark.gpu
def test_js_dot_many(addon):
    """GPU: node reproduces the fixture's values on the host and in a range of a resident array whose neighbours stay,
    pair by pair equal to innerProduct, and the evaluations"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["values"] == fx["values"] and got["resident"] == fx["values"] and got["around"] == ["7"] * 5
    assert got["evals"] == fx["evals"]
    assert got["pairs"] and got["sizes"] and got["refused"]
