"""Gate expressions through the JavaScript host (js/parallel.mjs evaluateExpression over napi/msmz_napi.c scalarsExpr)."""
import json
import os
import shutil
import subprocess

import pytest

import expr_util as E
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-expr.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "expr_js_fixture.json")
SIZES = {"exprColumn": 16, "exprFactor": 8, "exprTerm": 24, "expr": 40, "maxColumns": 16, "maxTerms": 32, "maxDegree": 8,
         "maxOperands": 32}


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_expr_script_parses(addon):
    """CPU: the addon exports the call, it refuses bad arguments without a device -- too few, no context, counts outside
    their bounds, buffers shorter than the counts say, a term of nine factors -- its descriptor sizes and limits are the
    header's, asked for by family, the call without an argument answering what it did; and the script parses"""
    js = ("const a=require(%r); const t=typeof a.scalarsExpr; let refused=0; const B=(n)=>Buffer.alloc(n);"
          "for (const f of [()=>a.scalarsExpr(), ()=>a.scalarsExpr(null,B(16),1,B(8),B(1),B(32),B(1),1,4,0,0),"
          "()=>a.scalarsExpr({},B(16),1,B(8),B(1),B(32),B(1),1,4,0,0), ()=>a.scalarsExpr({},B(16),0,B(8),B(1),B(32),B(1),1,4,0,0),"
          "()=>a.scalarsExpr({},B(16),17,B(8),B(1),B(32),B(1),1,4,0,0), ()=>a.scalarsExpr({},B(16),1,B(8),B(1),B(32),B(1),33,4,0,0),"
          "()=>a.scalarsExpr({},B(15),1,B(8),B(1),B(32),B(1),1,4,0,0), ()=>a.scalarsExpr({},B(16),1,B(8),B(1),B(31),B(1),1,4,0,0),"
          "()=>a.scalarsExpr({},B(16),1,B(8),Buffer.from([2]),B(32),B(1),1,4,0,0), ()=>a.scalarsExpr({},B(16),1,B(72),Buffer.from([9]),B(32),B(1),1,4,0,0)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused, a.descriptorSizes('expr'),"
          "Object.keys(a.descriptorSizes()).length, Object.keys(a.descriptorSizes('lookup')).length]))" % addon)
    t, refused, sizes, old, lookup = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert (t, refused) == ("function", 10)
    assert sizes == SIZES and old == 7 and lookup == 3
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_js_expr_host_args():
    """CPU: the host-only argument checks of js/parallel.mjs refuse what the Python twin refuses, and accept what it accepts"""
    q = S.order("bls12-377")
    js = ("import('%s').then((m)=>{ const q=%dn; const a={handle:1,n:64,kind:'scalars'}; const b={handle:2,n:64,kind:'scalars'};"
          "const o={handle:3,n:100,kind:'scalars'}; const p={handle:4,n:64,kind:'points'}; let ok=0, refused=0;"
          "const g=(c,t,op)=>m.exprArgs(c,t,op,q); const T=[[null,[0]]];"
          "const many=[0,1,2,3].map((t)=>[null,[0,1,2,3,4,5,6,7].map((k)=>[(8*t+k)%%2,Math.floor((8*t+k)/2)])]);"
          "const good=[()=>g([a,[b,0]],[[5n,[0,[1,-1]]],[null,[]],[q-1n,[1,1,1,1,1,1,1,1]]]).n===64, ()=>g([[a,4],[b,4]],T).n===60,"
          "()=>g([[a,4],[o,40]],T).n===60, ()=>g([a,o],T,{n:10,out:o,firstOut:90}).n===10, ()=>g([a],[[null,[[0,2**31-1],[0,-(2**31)]]]]).n===64,"
          "()=>g([[a,8]],[[3n,[0,[0,8],[0,-16]]]],{n:8,out:{...a},firstOut:8}).n===8, ()=>g([[a,8]],[[null,[[0,1]]]],{n:8,out:a,firstOut:16}).n===8,"
          "()=>g([[b,8],[a,12]],[[null,[[0,1]]]],{n:8,out:a,firstOut:13}).n===8, ()=>g([[a,8]],[[7n,[]]],{n:8,out:a,firstOut:11}).n===8,"
          "()=>g([a,a],many.concat([[null,[[0,64]]]])).n===64,"
          "()=>JSON.stringify(g([a],[[2n,[0,[0,3]]],[null,[]]]).terms.map((t)=>t[1]))==='[[[0,0],[0,3]],[]]'];"
          "const bad=[()=>g(a,T), ()=>g([a],[null,[0]]), ()=>g([7],T), ()=>g([p],T), ()=>g([[a,0,0]],T), ()=>g([a],[null]), ()=>g([a],[[null]]),"
          "()=>g([a],[[null,0]]), ()=>g([a],[[1,[0]]]), ()=>g([a],[[null,[0.5]]]), ()=>g([a],[[null,[[0,1.5]]]]), ()=>g([a],T,{out:7}), ()=>g([a],T,{out:p}),"
          "()=>g([],[[null,[]]],{n:4}), ()=>g(Array(17).fill(a),T), ()=>g([a],[]), ()=>g([a],Array(33).fill(T[0])), ()=>g([a],[[q,[0]]]), ()=>g([a],[[-1n,[0]]]),"
          "()=>g([a],[[null,[1]]]), ()=>g([a],[[null,[-1]]]), ()=>g([a],[[null,[[0,2**31]]]]), ()=>g([a],[[null,[[0,-(2**31)-1]]]]),"
          "()=>g([a],[[null,[0,0,0,0,0,0,0,0,0]]]), ()=>g([a,o],T), ()=>g([[a,1],b],T), ()=>g([a],T,{n:0}), ()=>g([a],T,{n:65}), ()=>g([a],T,{n:1.5}),"
          "()=>g([a],T,{n:2**32}), ()=>g([[a,64]],T,{n:1}), ()=>g([[a,-1]],T,{n:1}), ()=>g([[a,60]],T,{n:5}), ()=>g([a],T,{firstOut:1}),"
          "()=>g([a],T,{out:o,firstOut:37}), ()=>g([a],T,{out:o,firstOut:-1}), ()=>g([a,a],many.concat([[null,[[0,16]]]])),"
          "()=>g([[a,8]],T,{n:8,out:{...a},firstOut:9}), ()=>g([[a,8]],T,{n:8,out:a,firstOut:1}), ()=>g([[a,8]],T,{n:8,out:a,firstOut:15}),"
          "()=>g([[a,8]],[[null,[[0,1]]]],{n:8,out:a,firstOut:8}), ()=>g([[a,8]],[[null,[0,[0,8],[0,-3]]]],{n:8,out:{...a},firstOut:15}),"
          "()=>g([[a,8]],[[null,[[0,1]]]],{n:8,out:a,firstOut:1})];"
          "for (const c of good) { if (c()) ok++; } for (const c of bad) { try { c(); } catch (e) { refused++; } }"
          "console.log(JSON.stringify([ok, good.length, refused, bad.length])); })" % (os.path.join(ROOT, "js", "parallel.mjs"), q))
    ok, ngood, refused, nbad = json.loads(subprocess.check_output([NODE, "-e", js], text=True, cwd=ROOT))
    assert ok == ngood == 11 and refused == nbad == 43


def test_fixture_is_self_consistent():
    """CPU: the committed fixture holds what Python integers say today, and the shapes the script relies on"""
    fx = json.load(open(FIXTURE))
    q = S.order(fx["curve"])
    n = fx["n"]
    cols = [[int(v) for v in col] for col in fx["columns"]]
    assert fx["curve"] == "bls12-377" and n == 70 and len(cols) == 8 and all(len(c) == n for c in cols)
    assert all(0 <= v < q for c in cols for v in c) and {0, 1, q - 1} <= set(cols[0])
    assert list(fx["expressions"]) == ["plonk", "permutation", "sbox", "rotations", "a8"]
    acc, y = [0] * n, int(fx["y"])
    for name, e in fx["expressions"].items():
        terms = [(None if c is None else int(c), [tuple(f) for f in fs]) for c, fs in e["terms"]]
        want = E.model(cols, terms, n, q)
        assert [int(v) for v in e["expected"]] == want and any(want)
        if name in ("plonk", "permutation", "sbox"):
            acc = [(y * a + g) % q for a, g in zip(acc, want)]
    assert [int(v) for v in fx["accumulated"]] == acc
    rots = {rot for e in fx["expressions"].values() for _, fs in e["terms"] for _, rot in fs}
    assert {0, 1, -1, 2, E.INT32_MAX, E.INT32_MIN} <= rots
    assert max(len(fs) for e in fx["expressions"].values() for _, fs in e["terms"]) == E.MAX_DEGREE
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.gpu
def test_js_expr(addon):
    """GPU: node evaluates every expression of the fixture into a new array, accumulates three of them in place and
    writes one behind its own columns in one array"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["values"] == {name: e["expected"] for name, e in fx["expressions"].items()}
    assert got["accumulated"] == fx["accumulated"]
    assert got["intoRange"] == fx["columns"][5] + fx["columns"][6] + fx["expressions"]["plonk"]["expected"]
    assert got["sizes"] and got["refused"]
