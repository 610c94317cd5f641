"""Multilinear polynomials over resident scalar arrays through the JavaScript host (js/parallel.mjs eqTable / evaluateMle /
bindMle / sumcheckRound over napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

import mle_util as M
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-mle.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "mle_js_fixture.json")
MODES = ("eq", "evals", "bindHigh", "bindLow", "inPlace", "roundHigh", "roundLow")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_mle_script_parses(addon):
    """CPU: the addon exports the four calls, they refuse bad arguments without a device, its descriptor sizes and limits
    are the header's, and the script parses"""
    js = ("const a=require(%r); const t=[a.scalarsEqTable,a.scalarsMleEval,a.scalarsMleBind,a.scalarsSumcheckRound].map((f)=>typeof f);"
          "let refused=0; const b=Buffer.alloc(64);"
          "for (const f of [()=>a.scalarsEqTable(), ()=>a.scalarsEqTable(null,b,2,null), ()=>a.scalarsMleEval(null,1,0,b,2),"
          "()=>a.scalarsMleBind(null,1,0,1,1,0,b.subarray(0,32),0,0), ()=>a.scalarsSumcheckRound(null,b,1,1,b,b,b,1,0)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused, a.descriptorSizes()]))" % addon)
    t, refused, sizes = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert (t, refused) == (["function"] * 4, 5)
    assert sizes == {"mleBind": 40, "sumcheck": 32, "sumcheckTable": 16, "sumcheckTerm": 16, "maxTables": 6, "maxDegree": 4,
                     "maxTerms": 8}
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_js_mle_host_args():
    """CPU: the host-only argument checks of js/parallel.mjs refuse what the Python twins refuse"""
    js = ("import('%s').then((m)=>{ const q=1009n; const f={handle:1,n:64,kind:'scalars'}; let ok=0, refused=0;"
          "const good=[()=>m.eqTableArgs([3n,5n],1n,q), ()=>m.mleEvalArgs(f,[1n,2n,3n],{first:56},q), ()=>m.mleBindArgs(f,5n,{out:f},q),"
          "()=>m.mleBindArgs(f,5n,{nVars:4,first:16,out:f,firstOut:32},q), ()=>m.sumcheckRoundArgs([f,[f,0]],[[null,3],[q-1n,2]],{},q)];"
          "const bad=[()=>m.eqTableArgs([q],1n,q), ()=>m.eqTableArgs([1],1n,q), ()=>m.eqTableArgs(Array(32).fill(0n),1n,q),"
          "()=>m.mleEvalArgs(f,[1n,2n,3n],{first:57},q), ()=>m.mleBindArgs(f,5n,{out:f,firstOut:32},q), ()=>m.mleBindArgs(f,5n,{low:true,out:f},q),"
          "()=>m.mleBindArgs(f,5n,{count:2,out:f},q), ()=>m.mleBindArgs(f,q,{},q), ()=>m.mleBindArgs(f,5n,{nVars:31,count:2},q),"
          "()=>m.sumcheckRoundArgs([f],[[null,2]],{},q), ()=>m.sumcheckRoundArgs(Array(5).fill(f),[[null,31]],{},q),"
          "()=>m.sumcheckRoundArgs(Array(7).fill(f),[[null,1]],{},q), ()=>m.sumcheckRoundArgs([f],[],{},q), ()=>m.sumcheckRoundArgs([f],[[q,1]],{},q)];"
          "for (const g of good) { g(); ok++; } for (const g of bad) { try { g(); } catch (e) { refused++; } }"
          "console.log(JSON.stringify([ok, refused, bad.length])); })" % os.path.join(ROOT, "js", "parallel.mjs"))
    ok, refused, nbad = json.loads(subprocess.check_output([NODE, "-e", js], text=True, cwd=ROOT))
    assert ok == 5 and refused == nbad == 14


def test_fixture_is_self_consistent():
    """CPU: the committed fixture holds the planted values and what Python integers say today"""
    fx = json.load(open(FIXTURE))
    q = S.order(fx["curve"])
    v = fx["nVars"]
    n = 1 << v
    assert fx["curve"] == "bls12-377" and v == 6 and len(fx["tables"]) == 3 and len(fx["point"]) == v
    tables = [[int(e) for e in t] for t in fx["tables"]]
    point, scale, r = [int(e) for e in fx["point"]], int(fx["scale"]), int(fx["r"])
    terms = [(None if c is None else int(c), m) for c, m in fx["terms"]]
    assert all(len(t) == n and all(0 <= e < q for e in t) for t in tables) and all(0 <= e < q for e in point + [scale, r])
    assert {0, 1, q - 1, S.low_words_full(q)} <= set(tables[0]) and {0, 1, q - 1} <= set(point)
    assert sorted(bin(m).count("1") for _, m in terms) == [1, 2]            # mixed degree
    ints = lambda key: [int(e) for e in fx[key]]   # noqa: E731
    assert ints("eq") == M.eq(point, q, scale)
    assert ints("evals") == [M.mle_eval(t, point, q) for t in tables]
    assert ints("bindHigh") == sum((M.bind(t, r, q) for t in tables), [])
    assert ints("bindLow") == sum((M.bind(t, r, q, True) for t in tables), [])
    assert ints("inPlace") == M.bind(tables[0], r, q) + tables[0][n // 2:]
    assert ints("roundHigh") == M.round_poly(tables, terms, q) and ints("roundLow") == M.round_poly(tables, terms, q, True)
    assert len(fx["roundHigh"]) == 3


@pytest.mark.gpu
def test_js_mle(addon):
    """GPU: node runs the four calls on the fixture; every value is the fixture's"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert got[mode] == fx[mode], mode
    assert got["sizes"] and got["refused"]
