"""The multiplicities of a column in a table through the JavaScript host (js/parallel.mjs lookupMultiplicities over
napi/msmz_napi.c scalarsLookup)."""
import json
import os
import shutil
import subprocess

import pytest

import lookup_util as L
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-lookup.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "lookup_js_fixture.json")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_lookup_script_parses(addon):
    """CPU: the addon exports the call, it refuses bad arguments without a device, its descriptor sizes are the header's --
    asked for by family, the call without an argument answering what it did -- and the script parses"""
    js = ("const a=require(%r); const t=typeof a.scalarsLookup; let refused=0;"
          "for (const f of [()=>a.scalarsLookup(), ()=>a.scalarsLookup(null,1,0,4,2,0,4,0,0,false), ()=>a.scalarsLookup({},1,0,4,2,0,4,0,0,true),"
          "()=>a.scalarsLookup(null,1,0,4,2,0,0,0,0,false)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused, a.descriptorSizes('lookup'),"
          "Object.keys(a.descriptorSizes()).length, Object.keys(a.descriptorSizes('matrix')).length]))" % addon)
    t, refused, sizes, old, matrix = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert (t, refused) == ("function", 4)
    assert sizes == {"lookup": 64, "lookupResult": 24, "none": 0xffffffff} and old == 7 and matrix == 5
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_js_lookup_host_args():
    """CPU: the host-only argument checks of js/parallel.mjs refuse what the Python twin refuses"""
    js = ("import('%s').then((m)=>{ const f={handle:1,n:64,kind:'scalars'}; const t={handle:2,n:16,kind:'scalars'};"
          "const o={handle:3,n:40,kind:'scalars'}; const p={handle:4,n:64,kind:'points'}; let ok=0, refused=0;"
          "const g=(c,tb,op)=>JSON.stringify(m.lookupArgs(c,tb,op));"
          "const good=[()=>g(f,t)==='{\"n\":64,\"tableN\":16}', ()=>g(f,t,{firstColumn:60,firstTable:15})==='{\"n\":4,\"tableN\":1}',"
          "()=>g(f,t,{n:10,tableN:4,out:o,firstOut:36,positions:true})==='{\"n\":10,\"tableN\":4}',"
          "()=>g(f,f,{firstColumn:8,n:20,tableN:16})!==null, ()=>g(f,f,{firstColumn:8,n:8,firstTable:16,tableN:8,out:f,firstOut:0})!==null,"
          "()=>g(f,f,{firstColumn:8,n:8,firstTable:16,tableN:8,out:f,firstOut:24})!==null, ()=>g(f,t,{firstColumn:20,n:10,tableN:4,out:f,firstOut:30})!==null];"
          "const bad=[()=>g(null,t), ()=>g(f,null), ()=>g(p,t), ()=>g(f,p), ()=>g(f,t,{out:p}), ()=>g(f,t,{positions:1}), ()=>g(f,t,{n:0}),"
          "()=>g(f,t,{tableN:0}), ()=>g(f,t,{n:65}), ()=>g(f,t,{tableN:17}), ()=>g(f,t,{n:1.5}), ()=>g(f,t,{firstColumn:64}), ()=>g(f,t,{firstColumn:-1}),"
          "()=>g(f,t,{firstTable:10,tableN:7}), ()=>g(f,t,{firstOut:1}), ()=>g(f,t,{out:o,firstOut:25}), ()=>g(f,t,{out:t}), ()=>g(f,t,{out:f}),"
          "()=>g(f,t,{firstTable:4,tableN:4,out:t,firstOut:1}), ()=>g(f,t,{firstTable:4,tableN:4,out:t,firstOut:7}),"
          "()=>g(f,t,{firstColumn:20,n:10,tableN:4,out:f,firstOut:17}), ()=>g(f,t,{firstColumn:20,n:10,tableN:4,out:{...f},firstOut:29})];"
          "for (const c of good) { if (c()) ok++; } for (const c of bad) { try { c(); } catch (e) { refused++; } }"
          "console.log(JSON.stringify([ok, refused, bad.length])); })" % os.path.join(ROOT, "js", "parallel.mjs"))
    ok, refused, nbad = json.loads(subprocess.check_output([NODE, "-e", js], text=True, cwd=ROOT))
    assert ok == 7 and refused == nbad == 22


def test_fixture_is_self_consistent():
    """CPU: the committed fixture has the structure the issue asks for and holds what Python integers say today"""
    fx = json.load(open(FIXTURE))
    q = S.order(fx["curve"])
    table, column = [int(v) for v in fx["table"]], [int(v) for v in fx["column"]]
    assert fx["curve"] == "bls12-377" and len(table) == 48 and len(column) == 200
    assert all(0 <= v < q for v in table + column) and {0, 1, q - 1} <= set(table)
    assert len(set(table)) < 48 and fx["missing"] >= 2 and fx["firstMissing"] not in (None, 0)
    m, positions, info = L.model(table, column)
    assert [int(v) for v in fx["multiplicities"]] == m and fx["positions"] == positions
    assert {k: fx[k] for k in ("missing", "firstMissing", "distinct")} == info
    assert sum(m) + info["missing"] == 200 and 0 in m


@pytest.mark.gpu
def test_js_lookup(addon):
    """GPU: node runs the lookup with positions, without, and into a range of the inputs' own array on the fixture"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    info = {k: fx[k] for k in ("missing", "firstMissing", "distinct")}
    assert got["multiplicities"] == fx["multiplicities"] and got["positions"] == fx["positions"]
    assert got["info"] == info and got["plain"] == info
    assert got["intoRange"] == fx["table"] + fx["column"] + fx["multiplicities"]
    assert got["sizes"] and got["refused"]
