"""The sumcheck step through the JavaScript host (js/parallel.mjs sumcheckStep / sumcheckProve over napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

import scalar_ops_util as S
import sumcheck_step_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-sumcheck-step.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "sumcheck_step_js_fixture.json")
KEYS = ("steps", "tables", "last", "lastTables", "polys", "claim")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_script_parses(addon):
    """CPU: the addon exports the call and allocScalars, they refuse bad arguments without a device, the descriptor sizes
    are the header's and the call without a family answers what it did, and the script parses"""
    js = ("const a=require(%r); const t=[a.scalarsSumcheckStep,a.allocScalars].map((f)=>typeof f);"
          "let refused=0; const b=Buffer.alloc(64);"
          "for (const f of [()=>a.scalarsSumcheckStep(), ()=>a.scalarsSumcheckStep(null,b,null,1,1,b,b,b,1,0,b.subarray(0,32)),"
          "()=>a.scalarsSumcheckStep(null,b,b,1,1,b,b,b,1,0,null), ()=>a.allocScalars(null,4)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused, a.descriptorSizes('sumcheckStep'),"
          " a.descriptorSizes()]))" % addon)
    t, refused, sizes, plain = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert (t, refused) == (["function"] * 2, 4)
    assert sizes == {"sumcheckStep": 48, "sumcheckTable": 16, "sumcheckTerm": 16}
    assert plain == {"mleBind": 40, "sumcheck": 32, "sumcheckTable": 16, "sumcheckTerm": 16, "maxTables": 6, "maxDegree": 4,
                     "maxTerms": 8}
    subprocess.run([NODE, "--check", SCRIPT], check=True)


# what sumcheck_step_args refuses and accepts in tests/test_sumcheck_step_cpu.py, in JavaScript's notation: f and d of 64
# entries, g of 100
_GOOD = ["[[f,[g,36]],[[null,3],[q-1n,2]],5n,{out:[d,[g,4]]}]", "[[f],one,5n,{}]", "[[[f,0]],one,5n,{nVars:5,out:[[f,0]]}]",
         "[[[f,16]],one,5n,{nVars:4,out:[[f,0]]}]", "[[[f,16]],one,5n,{nVars:4,out:[[f,32]]}]", "[[f,f],[[1n,3]],5n,{out:[d,[g,0]],low:true}]",
         "[[[f,0],[f,32]],one,5n,{nVars:5}]", "[[[f,2]],one,5n,{nVars:1}]", "[[f],one,0n,{}]", "[[f],one,q-1n,{}]"]
_BAD = ["[[f],one,5,{}]", "[[f],one,null,{}]", "[[f],one,5n,{out:7}]", "[[f],one,5n,{out:[7]}]", "[[f],one,5n,{out:[[d,0,0]]}]",
        "[[f],one,5n,{low:1}]", "[null,one,5n,{}]", "[[f],[1],5n,{}]",
        "[[f],one,q,{}]", "[[f],one,-1n,{}]", "[[f],one,5n,{out:[]}]", "[[f],one,5n,{out:[d,d]}]", "[[f,f],one,5n,{out:[d]}]",
        "[[f],one,5n,{out:[[d,33]]}]", "[[f],one,5n,{out:[[d,-1]]}]", "[[f],one,5n,{out:[[g,69]]}]", "[[f],one,5n,{nVars:0}]",
        "[[f],one,5n,{nVars:7}]", "[[g],one,5n,{}]", "[[f],[[1n,2]],5n,{}]", "[[f],[[q,1]],5n,{}]", "[[],one,5n,{}]",
        "[[f],one,5n,{out:[[f,32]]}]", "[[f],one,5n,{out:[[f,1]]}]", "[[f],one,5n,{out:[[f,31]]}]",
        "[[[f,16]],one,5n,{nVars:4,out:[[f,9]]}]", "[[[f,16]],one,5n,{nVars:4,out:[[f,24]]}]", "[[[f,16]],one,5n,{nVars:4,out:[[f,31]]}]",
        "[[f],one,5n,{low:true}]", "[[f],one,5n,{low:true,out:[f]}]", "[[[f,16]],one,5n,{nVars:4,low:true,out:[[f,16]]}]",
        "[[f,f],[[1n,3]],5n,{}]", "[[f,d],one,5n,{out:[[d,0],[g,0]]}]", "[[f,d],one,5n,{out:[[g,0],[f,0]]}]",
        "[[[f,0],[f,16]],one,5n,{nVars:5}]", "[[f,d],one,5n,{out:[[g,0],[g,31]]}]", "[[f,d],one,5n,{out:[g,g]}]",
        "[[f,d,g],one,5n,{nVars:6,out:[[g,64],[g,0],[d,0]]}]", "[[f],one,5n,{out:[[same,3]]}]"]


def test_js_host_args():
    """CPU: the host-only argument checks of js/parallel.mjs accept and refuse what the Python twin does in
    tests/test_sumcheck_step_cpu.py, case for case, with a TypeError where Python raises one"""
    js = ("import('%s').then((m)=>{ const q=1009n; const f={handle:1,n:64,kind:'scalars'}, g={handle:2,n:100,kind:'scalars'},"
          "d={handle:3,n:64,kind:'scalars'}, same={handle:1,n:64,kind:'scalars'}, one=[[null,1]];"
          "const run=(a)=>{ try { const t=m.sumcheckStepArgs(a[0],a[1],a[2],a[3],q); return ['ok',t.nVars,t.degree,t.flags,t.out===null?null:t.out.map((o)=>[o[0].handle,o[1]])]; }"
          " catch (e) { return [e instanceof TypeError ? 'type' : 'value']; } };"
          "console.log(JSON.stringify([[%s].map(run), [%s].map(run)])); })"
          % (os.path.join(ROOT, "js", "parallel.mjs"), ",".join(_GOOD), ",".join(_BAD)))
    good, bad = json.loads(subprocess.check_output([NODE, "-e", js], text=True, cwd=ROOT))
    assert [g[0] for g in good] == ["ok"] * len(_GOOD), good
    assert all(b[0] in ("type", "value") for b in bad), [c for c, b in zip(_BAD, bad) if b[0] == "ok"]
    assert [b[0] for b in bad[:8]] == ["type"] * 8 and [b[0] for b in bad[8:]] == ["value"] * (len(_BAD) - 8)
    assert good[0] == ["ok", 6, 2, 0, [[3, 0], [2, 4]]] and good[5][3] == 1 and good[7] == ["ok", 1, 0, 0, None]


def test_fixture_is_self_consistent():
    """CPU: the committed fixture holds the planted values and what Python integers say today"""
    fx = json.load(open(FIXTURE))
    q = S.order(fx["curve"])
    v = fx["nVars"]
    assert fx["curve"] == "bls12-377" and v == 6 and len(fx["tables"]) == 3 and len(fx["challenges"]) == v
    tables = [[int(e) for e in t] for t in fx["tables"]]
    rs = [int(e) for e in fx["challenges"]]
    terms = [(None if c is None else int(c), m) for c, m in fx["terms"]]
    assert all(len(t) == 1 << v and all(0 <= e < q for e in t) for t in tables) and all(0 <= e < q for e in rs)
    assert {0, 1, q - 1, S.low_words_full(q)} <= set(tables[0]) and {1, q - 1} <= set(rs)
    assert sorted(bin(m).count("1") for _, m in terms) == [1, 2]            # mixed degree
    for key, low in (("high", False), ("low", True)):
        want = fx[key]
        cur = tables
        for k in range(3):
            cur, degree, values = U.step(cur, terms, rs[k], q, low)
            assert degree == 2 and [int(e) for e in want["steps"][k]] == values
        assert [[int(e) for e in t] for t in want["tables"]] == cur and len(cur[0]) == 8
        bound, degree, values = U.step([t[:2] for t in cur], terms, rs[3], q, low)
        assert degree == 0 and [int(want["last"])] == values and [int(e) for e in want["lastTables"]] == [b[0] for b in bound]
        polys, _, claim, _ = U.prove(tables, terms, q, lambda values, it=iter(rs): next(it), low)
        assert [[int(e) for e in p] for p in want["polys"]] == polys and int(want["claim"]) == claim
        assert polys[1] == [int(e) for e in want["steps"][0]]


@pytest.mark.gpu
def test_js_sumcheck_step(addon):
    """GPU: node runs three steps, the last-variable step and a whole protocol on the fixture in both orders; every value
    is the fixture's"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for order in ("high", "low"):
        for key in KEYS:
            assert got[order][key] == fx[order][key], (order, key)
    assert got["sizes"] and got["refused"]
