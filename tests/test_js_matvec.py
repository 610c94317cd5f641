"""Sparse matrices against resident scalar arrays through the JavaScript host (js/parallel.mjs sparseMatrix / matVec over
napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

import matrix_util as M
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-matvec.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "matvec_js_fixture.json")
MODES = ("mx", "mty", "mxOnes", "mtyOnes")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def test_js_matvec_script_parses(addon):
    """CPU: the addon exports the three calls, they refuse bad arguments without a device, its descriptor sizes and flags
    are the header's -- asked for by family, the call without an argument answering what it did -- and the script parses"""
    js = ("const a=require(%r); const t=[a.matrixCreate,a.matrixInfo,a.matrixMul].map((f)=>typeof f);"
          "let refused=0; const b=Buffer.alloc(64);"
          "for (const f of [()=>a.matrixCreate(), ()=>a.matrixCreate(null,b,b,4,0,0,4,4,1), ()=>a.matrixInfo(null,1),"
          "()=>a.matrixMul(null,1,1,0,0,0,0)])"
          "{ try { f(); } catch (e) { refused++; } } console.log(JSON.stringify([t, refused, a.descriptorSizes('matrix'), Object.keys(a.descriptorSizes()).length]))"
          % addon)
    t, refused, sizes, old = json.loads(subprocess.check_output([NODE, "-e", js], text=True))
    assert (t, refused) == (["function"] * 3, 4)
    assert sizes == {"sparse": 56, "matvec": 32, "matRows": 1, "matCols": 2, "matvecTranspose": 1} and old == 7
    subprocess.run([NODE, "--check", SCRIPT], check=True)


def test_js_matvec_host_args():
    """CPU: the host-only argument checks of js/parallel.mjs refuse what the Python twins refuse"""
    js = ("import('%s').then((m)=>{ const x={handle:1,n:64,kind:'scalars'}; const y={handle:2,n:8,kind:'scalars'};"
          "const M={handle:9,shape:[3,5],orientations:'rows',kind:'matrix'}; const B={...M,orientations:'both'}; let ok=0, refused=0;"
          "const s=(r,c,v,o)=>m.sparseMatrixArgs(r,c,v,{shape:[2,2],...o});"
          "const good=[()=>s([0,1],[1,0],null,{}), ()=>s(Uint32Array.from([0,1]),[1,0],x,{firstValue:62,orientations:'both'}),"
          "()=>m.matVecArgs(M,x,{}), ()=>m.matVecArgs(B,y,{transpose:true,firstX:5}), ()=>m.matVecArgs(M,x,{firstX:3,out:x,firstOut:0}),"
          "()=>m.matVecArgs(M,x,{firstX:3,out:x,firstOut:8}), ()=>m.matVecArgs(M,x,{out:y,firstOut:5})];"
          "const bad=[()=>s([0,2],[1,0],null,{}), ()=>s([0,1],[1,-1],null,{}), ()=>s([0,1],[1],null,{}), ()=>s([],[],null,{}),"
          "()=>s([0,1.5],[1,0],null,{}), ()=>s([0,1],[1,0],null,{orientations:'row'}), ()=>s([0,1],[1,0],x,{firstValue:63}),"
          "()=>s([0,1],[1,0],null,{firstValue:1}), ()=>s([0,1],[1,0],null,{shape:[0,2]}), ()=>s([0,1],[1,0],7,{}),"
          "()=>m.matVecArgs(M,x,{transpose:true}), ()=>m.matVecArgs(x,x,{}), ()=>m.matVecArgs(M,M,{}), ()=>m.matVecArgs(M,x,{firstX:60}),"
          "()=>m.matVecArgs(M,x,{out:x}), ()=>m.matVecArgs(M,x,{firstX:3,out:x,firstOut:1}), ()=>m.matVecArgs(M,x,{firstX:3,out:x,firstOut:7}),"
          "()=>m.matVecArgs(M,x,{out:y,firstOut:6}), ()=>m.matVecArgs(M,x,{firstOut:1}), ()=>m.matVecArgs({...M,handle:null},x,{})];"
          "for (const g of good) { g(); ok++; } for (const g of bad) { try { g(); } catch (e) { refused++; } }"
          "console.log(JSON.stringify([ok, refused, bad.length])); })" % os.path.join(ROOT, "js", "parallel.mjs"))
    ok, refused, nbad = json.loads(subprocess.check_output([NODE, "-e", js], text=True, cwd=ROOT))
    assert ok == 7 and refused == nbad == 20


def test_fixture_is_self_consistent():
    """CPU: the committed fixture has the structure the issue asks for and holds what Python integers say today"""
    fx = json.load(open(FIXTURE))
    q = S.order(fx["curve"])
    n_rows, n_cols = fx["shape"]
    rows, cols = fx["rows"], fx["cols"]
    ints = lambda key: [int(e) for e in fx[key]]   # noqa: E731
    vals, x, y = ints("values"), ints("x"), ints("y")
    assert fx["curve"] == "bls12-377" and (n_rows, n_cols) == (40, 48) and len(rows) == len(cols) == len(vals) == 150
    assert len(x) == n_cols and len(y) == n_rows and all(0 <= e < q for e in vals + x + y)
    assert len(set(range(n_rows)) - set(rows)) >= 1 and len(set(range(n_cols)) - set(cols)) >= 1     # an empty row and column
    assert len(set(zip(rows, cols))) < 150 and rows != sorted(rows)                                  # a duplicate; shuffled
    assert {0, 1, q - 1} <= set(vals) and {0, q - 1} <= set(x) and {0, q - 1} <= set(y)
    assert ints("mx") == M.matvec(rows, cols, vals, x, n_rows, q)
    assert ints("mty") == M.matvec(rows, cols, vals, y, n_cols, q, transpose=True)
    assert ints("mxOnes") == M.matvec(rows, cols, None, x, n_rows, q)
    assert ints("mtyOnes") == M.matvec(rows, cols, None, y, n_cols, q, transpose=True)


@pytest.mark.gpu
def test_js_matvec(addon):
    """GPU: node runs both orientations with values and without on the fixture; every value is the fixture's"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert got[mode] == fx[mode], mode
    assert got["intoRange"] == fx["x"] + fx["mx"]
    assert got["info"] == {"nRows": 40, "nCols": 48, "nnz": 150, "flags": 3}
    assert got["sizes"] and got["refused"]
