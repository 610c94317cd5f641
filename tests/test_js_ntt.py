"""Number-theoretic transforms through the JavaScript host (js/parallel.mjs ntt / rootOfUnity / nttArgs over
napi/msmz_napi.c), and the parity of the two hosts' argument checks on one table."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

import ntt_util as N
import scalar_ops_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SCRIPT = os.path.join(ROOT, "js", "scripts", "msm-ntt.mjs")
ARGS_SCRIPT = os.path.join(ROOT, "js", "scripts", "ntt-args.mjs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ntt_js_fixture.json")
ARGS_TABLE = os.path.join(ROOT, "tests", "golden", "ntt_args_parity.json")
VALUES = ("roots", "forward", "coset", "cosetInverse", "short", "mirrored")


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_ntt_fixture", os.path.join(ROOT, "tests", "golden", "make_ntt_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_js_ntt_addon_and_scripts(addon):
    """CPU: the addon exports the two calls, scalarsRootOfUnity answers without a device, both refuse bad arguments, and
    the scripts parse"""
    js = ("const a=require(%r); const t=[a.scalarsNtt,a.scalarsRootOfUnity].map((f)=>typeof f); let refused=0;"
          "for (const f of [()=>a.scalarsNtt(), ()=>a.scalarsNtt(null,1,0,3,0,0,1,null,null,0,0), ()=>a.scalarsRootOfUnity(),"
          "()=>a.scalarsRootOfUnity(0,48), ()=>a.scalarsRootOfUnity(3,2), ()=>a.scalarsRootOfUnity(9,1)])"
          "{ try { f(); } catch (e) { refused++; } }"
          "const r=a.scalarsRootOfUnity(1,1); console.log(JSON.stringify([t, refused, r.length, r[0], r[31]]))" % addon)
    q = S.order("pallas")   # the 2nd root of unity is q - 1
    assert json.loads(subprocess.check_output([NODE, "-e", js], text=True)) == [["function"] * 2, 6, 32, (q - 1) & 255, (q - 1) >> 248]
    for script in (SCRIPT, ARGS_SCRIPT):
        subprocess.run([NODE, "--check", script], check=True)


def test_fixture_is_self_consistent(maker):
    """CPU: the committed fixture is what its maker builds from Python integers today, and it holds the planted values"""
    fx = json.load(open(FIXTURE))
    assert fx == maker.build()
    label = fx["curve"]
    q, n, m = S.order(label), 1 << fx["logN"], 1 << fx["small"]
    x = [int(v) for v in fx["x"]]
    assert len(x) == m and {0, 1, q - 1, S.low_words_full(q)} <= set(x[:8])
    w, ws, g = N.root(label, fx["logN"]), N.root(label, fx["small"]), int(fx["shift"])
    long = maker.long_input(q, x, n)
    assert {0, n // 2, n - 1} <= set(fx["samples"]) and len(fx["forward"]) == len(fx["samples"])
    for k, v in zip(fx["samples"], fx["forward"]):
        b, acc = pow(w, k, q), 0
        for c in reversed(long):
            acc = (acc * b + c) % q
        assert int(v) == acc, k
    coset = [int(v) for v in fx["coset"]]
    assert coset[3] == sum(v * pow(g * pow(ws, 3, q), i, q) for i, v in enumerate(x)) % q
    plain = N.transform(q, x, m, ws)
    assert [int(v) for v in fx["mirrored"]] == [plain[(m - k) % m] for k in range(m)]
    assert N.transform(q, [int(v) for v in fx["cosetInverse"]], m, ws, shift=g) == x
    assert len(fx["short"]) == 2 * m and [int(v) for v in fx["roots"]][:2] == [1, q - 1]


def test_args_table_python(maker):
    """CPU: ntt_args gives what the committed table says, row by row; the table has good and bad rows of every kind"""
    table = json.load(open(ARGS_TABLE))
    assert table == maker.build_args()
    kinds = [next(iter(outcome)) + ":" + str(outcome.get("err")) for _, _, outcome in table["cases"]]
    assert kinds.count("ok:None") >= 10 and kinds.count("err:TypeError") >= 15 and kinds.count("err:ValueError") >= 30


def test_args_table_javascript(addon):
    """CPU: nttArgs of js/parallel.mjs gives the same outcome as the Python twin on every row of the table"""
    table = json.load(open(ARGS_TABLE))
    out = subprocess.run([NODE, ARGS_SCRIPT, ARGS_TABLE], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    want = [[label, outcome] for label, _, outcome in table["cases"]]
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not bad, bad[:5]


@pytest.mark.gpu
def test_js_ntt(addon):
    """GPU: node runs the transforms on the fixture's scalars; every value is the fixture's, the round trips, the
    in-place transform and the polynomial product hold, the bad calls throw"""
    fx = json.load(open(FIXTURE))
    out = subprocess.run([NODE, SCRIPT, FIXTURE], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for key in VALUES:
        assert got[key] == fx[key], key
    assert got["roundTrip"] and got["inPlace"] and got["product"] and got["refused"]
