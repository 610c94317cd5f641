"""The argument checks of the JavaScript host (js/parallel.mjs) against their record from before the host bindings were
restructured, and the sizes of the N-API addon's output Buffers (napi/msmz_napi.c)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
ARGS = os.path.join(ROOT, "js", "scripts", "msm-args.mjs")
SIZES = os.path.join(ROOT, "js", "scripts", "addon-sizes.mjs")
GOLDEN = os.path.join(ROOT, "tests", "golden", "js_args_parity.json")

# The messages whose wording was unified on purpose: innerProduct's faults of firstX / firstY now go through scanRanges
# like every other operation's and say what is wrong with the index.  label -> the new text.
REWORDED = {f"dot {name}={v}": f"innerProduct: {name} = {v} but the array holds {size}"
            for name, size in (("firstX", 16), ("firstY", 8)) for v in ("-1", "1.5", "1", "true", "null", "16")}
REWORDED["dot firstY=8"] = "innerProduct: firstY = 8 but the array holds 8"
REWORDED["dot double"] = "innerProduct: firstX = 16 but the array holds 16"
REWORDED["dot firstY without"] = "innerProduct: firstY = 1 without the array it indexes"


@pytest.fixture(scope="module")
def addon():
    from msm_zprize_amd import build
    build.build(verbose=False)
    return build.build_napi(verbose=False)


def _node(script, *args):
    out = subprocess.run([NODE, script] + list(args), capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_scripts_parse_and_the_record_is_whole(addon):
    """CPU: both scripts parse; the record holds every Parallel.* call of the issue, accepted and refused cases, and
    every reworded label is a fault that innerProduct reported before, in its shorter wording"""
    for s in (ARGS, SIZES):
        subprocess.run([NODE, "--check", s], check=True)
    rows = json.load(open(GOLDEN))
    labels = [r[0] for r in rows]
    assert len(set(labels)) == len(labels) >= 300
    for prefix in ("mul ", "comb ", "dot ", "pow ", "rec ", "inv ", "check ", "pre ", "seg ", "batch ", "pfb ", "pfb ptr ", "sfb ",
                   "sfb ptr "):
        mine = [r for r in rows if r[0].startswith(prefix)]
        assert any(r[1] for r in mine) and any(not r[1] for r in mine), prefix
    by = {r[0]: r for r in rows}
    for label, text in REWORDED.items():
        old = by[label]
        assert old[1] and old[2] == "Error" and text.startswith(old[3]) and text != old[3]


def test_point_add_sizes_come_from_the_library(addon):
    """CPU, no device: pointAdd refuses (code "1") a feBytes that is not the curve's, an input Buffer shorter than the
    2 * fe_bytes the library reads, and a curve the library does not know; zero + zero is still zero"""
    rows = {label: (code, inf) for label, code, inf in _node(SIZES, "--cpu")["pointAdd"]}
    for label in ("feBytes 8 for a 48-byte curve", "a 4-byte input", "a 95-byte second input", "curve 9", "curve 9, feBytes 0",
                  "feBytes 32 for a 48-byte curve", "a short argument list"):
        assert rows[label] == ("1", None), (label, rows[label])
    assert rows["zero + zero"] == (None, True) and rows["zero + zero, 32-byte curve"] == (None, True)


@pytest.mark.gpu
def test_js_arguments_give_what_they_gave(addon):
    """GPU: js/scripts/msm-args.mjs on the code under test == tests/golden/js_args_parity.json (recorded on an MI355X at
    the commit before): every call throws or runs as it did, an error has the class it had and the message it had -- or
    the new text above, for innerProduct's unified wording"""
    want = json.load(open(GOLDEN))
    got = _node(ARGS)
    assert [r[0] for r in got] == [r[0] for r in want]
    bad = []
    for g, w in zip(got, want):
        text = REWORDED.get(w[0], w[3])
        if g[1] != w[1] or g[2] != w[2] or g[3] != text:
            bad.append((g, w))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.gpu
def test_addon_refuses_a_wrong_fe_bytes(addon):
    """GPU: on a BLS12-377 context of 8 points and 8 scalars, downloadPoints / msm / msmBatch / msmSegments of the addon
    with feBytes = 8 throw code "1"; with 48 they give what Parallel gives"""
    rep = _node(SIZES)
    assert rep["refused"] == {k: "1" for k in ("downloadPoints", "msm", "msmBatch", "msmSegments")}
    assert rep["same"] == {k: True for k in ("downloadPoints", "msm", "msmBatch", "msmSegments")}
