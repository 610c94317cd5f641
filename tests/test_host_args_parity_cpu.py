"""The argument checks of msm_zprize_amd/parallel.py give what they gave before the host bindings were restructured:
tests/golden/host_args_parity.json is the table of tests/golden/make_host_args_fixture.py (several hundred calls, good and
bad, double faults included) as recorded at the commit before; the same table is run here on the code under test.  Every
call throws or returns as it did, an exception has the class it had, a returned value is equal, and a message is the
recorded one -- or, for the faults whose wording was unified on purpose, the new text the case carries.  CPU only."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_args_parity.json")


@pytest.fixture(scope="module")
def table():
    spec = importlib.util.spec_from_file_location("make_host_args_fixture",
                                                  os.path.join(ROOT, "tests", "golden", "make_host_args_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cases = mod.cases()
    return cases, mod.record(cases), json.load(open(GOLDEN))


def test_the_table_is_the_recorded_one(table):
    cases, got, want = table
    assert sorted(got) == sorted(want) and len(want) >= 300
    refused = [k for k, v in want.items() if "err" in v]
    assert len(refused) >= 200 and len(want) - len(refused) >= 100
    # every fault of the range block is in the record, for each of the four functions that share it
    for fn in ("mul_points_args", "combine_scalars_args", "scalar_recurrence_args", "invert_scalars_args"):
        text = " ".join(v["err"][1] for k, v in want.items() if k.startswith(fn) and "err" in v)
        for part in ("without the array it indexes", "but the array holds", ": N = ", "entries ["):
            assert part in text, (fn, part)
        if fn != "mul_points_args":
            assert "overlaps the input range" in text, fn


def test_every_call_gives_what_it_gave(table):
    cases, got, want = table
    bad = []
    for label, _, new in cases:
        g, w = got[label], want[label]
        if ("err" in g) != ("err" in w):
            bad.append((label, g, w))
        elif "err" in w:
            if g["err"][0] != w["err"][0] or g["err"][1] != (new if new is not None else w["err"][1]):
                bad.append((label, g, w, new))
        elif g != w:
            bad.append((label, g, w))
    assert not bad, (len(bad), bad[:5])


def test_reworded_messages_are_the_listed_ones(table):
    """only mulPoints' "N does not fit" fault took the shared helper's wording; each such case was a fault before, too"""
    cases, _, want = table
    new = [(label, text) for label, _, text in cases if text is not None]
    assert new and all(label.startswith(("mul_points_args", "mulPoints")) for label, _ in new)
    for label, text in new:
        assert want[label]["err"][0] == "ValueError" and want[label]["err"][1] != text
        assert " of points that hold " in want[label]["err"][1] or " of scalars that hold " in want[label]["err"][1] or \
            " of addends that hold " in want[label]["err"][1]
        assert text.startswith("mulPoints: entries [") and " from first" in text
