"""msmz_test_poison (include/msmz_test.h) fills every device scratch buffer of a context.  Which buffers those are is said
once, by the each_scratch visitors of the classes that own them (csrc/sets_core.h, the five family stages that
resident.h holds, sort.h, reduce.h, engine.h).  This test
keeps that enumeration complete: every DevBuf member declared in csrc/*.h is either named in a visitor of its own file or
listed below as kept on purpose, so a scratch buffer added without the hook fails here, without a GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "msm_zprize_amd", "csrc")

# (file, name): device buffers that hold data which is valid across calls, or that no context owns
KEPT = {
    ("store.h", "mem"),        # Handle::mem: the records of a resident set
    ("store.h", "form"),       # Handle::form[2]: the two sorted forms of a sparse matrix
    ("ntt_ops.h", "mem"),      # NttTwiddles::mem: the twiddle cache
    ("point_ops.h", "mem"),    # FixedTable::mem: the fixed-base table cache
    ("resident.h", "gen_table_"),   # the generator's window table, built once by the first random_points
    # function-local buffers of the stage hooks, freed on every return
    ("test_hooks.h", "d_pts"), ("test_hooks.h", "d_off"), ("test_hooks.h", "d_refs"),
}

DECL = re.compile(r"^\s*DevBuf\s+([^;()]*);", re.M)           # `DevBuf a_, b_[4], c_;` (no references, no functions)
VISITOR = re.compile(r"void\s+each_scratch\s*\(\s*Fn\s+f\s*\)\s*\{(.*?)\n  \}", re.S)


def _declared(text):
    names = []
    for m in DECL.finditer(text):
        for part in m.group(1).split(","):
            name = re.match(r"\s*(\w+)", part).group(1)
            names.append(name)
    return names


def _visited(text):
    names = set()
    for m in VISITOR.finditer(text):
        body = m.group(1)
        loops = re.findall(r"for\s*\(DevBuf&\s*(\w+)\s*:\s*(\w+)\)", body)       # for (DevBuf& b : red_) f(b);
        names |= set(re.findall(r"\bf\((\w+)\)", body)) - {var for var, _ in loops}   # f(desc_)
        names |= {array for _, array in loops}
    return names


def _headers():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))


def test_the_scan_sees_the_declarations():
    """the patterns find what the code is known to declare: arrays, lists on one line, members of nested structs"""
    found = {(f, n) for f in _headers() for n in _declared(open(os.path.join(CSRC, f)).read())}
    for want in (("reduce.h", "red_"), ("reduce.h", "f2desc_"), ("sort.h", "partials_"), ("sort.h", "packed_"),
                 ("engine.h", "slots_"), ("engine.h", "segs_"), ("ntt_ops.h", "ntt_coset_"), ("sets_core.h", "meta_"),
                 ("store.h", "form"), ("ntt_ops.h", "mem"), ("point_ops.h", "mem"), ("resident.h", "gen_table_"),
                 ("test_hooks.h", "d_refs")):
        assert want in found, want
    assert _declared("  DevBuf a_, b_[4], c_;   // x\n  DevBuf& r;\n  DevBuf f();\n") == ["a_", "b_", "c_"]
    assert _visited("  void each_scratch(Fn f) {\n    for (DevBuf& b : red_) f(b);\n    f(x_), f(y_);\n  }\n") == {"red_", "x_", "y_"}


def test_every_device_buffer_is_poisoned_or_kept():
    missing, visited_all = [], set()
    for f in _headers():
        text = open(os.path.join(CSRC, f)).read()
        visited = _visited(text)
        visited_all |= {(f, n) for n in visited}
        declared = _declared(text)
        for name in declared:
            if name not in visited and (f, name) not in KEPT:
                missing.append((f, name))
        # a visitor names only what its own file declares (the engine's also calls the visitors of its stages)
        assert visited <= set(declared), (f, visited - set(declared))
    assert not missing, f"device buffers that msmz_test_poison does not reach and the kept list does not name: {missing}"
    # nothing is both filled and kept, and the kept list names only what exists
    declared_all = {(f, n) for f in _headers() for n in _declared(open(os.path.join(CSRC, f)).read())}
    assert not (KEPT & visited_all)
    assert KEPT <= declared_all, KEPT - declared_all
    # 2 (sets_core.h) + 1 (point_ops.h) + 2 (scalar_ops.h) + 2 (ntt_ops.h) + 1 (matrix_ops.h) + 3 (lookup_ops.h)
    # + 10 (sort.h) + 4 names (reduce.h: red_[4] is one) + 6 (engine.h)
    assert len(visited_all) >= 31
    # every buffer of the resident sets is visited in the file that owns it, and resident.h itself has none to visit
    for want in (("sets_core.h", "stage_"), ("sets_core.h", "meta_"), ("point_ops.h", "check_"), ("scalar_ops.h", "sdot_"),
                 ("scalar_ops.h", "sscan_"), ("ntt_ops.h", "ntt_scratch_"), ("ntt_ops.h", "ntt_coset_"),
                 ("matrix_ops.h", "mat_carry_"), ("lookup_ops.h", "lookup_slots_"), ("lookup_ops.h", "lookup_count_"),
                 ("lookup_ops.h", "lookup_res_")):
        assert want in visited_all, want
    assert not {n for f, n in visited_all if f == "resident.h"}


def test_the_kept_names_are_the_members_they_are_meant_to_be():
    """the kept list goes by file and name, and `mem` is a name that a new scratch buffer could take: the file of the
    file of each cache declares it exactly once, inside the cache entry, and the handle's file declares mem and form once"""
    for f, struct in (("ntt_ops.h", "NttTwiddles"), ("point_ops.h", "FixedTable")):
        text = open(os.path.join(CSRC, f)).read()
        assert _declared(text).count("mem") == 1, f
        assert re.search(r"struct\s+%s\s*\{[^{}]*?^\s*DevBuf\s+mem;" % struct, text, re.M), struct
    assert _declared(open(os.path.join(CSRC, "resident.h")).read()) == ["gen_table_"]
    text = open(os.path.join(CSRC, "store.h")).read()
    assert sorted(_declared(text)) == ["form", "mem"]
    assert re.search(r"struct\s+Handle\s*\{[^{}]*?^\s*DevBuf\s+mem;[^{}]*?^\s*DevBuf\s+form\[2\];", text, re.M)
    text = open(os.path.join(CSRC, "test_hooks.h")).read()
    assert sorted(set(_declared(text))) == ["d_off", "d_pts", "d_refs"]
    for m in DECL.finditer(text):   # function-local: deeper than a member's two spaces
        assert m.group(0).split("\n")[-1].startswith("    "), m.group(0)


def test_the_engine_visits_its_stages():
    """Engine::each_scratch reaches the resident sets', the sort's and the reduction's lists, so one call fills all"""
    text = open(os.path.join(CSRC, "engine.h")).read()
    body = VISITOR.search(text).group(1)
    for call in ("Base::each_scratch(f)", "sort_.each_scratch(f)", "reduce_.each_scratch(f)"):
        assert call in body, call


def test_the_resident_sets_visit_their_stages():
    """ResidentSets::each_scratch reaches the core's list and that of each of its five stages"""
    text = open(os.path.join(CSRC, "resident.h")).read()
    body = VISITOR.search(text).group(1)
    for call in ("Core::each_scratch(f)", "point_ops_.each_scratch(f)", "scalar_ops_.each_scratch(f)",
                 "ntt_ops_.each_scratch(f)", "matrix_ops_.each_scratch(f)", "lookup_ops_.each_scratch(f)"):
        assert call in body, call
    for f in ("sets_core.h", "point_ops.h", "scalar_ops.h", "ntt_ops.h", "matrix_ops.h", "lookup_ops.h"):
        assert len(VISITOR.findall(open(os.path.join(CSRC, f)).read())) == 1, f
