"""The MSM planner (msm_zprize_amd/csrc/plan.h) needs no GPU: tests/native/plan_test.cpp replays it against a frozen
copy of the planning code engine.h had before it moved there, and asserts the planner's invariants."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_header_is_host_only():
    """plan.h compiles with a plain host compiler: no HIP runtime"""
    hdr = os.path.join(ROOT, "msm_zprize_amd", "csrc", "plan.h")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", hdr])


def test_planner_output_replays_the_engine_planner():
    """make_plan, the sort layout, plan chunks, the 2-D split, batch_size and precompute_params equal the engine's former
    planning code for every field of the planner's output and every size class, window size, GLV choice, batch,
    precomputed set and planning knob; folded plans and accepted precomputed sets take the two-level sort.  (The run
    state the engine keeps per call, engine.h Run, is not planner output and not part of a Plan.)"""
    src = os.path.join(ROOT, "tests", "native", "plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "native", "plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert "mismatches 0" in r.stdout, r.stdout
    shapes = int(r.stdout.split("shapes ")[1].split()[0])
    assert shapes >= 31650237, r.stdout   # the sweep compares no fewer shapes than when Plan still held run state
