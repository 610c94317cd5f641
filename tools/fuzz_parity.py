"""The MSM option-space sweep from the command line (development aid, needs the GPU): the cases of
tests/msm_sweep_util.py -- the one definition of a case, also run by tests/test_msm_sweep_gpu.py -- for any seed, each
against the closed form, bit-exact, and against its predicted plan.  usage: fuzz_parity.py [cases=0 (all)] [seed=1]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import msm_sweep_util as U   # noqa: E402

limit = int(sys.argv[1]) if len(sys.argv) > 1 else 0
sweep = U.Sweep(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
todo = sweep.cases[:limit] if limit > 0 else sweep.cases
import msm_zprize_amd as m   # noqa: E402
m.startThreads()
t0 = time.time()
bad = 0
for k, case in enumerate(todo):
    try:
        sweep.run(case)
    except AssertionError as e:
        bad += 1
        print(f"case {case['id']}: {e}", flush=True)
    if k % 100 == 0:
        print(f"case {k} of {len(todo)}  ({time.time() - t0:.0f} s)", flush=True)
sweep.close()
print(f"{len(todo)} cases, {bad} failures, {time.time() - t0:.0f} s; observed {sweep.observed}")
sys.exit(1 if bad else 0)
