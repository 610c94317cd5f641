"""The sweep of the resident-set operations on the GPU (tests/sets_sweep_util.py): every program of cases(1) against the
model, step by step -- the status and the scalars a call returns, the written range and its neighbours byte for byte,
every live set whole at the end.  Each program on a context of its own; the BLS12-377 programs again one after another
on one context, so that the grow-only scratch, the caches and the freed handles carry over from one program to the next;
one program under msmz_test_poison; one directed program on a context of two engines.  tests/test_sets_sweep_cpu.py holds
the list itself to its covering."""
import pytest

import sets_sweep_util as U
from test_scratch_poison_gpu import fresh, poison

pytestmark = pytest.mark.gpu

SEED = 1
SHARED = "bls12-377"


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


@pytest.fixture(scope="module")
def programs():
    return U.cases(SEED)


@pytest.mark.parametrize("label", U.CURVES)
def test_programs_each_on_a_fresh_context(mod, programs, label):
    mine = [p for p in programs if p["curve"] == label]
    assert mine
    for p in mine:
        with fresh(mod, label) as curve:
            U.run_program(curve, p)


def test_programs_one_after_another_on_one_context(mod, programs):
    """what a program leaves behind -- scratch that has grown, cached twiddle sets, freed handles and their memory -- is
    there when the next one starts; the expected bytes are those of the fresh-context runs"""
    mine = [p for p in programs if p["curve"] == SHARED]
    with fresh(mod, SHARED) as curve:
        for p in mine + mine[:2]:
            U.run_program(curve, p)


def test_a_program_under_poison(mod, programs):
    """the longest program of the shared curve once more with every scratch buffer, and every allocation to come, filled
    with 0xa5: the same bytes in every live set as the unarmed run (and as the model)"""
    p = max((p for p in programs if p["curve"] == SHARED), key=lambda p: len(p["steps"]))
    with fresh(mod, SHARED) as curve:
        plain = U.run_program(curve, p)
    with fresh(mod, SHARED) as curve:
        poison(curve, 0xa5)
        armed = U.run_program(curve, p)
    assert armed == plain and plain


def test_two_engines(mod):
    """devices = [0, 0] and n = 2^16 + 300: the operations csrc/multi.h runs per engine, chained on sets the program made,
    with the ranges on both sides of the block edge downloaded after every step"""
    p = U.two_engine_program()
    with fresh(mod, p["curve"], devices=[0, 0]) as curve:
        U.run_program(curve, p)
