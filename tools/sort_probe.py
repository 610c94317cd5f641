"""Development aid: runs only the bucket sort (test hook msmz_test_sort) on 2^log2n random BLS12-377 scalars, for the
workgroup timelines of a -DMSMZ_TRACE build (tools/wg_timeline.py); msmz_test_sort_ex names the full geometry.
usage: sort_probe.py [log2n] [c] [glv]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np

import msm_zprize_amd as m
from msm_zprize_amd import _native

log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
c = int(sys.argv[2]) if len(sys.argv) > 2 else 17
glv = int(sys.argv[3]) if len(sys.argv) > 3 else 0
n = 1 << log2n
m.startThreads()
curve = m.Weierstrass.create(m.curves.BY_LABEL["bls12-377"])
rng = np.random.default_rng(5)
raw = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
raw.reshape(n, 32)[:, 31] &= 0x0F   # below the group order (top byte of r is 0x12)
geom = (C.c_uint32 * 8)()
lib = _native.lib()
for _ in range(3):
    st = lib.msmz_test_sort(curve._ctx, raw.ctypes.data_as(C.c_char_p), n, c, glv, 0, geom, None, 0, None, 0)
    assert st == 0, st
print("geometry c K Keff L nb E maxb spread:", list(geom))
words = (C.c_uint32 * len(_native.TEST_SORT_GEOM))()
args = _native.MsmzTestSortArgs(scalars_le32=raw.ctypes.data_as(C.c_void_p), n=n, nprob=1, c=c, glv=glv,
                                geom=C.cast(words, C.c_void_p), geom_cap=len(words))
assert lib.msmz_test_sort_ex(curve._ctx, C.byref(args)) == 0
print("layout:", dict(zip(_native.TEST_SORT_GEOM, words)))
