"""msmz_check_points over point sets imported from device tensors.  Runs in a child process of its own
(tests/test_check_points_gpu.py starts it), for the reason tests/import_gpu_cases.py gives: torch carries its own copy of
the HIP runtime, so it is imported here before anything loads libmsmz.so."""
import torch as _torch_first  # noqa: F401  (before libmsmz.so: one HIP runtime per process)

import pytest

import check_points_util as U
from oracle import params as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    import msm_zprize_amd as m
    m.startThreads()
    return m


@pytest.mark.parametrize("label", U.ALL)
def test_device_tensor_route(mod, label):
    """the planted points through msmz_upload_points and, from a device tensor, through msmz_import_points (canonical and
    Montgomery, infinity flags in a device tensor): the same verdict bytes, and the planted ones are the oracle's"""
    import torch
    params = mod.curves.BY_LABEL[label]
    curve = (mod.Weierstrass if params["kind"] == "weierstrass" else mod.TwistedEdwards).create(params)
    try:
        n = 1 << 12
        gen = curve.Parallel.randomPointsFast(n, 77)
        good = [{"x": p["x"], "y": p["y"], "isZero": bool(p["isZero"])} for p in curve.Affine.toBigints(gen)]
        gen.free()
        pts, where = U.planted_set(label, good)
        data, inf = U.encode(P.CURVES[label], pts)
        up = curve.Parallel.pointsFromBytes(data, n, inf)
        ref = curve.Parallel.checkPoints(up, verdicts=True)
        up.free()
        for i in where:
            assert ref.verdicts[i] == U.verdict(P.CURVES[label], pts[i]), i
        assert not ref.ok and sum(1 for v in ref.verdicts if v) == ref.offCurve + ref.offSubgroup
        assert all(ref.verdicts[i] == 0 for i in range(n) if i not in set(where))
        flags = None if inf is None else torch.frombuffer(bytearray(inf), dtype=torch.uint8).to("cuda")
        for montgomery in (False, True):
            raw = U.encode(P.CURVES[label], pts, montgomery)[0]
            t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(n, 2 * params["fe_bytes"]).to("cuda")
            arr = curve.Parallel.pointsFromTensor(t, montgomery=montgomery, is_inf=flags)
            got = curve.Parallel.checkPoints(arr, verdicts=True)
            assert got.verdicts == ref.verdicts, montgomery
            assert (got.ok, got.offCurve, got.offSubgroup, got.firstBad) == (ref.ok, ref.offCurve, ref.offSubgroup, ref.firstBad)
            arr.free()
            with pytest.raises(ValueError, match="firstBad = %d" % ref.firstBad):
                curve.Parallel.pointsFromTensor(t, montgomery=montgomery, is_inf=flags, check="subgroup")
    finally:
        curve.close()
