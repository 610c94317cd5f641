"""The msmz_log of one call on every MSM path pinned against a recorded fixture (tests/golden/msm_log_counts.json):
the planner's choices (c, K, GLV), the device totals (entries, pairs, longest bucket, tree rounds), the scatter
launches, and which stage timers a timed call sets.  Fixed-seed inputs, so every count is deterministic; the timers
themselves are not compared, only whether each is set.

Record the fixture with `python tests/test_log_gpu.py --record tests/golden/msm_log_counts.json` on a GPU."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "msm_log_counts.json")
COUNTS = ["c", "K", "glv", "rounds", "n_entries", "n_pairs", "max_bucket", "scatter_launches"]

# name: curve, engines, points, scalar vectors, options (glv, c, buckets, reserved0; host: the scalars from a host
# buffer), GLV bits assumed (0 = default), precomputed copies (0 = plain points)
CASES = {
    "bls12-377 affine 2^16": ("bls12-377", 1, 1 << 16, 1, dict(glv=0), 0, 0),
    "bls12-377 affine 2^12 glv": ("bls12-377", 1, 1 << 12, 1, dict(glv=1), 0, 0),
    "bls12-377 batch 16 x 2^12": ("bls12-377", 1, 1 << 12, 16, dict(glv=0), 0, 0),
    "bls12-377 batch 4 x 2^12 projective": ("bls12-377", 1, 1 << 12, 4, dict(glv=0, buckets=1), 0, 0),
    "bls12-377 batch 4 x 2^12 precomputed": ("bls12-377", 1, 1 << 12, 4, dict(glv=0), 0, 2),
    "bls12-377 reduceAffine 2^12": ("bls12-377", 1, 1 << 12, 1, dict(glv=0, reserved0=1), 0, 0),
    "pallas projective 2^14": ("pallas", 1, 1 << 14, 1, dict(glv=0, buckets=1), 0, 0),
    "ed-on-bls12-377 2^14": ("ed-on-bls12-377", 1, 1 << 14, 1, dict(glv=0), 0, 0),
    "bls12-377 glv retry 2^12": ("bls12-377", 1, 1 << 12, 1, dict(glv=1, c=7), 64, 0),
    "bls12-377 batch 4 x 2^12 glv retry": ("bls12-377", 1, 1 << 12, 4, dict(glv=1, c=7), 64, 0),
    "bls12-377 fallback sort c 22": ("bls12-377", 1, 3000, 1, dict(glv=0, c=22), 0, 0),
    "bls12-377 two engines 2^16 + 5000": ("bls12-377", 2, (1 << 16) + 5000, 1, dict(glv=0), 0, 0),
    "bls12-377 two engines batch 4 x 2^16 + 5000": ("bls12-377", 2, (1 << 16) + 5000, 4, dict(glv=0), 0, 0),
    "bls12-377 two engines host scalars 2^16 + 5000": ("bls12-377", 2, (1 << 16) + 5000, 1, dict(glv=0, host=1), 0, 0),
}


def run_case(name):
    """one timed call of the case -> its counts, the stage timers it set, the tree rounds it timed, a digest of the
    results"""
    import msm_zprize_amd as m
    from msm_zprize_amd._native import MsmzLog, MsmzOpts, check, lib
    label, engines, n, batch, o, glv_bits, copies = CASES[name]
    m.startThreads(devices=[0] * engines)
    params = m.curves.BY_LABEL[label]
    curve = (m.Weierstrass if params["kind"] == "weierstrass" else m.TwistedEdwards).create(params)
    m.startThreads()
    try:
        pts = curve.Parallel.randomPointsFast(n, 4242)
        sc = curve.Parallel.randomScalars(n * batch, 4343)
        ph = pts.handle
        if copies:
            pre = curve.Parallel.precomputePoints(pts, n, {"glv": o.get("glv", 0)}, copies)
            ph = pre.handle
        opts = MsmzOpts()
        opts.c = o.get("c", 0)
        opts.glv = o.get("glv", -1)
        opts.buckets = o.get("buckets", 0)
        opts.timing = 1
        opts.reserved[0] = o.get("reserved0", 0)
        if glv_bits:
            check(lib().msmz_test_set_glv_bits(curve._ctx, glv_bits), "msmz_test_set_glv_bits")
        retries = lib().msmz_test_retries(curve._ctx)
        fb = curve.fe_bytes
        out = C.create_string_buffer(2 * fb * batch)
        inf = (C.c_int * batch)()
        log = MsmzLog()
        if o.get("host"):   # the same scalars from a host buffer
            hs = C.create_string_buffer(32 * n * batch)
            check(lib().msmz_download_scalars(curve._ctx, sc.handle, 0, n * batch, hs), "msmz_download_scalars")
            if batch == 1:
                st = lib().msmz_msm(curve._ctx, ph, hs.raw, n, C.byref(opts), out, inf, C.byref(log))
            else:
                st = lib().msmz_msm_batch(curve._ctx, ph, hs.raw, n, batch, C.byref(opts), out, inf, C.byref(log))
        elif batch == 1:
            st = lib().msmz_msm_resident(curve._ctx, ph, sc.handle, n, C.byref(opts), out, inf, C.byref(log))
        else:
            st = lib().msmz_msm_batch_resident(curve._ctx, ph, sc.handle, n, batch, C.byref(opts), out, inf,
                                               C.byref(log))
        check(st, name)
        rec = {k: int(getattr(log, k)) for k in COUNTS}
        rec["retries"] = lib().msmz_test_retries(curve._ctx) - retries
        rec["stages_set"] = [i for i in range(len(log.stage_ms)) if log.stage_ms[i] > 0]
        rec["rounds_timed"] = [r for r in range(32) if log.batch_add_ms[r] > 0]
        rec["results_sha256"] = hashlib.sha256(out.raw + bytes(inf)).hexdigest()
        return rec
    finally:
        curve.close()


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_log_matches_fixture(name):
    """every count and the result equal the recorded ones; a timed call sets at least the timers it set then"""
    want = _fixture()[name]
    got = run_case(name)
    for k in COUNTS + ["retries", "rounds_timed", "results_sha256"]:
        assert got[k] == want[k], (name, k, got[k], want[k])
    missing = set(want["stages_set"]) - set(got["stages_set"])
    assert not missing, (name, "stage timers no longer set", sorted(missing))


def test_fixture_covers_every_case():
    assert sorted(_fixture()) == sorted(CASES)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_log_gpu.py --record OUT.json")
    res = {name: run_case(name) for name in CASES}
    with open(sys.argv[2], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))
