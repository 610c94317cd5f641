"""The N > 1 path on CPU: two gloo ranks, each with its input shard; the exchange step
(all_gather of the partial sums + host-side msmz_point_add) must reproduce the whole MSM.
The per-shard MSM itself is computed by the oracle here (no GPU in this test); on the GPU box the
same combine code runs after the HIP MSM (bench.py --gpus N)."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, json, random
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from oracle import c_oracle, params as P, bigint_ref as B
from msm_zprize_amd import sharding
from msm_zprize_amd import curves
label = sys.argv[1]
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
oc, pc = P.CURVES[label], curves.BY_LABEL[label]
rng = random.Random(99)
n = 37
if oc["kind"] == "weierstrass":
    A = B.AffineWeierstrass(oc)
    pts = []
    for _ in range(n):
        x, y, z = A.scale(rng.randrange(1, 1 << 64), A.one)
        pts.append({"x": x, "y": y, "isZero": z})
else:
    T = B.TwistedEdwards(oc)
    pts = []
    for _ in range(n):
        x, y = T.to_affine(T.scale(rng.randrange(1, 1 << 64), T.one))
        pts.append({"x": x, "y": y})
scalars = [rng.randrange(oc["order"]) for _ in range(n)]
lo, hi = sharding.shard_range(n, rank, world)
partial = c_oracle.msm(oc, scalars[lo:hi], pts[lo:hi])
total = sharding.combine_partials(pc, partial)
whole = c_oracle.msm(oc, scalars, pts)
ok = (total["x"], total["y"]) == (whole["x"], whole["y"]) and bool(total.get("isZero")) == bool(whole.get("isZero"))
print(json.dumps({"rank": rank, "ok": ok, "range": [lo, hi]}), flush=True)
dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


@pytest.mark.parametrize("label", ["bls12-377", "pallas", "ed-on-bls12-377"])
def test_two_rank_gloo_combine(tmp_path, label):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    port = 29500 + random.Random(label).randrange(2000)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), str(script), label],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count('"ok": true') == 2, out.stdout


def test_shard_range_partition():
    from msm_zprize_amd.sharding import shard_range
    for n in (1, 7, 8, 1 << 20, (1 << 26) + 3):
        for world in (1, 2, 3, 8):
            edges = [shard_range(n, r, world) for r in range(world)]
            assert edges[0][0] == 0 and edges[-1][1] == n
            assert all(edges[i][1] == edges[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in edges]
            assert max(sizes) - min(sizes) <= 1


@pytest.mark.parametrize("label", ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"])
def test_point_add_host_only(label):
    """msmz_point_add is pure host code: works without a GPU, matches the oracle's group law on every curve.  It is the
    fold of the engine's partial sums (index-range passes, devices), so the cases are the fold's: P + Q, the doubling
    P + P, P + (-P), and the identity on either side and on both.  Twisted Edwards has no infinity flag: its identity is
    the point (0, 1), and a null operand is refused."""
    import ctypes as C
    from msm_zprize_amd import curves, sharding
    from msm_zprize_amd._native import lib
    from oracle import bigint_ref as B, params as P
    c, pc = P.CURVES[label], curves.BY_LABEL[label]
    rng = random.Random(label)
    k1, k2 = rng.randrange(1, c["order"]), rng.randrange(1, c["order"])
    if c["kind"] == "weierstrass":
        A = B.AffineWeierstrass(c)
        d = lambda t: {"x": t[0], "y": t[1], "isZero": t[2]}
        p1, p2, zero = A.scale(k1, A.one), A.scale(k2, A.one), A.zero
        add, neg = A.add, A.negate
    else:
        T = B.TwistedEdwards(c)
        d = lambda t: dict(zip("xy", T.to_affine(t)), isZero=False)
        p1, p2, zero = T.scale(k1, T.one), T.scale(k2, T.one), T.zero
        add, neg = T.add, T.negate
        assert d(zero) == sharding.identity(pc) == {"x": 0, "y": 1, "isZero": False}
    cases = [(p1, p2), (p2, p1), (p1, p1), (p1, neg(p1)), (neg(p2), p2), (zero, p1), (p1, zero), (zero, zero)]
    for a, b in cases:
        assert sharding.point_add(pc, d(a), d(b)) == d(add(a, b)), (label, cases.index((a, b)))
    assert sharding.point_add(pc, d(p1), d(neg(p1))) == sharding.identity(pc)
    assert sharding.point_add(pc, sharding.identity(pc), d(p2)) == d(p2)
    # null operands: Weierstrass takes one with its infinity flag and refuses one without; twisted Edwards refuses both
    fb = pc["fe_bytes"]
    xy = int(d(p1)["x"]).to_bytes(fb, "little") + int(d(p1)["y"]).to_bytes(fb, "little")
    out, inf = C.create_string_buffer(2 * fb), C.c_int()
    assert lib().msmz_point_add(pc["curve_id"], None, 0, xy, 0, out, C.byref(inf)) == 1   # MSMZ_ERR_ARG
    assert lib().msmz_point_add(pc["curve_id"], xy, 0, None, 0, out, C.byref(inf)) == 1
    want = 1 if c["kind"] == "twisted-edwards" else 0
    assert lib().msmz_point_add(pc["curve_id"], None, 1, xy, 0, out, C.byref(inf)) == want
    assert lib().msmz_point_add(pc["curve_id"], xy, 0, None, 1, out, C.byref(inf)) == want
    if not want:
        assert out.raw == xy and inf.value == 0
