"""Shared by the scalar-set arithmetic tests (tests/test_scalar_ops_cpu.py, tests/test_scalar_ops_gpu.py,
tests/test_js_scalar_ops.py, tests/golden/make_scalar_ops_fixture.py): the operands that exercise the carry chains of
csrc/fr.h, the rows planted into every set, and the byte encodings of the C ABI.  Expected values are Python integers
mod oracle.params.CURVES[label]["order"]."""
import random

from oracle import params as P

ALL = ["bls12-377", "pallas", "bls12-381", "ed-on-bls12-377"]


def order(label):
    return P.CURVES[label]["order"]


def low_words_full(q):
    """the largest value below q whose low 7 words are all 0xffffffff"""
    v = ((q >> 224) << 224) | ((1 << 224) - 1)
    return v if v < q else v - (1 << 224)


def edge_values(q):
    """the operands of the issue: small values, q - 1, q - 2, the halves, the word and limb boundaries, and the value
    whose low seven words carry all the way up"""
    return [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 128, 1 << 224,
            low_words_full(q)]


def operands(label, seed=0):
    """edge values and 64 random ones"""
    q = order(label)
    rng = random.Random(1000 * ALL.index(label) + seed)
    return edge_values(q) + [rng.randrange(q) for _ in range(64)]


def planted_pairs(q, rng):
    """(x, y) rows for out = a x + b y with a = b = 1 and for dot products: 0, 1, q - 1, the carry-chain values, and
    pairs whose sum is exactly q (-> 0), q - 1 and 0"""
    r = rng.randrange(1, q)
    rows = [(0, 0), (1, q - 1), (q - 1, q - 1), (q - 1, 1), (0, q - 1), (r, q - r), (r, q - 1 - r), ((q - 1) // 2, (q + 1) // 2),
            (low_words_full(q), 1), (low_words_full(q), low_words_full(q))]
    edges = edge_values(q)
    rows += [(e, edges[(k + 3) % len(edges)]) for k, e in enumerate(edges)]
    return rows


def random_below_2_250(n, rng):
    """n values below 2^250 (< q on all four curves), quickly: one draw of random bytes, the top byte of each record
    masked.  The values that matter for the carry chains are planted, not drawn."""
    raw = bytearray(rng.getrandbits(256 * n).to_bytes(32 * n, "little"))
    raw[31::32] = bytes(v & 3 for v in raw[31::32])
    return decode(bytes(raw))


def build_vectors(label, n, seed):
    """two vectors of n scalars: the planted pairs in the first 64 entries AND ending at the last index (the partial
    wave), random values elsewhere"""
    q = order(label)
    rng = random.Random(seed)
    xs = random_below_2_250(n, rng)
    ys = random_below_2_250(n, rng)
    rows = planted_pairs(q, rng)
    assert len(rows) <= 64
    for k, (x, y) in enumerate(rows):
        if k < n:
            xs[k], ys[k] = x, y
    for k in range(len(rows)):   # (rotated by n, so that the one-entry last waves of different sizes get different rows)
        if n - 1 - k >= min(len(rows), n):
            xs[n - 1 - k], ys[n - 1 - k] = rows[(k + n) % len(rows)]
    return xs, ys


def encode(scalars):
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def decode(raw):
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]
