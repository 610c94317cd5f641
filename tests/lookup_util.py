"""Shared by the lookup tests (tests/test_lookup_cpu.py, tests/test_lookup_gpu.py, tests/test_js_lookup.py,
tests/golden/make_lookup_fixture.py): msmz_scalars_lookup in Python integers -- collections.Counter plus "the first index
of each value" -- and the tables and columns that decide where the probes of csrc/lookup_kernels.h collide and where the
wave aggregation of k_lookup_count meets runs of equal values.  W is a workgroup, from msmz_test_lookup_geometry (or the
CPU driver's `geometry`), never a copy of the constant."""
import collections
import random

NONE = 0xffffffff


def model(table, column):
    """-> (multiplicities, positions, info) of the issue: m[j] = the count of table[j] in the column if j is the first
    index that holds that value, else 0; positions[i] = that first index or NONE"""
    first = {}
    for j, t in enumerate(table):
        first.setdefault(t, j)
    counts = collections.Counter(column)
    m = [counts[t] if first[t] == j else 0 for j, t in enumerate(table)]
    positions = [first.get(f, NONE) for f in column]
    missing = [i for i, p in enumerate(positions) if p == NONE]
    info = {"missing": len(missing), "firstMissing": missing[0] if missing else None, "distinct": len(first)}
    return m, positions, info


def slots(n):
    """the power of two S with 2 n <= S < 4 n"""
    s = 2
    while s < 2 * n:
        s *= 2
    return s


def distinct(n, q, rng, avoid=()):
    """n distinct random values below q, none of them in `avoid`"""
    seen, out = set(avoid), []
    while len(out) < n:
        v = rng.randrange(q)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def colliding(n, q, rng, slot_of, target):
    """n distinct values below q whose probe all starts at slot `target` of a table of n entries; slot_of(value) is the
    hash under test (msmz_test_lookup_slot or the driver's `slot`)"""
    out, seen = [], set()
    while len(out) < n:
        v = rng.randrange(q)
        if v not in seen and slot_of(v) == target:
            seen.add(v)
            out.append(v)
    return out


def tables(n, q, rng, slot_of=None):
    """{name: table of n entries}: the table kinds of the issue that exist at this size"""
    out = {"distinct": distinct(n, q, rng), "range": list(range(n)), "all_equal": [rng.randrange(q)] * n}
    if n >= 3:
        vals = distinct((n + 2) // 3, q, rng)
        t = (vals * 3)[:n]
        rng.shuffle(t)
        out["thrice"] = t                                   # each value three times at scattered indices
        edge = distinct(n, q, rng, avoid=(0, 1, q - 1))
        edge[0], edge[n // 2], edge[n - 1] = q - 1, 0, 1
        out["edges"] = edge                                  # 0, 1, q - 1 as ordinary keys
    if n >= 2:
        vals = distinct((n + 1) // 2, q, rng)
        out["twice"] = (vals + vals)[:n]                     # every value twice: the second half repeats the first
    if slot_of is not None:
        s = slots(n)
        out["one_slot"] = colliding(n, q, rng, slot_of, s // 3)
        out["last_slot"] = colliding(n, q, rng, slot_of, s - 1)   # every probe but the first wraps around
    return out


def columns(n, table, q, rng, W=256):
    """{name: column of n entries} over one table: the column kinds of the issue"""
    present = set(table)

    def absent():
        while True:
            v = rng.randrange(q)
            if v not in present:
                return v

    uniform = [rng.choice(table) for _ in range(n)]
    out = {"uniform": uniform, "constant": [table[len(table) // 2]] * n}
    popular = table[0]
    out["mostly_one"] = [popular if i % 64 != 37 else rng.choice(table) for i in range(n)]   # 63 of every 64 lanes
    runs, i = [], 0                                     # runs of equal values whose lengths straddle 64 and W
    lengths = [63, 2, 64, 1, W - 1, 3, W + 1, 65, 2 * W + 5]
    while len(runs) < n:
        runs += [table[(7 * i) % len(table)]] * lengths[i % len(lengths)]
        i += 1
    out["runs"] = runs[:n]
    out["all_missing"] = [absent() for _ in range(n)]
    for name, at in (("missing_first", 0), ("missing_last", n - 1), ("missing_wave_edge", min(n - 1, 64)),
                     ("missing_wave_end", min(n - 1, 63))):
        col = list(uniform)
        col[at] = absent()
        out[name] = col
    if n >= 3:
        col = list(uniform)
        col[n // 2], col[n - 1] = absent(), absent()   # two missing: the lowest is reported
        out["missing_two"] = col
    return out
