#!/usr/bin/env python3
"""LDS bank conflicts of k_ntt_pass (msm_zprize_amd/csrc/ntt_kernels.h), derived, not measured.

    python tools/ntt_lds_model.py [--pad WORDS] [--every LOG2_ENTRIES] [--search]

The tile lies in eight word planes and every access is 32 bits wide, so one wave instruction is served in two groups of
32 lanes over 32 banks, bank = slot mod 32 (MI355X: ds_read_b32 / ds_write_b32).  The model replays the slot of every
lane for every instruction of a pass -- the load, each radix-4 or radix-2 step, the bit-reversed read of the store --
with the index maps of the kernel, for the pass shapes the planner makes (stages, columns, first pass or later), and
(tests/test_ntt_cpu.py holds these maps against the slots the kernel's own thread bodies touch, and runs the model
over every shape of every plan) and prints the most distinct slots any group puts on one bank: 1 is conflict-free, 2 costs a store nothing.  slot = pos +
(pos >> every) * pad; the kernel uses pad 5 every 2^5 entries.  --search ranks the paddings."""
import argparse

THREADS = 256
SHAPES = [(10, 0, 0), (9, 0, 0), (8, 2, 0), (8, 2, 8), (7, 3, 7), (6, 4, 0), (6, 4, 6), (5, 5, 6), (4, 0, 0), (3, 0, 0)]   # (s, log_c, log_t)


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def instructions(s, log_c, log_t):
    """(name, the tile position each of the 256 threads touches, or None) for every LDS instruction of one pass"""
    entries, cmask = 1 << (s + log_c), (1 << log_c) - 1
    for first in range(0, entries, THREADS):
        yield "load", [o if o < entries else None for o in range(first, first + THREADS)]
    rem = s
    while rem >= 2:
        b = rem - 2
        for m in range(4):
            pos = []
            for bu in range(THREADS):
                q = bu >> log_c
                a0 = ((q >> b) << (b + 2)) | (q & ((1 << b) - 1))
                pos.append((((a0 + (m << b)) << log_c) + (bu & cmask)) if bu < entries // 4 else None)
            yield "radix-4 b=%d" % b, pos
        rem -= 2
    if rem:
        for first in range(0, entries // 2, THREADS):
            for m in range(2):
                yield "radix-2", [((((bu >> log_c) << 1) + m) << log_c) + (bu & cmask) if bu < entries // 2 else None
                                  for bu in range(first, first + THREADS)]
    for first in range(0, entries, THREADS):
        pos = []
        for o in range(first, first + THREADS):
            k, c = (o & ((1 << s) - 1), o >> s) if log_t == 0 else (o >> log_c, o & cmask)
            pos.append((bitrev(k, s) << log_c) + c if o < entries else None)
        yield "store", pos


def worst(slot, shapes=SHAPES):
    """{(shape, instruction): the most distinct slots one group of 32 lanes puts on one bank}"""
    res = {}
    for shape in shapes:
        for name, pos in instructions(*shape):
            for g in range(0, THREADS, 32):
                banks = {}
                for sl in {slot(p) for p in pos[g:g + 32] if p is not None}:
                    banks[sl % 32] = banks.get(sl % 32, 0) + 1
                if banks:
                    res[shape, name] = max(res.get((shape, name), 0), max(banks.values()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pad", type=int, default=5)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--search", action="store_true")
    args = ap.parse_args()
    if args.search:
        rows = []
        for every in (5, 6):
            for pad in range(33):
                r = worst(lambda p: p + (p >> every) * pad)
                rows.append((max(r.values()), sum(r.values()), 1024 + (1024 >> every) * pad, every, pad))
        for mx, total, words, every, pad in sorted(rows)[:10]:
            print(f"pad {pad} every 2^{every}: worst {mx}-way, sum of worsts {total}, {words} words per plane")
        return
    r = worst(lambda p: p + (p >> args.every) * args.pad)
    for (shape, name), ways in sorted(r.items()):
        print(f"s={shape[0]} log_c={shape[1]} log_t={shape[2]} {name}: {ways}-way")
    print(f"worst: {max(r.values())}-way; unpadded: {max(worst(lambda p: p).values())}-way")


if __name__ == "__main__":
    main()
