#!/usr/bin/env python3
"""Freezes small exact sets and their answers under tests/golden/exact/sets.npz, all from tests/exact_ref.py (nothing of the product):
keys, counts, set_off of seven sets, and the intersection matrices of --set and --countdict by the literal merge of wcompare.cpp."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import exact_ref as X  # noqa: E402


def main():
    rng = np.random.default_rng(5100)
    pool = X.rng_keys(5101, 400)
    sets = []
    for m in (0, 1, 37, 120, 120, 64, 250):
        k = np.sort(rng.choice(pool, m, replace=False))
        c = rng.integers(1, 6, m).astype(np.uint32)
        if m == 64:
            c[:] = 2 ** 32 - 1
        sets.append((k, c))
    sets[4] = (sets[3][0].copy(), rng.integers(1, 6, 120).astype(np.uint32))      # the same keys as set 3, other counts
    keys, counts, off, cards = X.flat(sets)
    n = len(sets)
    isz_set, isz_cd = np.zeros((n, n), np.uint64), np.zeros((n, n), np.uint64)
    for i in range(n):
        for j in range(n):
            isz_set[i, j] = X.merge_isz(sets[i][0], None, sets[j][0], None)
            isz_cd[i, j] = X.merge_isz(sets[i][0], sets[i][1], sets[j][0], sets[j][1])
    np.savez_compressed(os.path.join(HERE, "exact", "sets.npz"), keys=keys, counts=counts, set_off=off, cards=cards, isz_set=isz_set, isz_countdict=isz_cd)


if __name__ == "__main__":
    main()
