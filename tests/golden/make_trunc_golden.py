#!/usr/bin/env python3
"""Freezes tests/golden/trunc_kat.npz from the NumPy restatement of the reference's truncated-register path (tests/trunc_ref.py):
codes, a and b of make_compressed() for three small matrices, and values of both compressed epilogues of compare().

    python tests/golden/make_trunc_golden.py          (run in the build container; the .npz is committed)

The product (dashing2_amd/csrc/d2g_epilogue.cpp) must reproduce every value bit for bit (tests/test_trunc_host.py).  long double
logl/expl/powl come from the machine's libm: the file pins what the build container's libm gives."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import trunc_cases as TC  # noqa: E402
import trunc_ref as R  # noqa: E402


def ld_bytes(x):
    """the 10 significant bytes of an x87 long double"""
    return np.frombuffer(np.array([x], np.longdouble).tobytes()[:10], np.uint8).copy()


def epilogue_rows(rng):
    rows_g, rows_n = [], []
    cards = [(1e6, 2.5e6), (123456.789, 99.5), (1.0, 1.0), (0.0, 5.0), (7.25, 0.0), (3e9, 3e9)]
    bases = [np.longdouble("1.0411682651016159572"), np.longdouble("1.0001565619892149694"), np.longdouble("1.0000000023886864839"),
             np.longdouble(1.5)]
    for S in (3, 100, 1000, 1024):
        pairs = {(0, 0), (S, 0), (0, S), (S // 2, S - S // 2), (1, 0), (0, 1), (S - 1, 0), (S - 1, 1), (S // 3, S // 3), (S // 3, S - S // 3 - 1)}
        for _ in range(5):
            g = int(rng.integers(0, S + 1))
            pairs.add((g, int(rng.integers(0, S - g + 1))))
        for bi, b in enumerate(bases):
            for gt, lt in sorted(pairs):
                for lhc, rhc in cards:
                    for meas in range(6):
                        for k in ((31,) if meas != R.POISSON_LLR else (31, 1, 0)):
                            v = R.epilogue_gtlt([gt], [lt], S, b, [lhc], [rhc], meas, k)[0]
                            rows_g.append((gt, lt, S, bi, meas, k, lhc, rhc, v))
        for neq in sorted({0, 1, S // 2, S - 1, S} | {int(x) for x in rng.integers(0, S + 1, 4)}):
            for regbytes in (1, 2, 4):
                for lhc, rhc in cards:
                    for meas in range(6):
                        for k in ((31,) if meas != R.POISSON_LLR else (31, 1, 0)):
                            v = R.epilogue_bbit([neq], S, regbytes, [lhc], [rhc], meas, k)[0]
                            rows_n.append((neq, S, regbytes, meas, k, lhc, rhc, v))
    return bases, rows_g, rows_n


def main():
    rng = np.random.default_rng(20261017)
    mats = {"oph": TC.oph_shaped(rng, 24, 50, families=3, unrelated=3, empty_rows=1)[0], "wide": TC.wide_range(rng, 16, 33),
            "seam": TC.exp_over_1024(rng, 16, 40)}
    out = {}
    for name, m in mats.items():
        out[f"sig_{name}"] = m
        for rb in (1, 2, 4):
            for bb in (0, 1):
                codes, a, b, _, _ = R.truncate(m, rb, bb)
                out[f"codes_{name}_{rb}_{bb}"] = codes
                if not bb:
                    out[f"a_{name}_{rb}"], out[f"b_{name}_{rb}"] = ld_bytes(a), ld_bytes(b)
    bases, rows_g, rows_n = epilogue_rows(rng)
    out["bases"] = np.stack([ld_bytes(b) for b in bases])
    out["gtlt_in"] = np.array([r[:6] for r in rows_g], np.int64)
    out["gtlt_cards"] = np.array([r[6:8] for r in rows_g], np.float64)
    out["gtlt_out"] = np.array([r[8] for r in rows_g], np.float32).view(np.uint32)
    out["neq_in"] = np.array([r[:5] for r in rows_n], np.int64)
    out["neq_cards"] = np.array([r[5:7] for r in rows_n], np.float64)
    out["neq_out"] = np.array([r[7] for r in rows_n], np.float32).view(np.uint32)
    path = os.path.join(HERE, "trunc_kat.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(mats)} matrices, {len(rows_g)} (gt, lt) rows, {len(rows_n)} neq rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
