#!/usr/bin/env python3
"""Times the (gt, lt) launch on truncated codes against the route without them -- the same codes widened to 64 bits in a
D2G_CMP_DIRECT set -- on one GPU: N = 10 000, S = 1024, upper triangle, D2G_TIME_K2 events, median of 20 launches after 3 warm-up
launches; also the k2prep time of each set and its operand bytes.  Writes profiles/fastcmp_time.json.

    python tools/trunc_time.py [--n 10000] [--s 1024] [--out profiles/fastcmp_time.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dashing2_amd as D  # noqa: E402


def time_set(ctx, make, N, launches, warm):
    make().close()                                   # code objects loaded, allocator warm: the prepare below is a steady one
    ctx.sync()
    ctx.set_timing(D.TIME_K2 | D.TIME_K2PREP)
    ctx.kernel_ms("k2prep")
    cs = make()
    ctx.sync()
    prep = ctx.kernel_ms("k2prep")
    n = D.ut_count(N)
    dg, dl = ctx.malloc(n * 4), ctx.malloc(n * 4)
    ms = []
    try:
        for it in range(warm + launches):
            cs.gtlt_ut_dev(dg, dl)
            ctx.sync()
            last = ctx.kernel_ms("k2")
            if it >= warm:
                ms.append(last[2])
        g, l = np.empty(n, np.uint32), np.empty(n, np.uint32)
        ctx.d2h(g, dg)
        ctx.d2h(l, dl)
    finally:
        ctx.free(dg)
        ctx.free(dl)
    rec = {"k2_ms_median": statistics.median(ms), "k2_ms_min": min(ms), "k2_ms_max": max(ms), "launches": launches, "warmup": warm,
           "k2prep_ms": prep[2], "operand_bytes": cs.operand_bytes}
    cs.close()
    ctx.set_timing(False)
    return rec, g, l


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--s", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastcmp_time.json"))
    a = ap.parse_args()
    N, S = a.n, a.s
    rng = np.random.default_rng(1)
    ctx = D.Context(0)
    res = {"N": N, "S": S, "shape": "upper triangle", "pairs": D.ut_count(N), "timer": "D2G_TIME_K2 events, median", "rows": []}
    for regbytes in (1, 2, 4):
        P = 8 * regbytes
        codes = rng.integers(0, 1 << P, (N, S), dtype=np.uint64).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[regbytes])
        base, g0, l0 = time_set(ctx, lambda: ctx.cmp_set(codes.astype(np.uint64), algo=D.CMP_DIRECT), N, a.launches, a.warmup)
        new, g1, l1 = time_set(ctx, lambda: ctx.cmp_set_codes(codes), N, a.launches, a.warmup)
        assert np.array_equal(g0, g1) and np.array_equal(l0, l1), "the two routes disagree"
        row = {"regbytes": regbytes, "direct_u64": base, "planes": new, "speedup": base["k2_ms_median"] / new["k2_ms_median"],
               "valu_ops_per_register_pair_bound": (2 * P + 2) / 32}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
