#!/usr/bin/env python3
"""What --filterset costs K1 (GPU box): python tools/filter_time.py --parent-root DIR [--out profiles/filter_time.json]

Shape: the bench's sketch leg, the one tools/oph_counts_time.py uses -- 1000 genomes x 5 Mbp of random packed bases, k = 31, S = 1024;
D2G_TIME_K1 events around d2g_oph_sketch_dev, medians of 20 launches after 3 warm-up launches.

  (a) unfiltered   K1 with no filter attached, this tree against the parent commit: DIR is a checkout of the parent commit with its
                   library built (git worktree add DIR HEAD~1 && make -C DIR/dashing2_amd/csrc).  One fresh process per measurement,
                   parent and this tree taking turns, `--rounds` rounds; the run-to-run range of each side is the range of its medians
  (b) filtered     K1 with a filter of 5 kbp, 5 Mbp and 100 Mbp of random sequence attached, with the build time ("filter" events:
                   the table's memset and the insert kernel) and the table's size"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG, L, K, S = 1000, 5_000_000, 31, 1024


def med(x):
    return float(np.median(np.asarray(x, np.float64)))


def runs(ng, length):
    stride = ((length + 3) // 4 + 63) // 64 * 64
    return (np.arange(ng, dtype=np.uint64) * np.uint64(stride * 4), np.full(ng, length, np.uint32), np.arange(ng + 1, dtype=np.uint64), stride)


def k1_launches(ctx, torch, plan, packed, regs, reps, warm):
    ts = []
    for i in range(warm + reps):
        ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr())
        torch.cuda.synchronize()
        t = ctx.kernel_ms("k1")[2]
        if i >= warm:
            ts.append(t)
    return ts


def setup(root):
    sys.path.insert(0, root)
    import torch
    import dashing2_amd as D
    ctx = D.Context(0)
    ctx.set_timing(True)
    rs, rl, go, stride = runs(NG, L)
    torch.manual_seed(1)
    packed = torch.randint(0, 256, (NG * stride + 64,), dtype=torch.uint8, device="cuda")
    plan = ctx.oph_plan(rs, rl, go, K)
    regs = torch.empty((NG, D.oph_m(S)), dtype=torch.int64, device="cuda")
    return D, torch, ctx, plan, packed, regs


def child(root, reps, warm):
    """one measurement of unfiltered K1 from the tree at `root`, in this (fresh) process: one JSON line"""
    D, torch, ctx, plan, packed, regs = setup(root)
    ts = k1_launches(ctx, torch, plan, packed, regs, reps, warm)
    print(json.dumps({"k1_ms": med(ts), "min_max": [min(ts), max(ts)], "checksum": int(regs.sum().item()) & 0xFFFFFFFF}), flush=True)


def filtered(reps, warm, sizes):
    D, torch, ctx, plan, packed, regs = setup(ROOT)
    base = k1_launches(ctx, torch, plan, packed, regs, reps, warm)
    plain = regs.clone()
    out = {"unfiltered_k1_ms": med(base), "unfiltered_min_max": [min(base), max(base)], "filters": []}
    for fl in sizes:
        e = {"filter_bases": fl}
        try:
            rs, rl, go, stride = runs(1, fl)
            torch.manual_seed(2)
            fpacked = torch.randint(0, 256, (stride + 64,), dtype=torch.uint8, device="cuda")
            fplan = ctx.oph_plan(rs, rl, go, K)
            ctx.kernel_ms("filter")
            f = ctx.kmer_filter_dev(fplan, fpacked.data_ptr(), canon=True)
            nocc, ndist, nbytes = f.info()
            e.update(kmers=nocc, distinct=ndist, table_bytes=nbytes, build_ms=ctx.kernel_ms("filter")[2])
            plan.set_filter(f)
            ts = k1_launches(ctx, torch, plan, packed, regs, reps, warm)
            plan.set_filter(None)
            e.update(k1_ms=med(ts), min_max=[min(ts), max(ts)], over_unfiltered=med(ts) / med(base),
                     registers_changed=int((regs != plain).sum().item()))
            f.close()
            fplan.close()
            del fpacked
            torch.cuda.empty_cache()
        except D.D2GError as err:                                      # a size that could not be run is reported, not hidden
            e["error"] = str(err)
        out["filters"].append(e)
        print(json.dumps(e), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_time.json"))
    ap.add_argument("--parent-root", help="checkout of the parent commit, library built")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--sizes", default="5000,5000000,100000000")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warm)
    res = {"shape": {"genomes": NG, "len": L, "k": K, "S": S},
           "timer": f"D2G_TIME_K1 events, medians of {a.reps} launches after {a.warm} warm-up launches; one fresh process per unfiltered measurement"}
    if a.parent_root:
        sides = {"parent": os.path.abspath(a.parent_root), "this": ROOT}
        got = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, root in sides.items():                              # the two take turns
                env = dict(os.environ, D2G_LIB=os.path.join(root, "dashing2_amd", "libd2g.so"))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--reps", str(a.reps), "--warm", str(a.warm)],
                                   capture_output=True, text=True, env=env, timeout=300)
                if r.returncode:
                    raise SystemExit(f"{s}: {r.stderr[-2000:]}")
                got[s].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(s, got[s][-1], flush=True)
        pm, tm = [x["k1_ms"] for x in got["parent"]], [x["k1_ms"] for x in got["this"]]
        res["unfiltered_vs_parent"] = {"parent": got["parent"], "this": got["this"], "parent_range_of_medians": [min(pm), max(pm)],
                                       "this_range_of_medians": [min(tm), max(tm)], "this_median_of_medians": med(tm),
                                       "this_inside_or_below_parent_range": med(tm) <= max(pm)}
    res["filtered"] = filtered(a.reps, a.warm, [int(x) for x in a.sizes.split(",")])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
