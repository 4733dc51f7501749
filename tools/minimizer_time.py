#!/usr/bin/env python3
"""What a window costs the walkers (GPU box): python tools/minimizer_time.py [--parent-root DIR] [--out profiles/minimizer_time.json]

Shape: the bench's sketch leg, the one tools/filter_time.py uses -- 1000 genomes x 5 Mbp of random packed bases, k = 31, S = 1024;
D2G_TIME_K1 events, medians of 20 launches after 3 warm-up launches.

  (a) windowed K1   d2g_oph_sketch_dev over plans made with w = 40, 50, 100, 250, each as a ratio to plain K1 measured in the same run
  (b) K1b, K3       the count pass ("k1count") and the --multiset chain ("k3": hist, scan, scatter, refine, count, sketch) at w = 50
                    against their unwindowed selves, same run
  (c) unwindowed    plain K1 of this tree against the parent commit: DIR is a checkout of the parent commit with its library built.
                    One fresh process per measurement, the two taking turns; the run-to-run range of a side is the range of its medians"""
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


def launches(ctx, torch, call, event, reps, warm):
    ts = []
    for i in range(warm + reps):
        call()
        torch.cuda.synchronize()
        t = ctx.kernel_ms(event)[2]
        if i >= warm:
            ts.append(t)
    return ts


def setup(root, ng):
    sys.path.insert(0, root)
    import torch
    import dashing2_amd as D
    ctx = D.Context(0)
    ctx.set_timing(True)
    rs, rl, go, stride = runs(ng, L)
    torch.manual_seed(1)
    packed = torch.randint(0, 256, (ng * stride + 64,), dtype=torch.uint8, device="cuda")
    regs = torch.empty((ng, D.oph_m(S)), dtype=torch.int64, device="cuda")
    return D, torch, ctx, (rs, rl, go), packed, regs


def child(root, reps, warm):
    """one measurement of unwindowed K1 from the tree at `root`, in this (fresh) process: one JSON line"""
    D, torch, ctx, (rs, rl, go), packed, regs = setup(root, NG)
    plan = ctx.oph_plan(rs, rl, go, K)
    ts = launches(ctx, torch, lambda: ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr()), "k1", reps, warm)
    print(json.dumps({"k1_ms": med(ts), "min_max": [min(ts), max(ts)], "checksum": int(regs.sum().item()) & 0xFFFFFFFF}), flush=True)


def entry(ts, base=None):
    e = {"ms": med(ts), "min_max": [min(ts), max(ts)]}
    if base is not None:
        e["over_unwindowed"] = med(ts) / med(base)
    return e


def windowed(reps, warm, windows, w_other, k3_reps):
    D, torch, ctx, (rs, rl, go), packed, regs = setup(ROOT, NG)
    plain = ctx.oph_plan(rs, rl, go, K)
    out = {"k1": {}, "k1b": {}, "multiset": {}}
    base = launches(ctx, torch, lambda: ctx.oph_sketch_dev(plain, packed.data_ptr(), S, regs.data_ptr()), "k1", reps, warm)
    out["k1"]["unwindowed"] = entry(base)
    out["k1"]["unwindowed"]["kmers"] = plain.nkmers
    print("k1 unwindowed", out["k1"]["unwindowed"], flush=True)
    keep = regs.clone()
    for w in windows:
        plan = ctx.oph_plan(rs, rl, go, K, w=w)
        ts = launches(ctx, torch, lambda: ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr()), "k1", reps, warm)
        e = entry(ts, base)
        e.update(q=w - K + 1, emissions=plan.nkmers, registers_changed=int((regs != keep).sum().item()))
        out["k1"][f"w{w}"] = e
        print(f"k1 w{w}", e, flush=True)
        plan.close()
    # K1b over final registers, unwindowed and at w_other
    counts = torch.empty((NG, D.oph_m(S)), dtype=torch.int32, device="cuda")
    wplan = ctx.oph_plan(rs, rl, go, K, w=w_other)
    for name, plan in (("unwindowed", plain), (f"w{w_other}", wplan)):
        ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr())
        ts = launches(ctx, torch, lambda: ctx.oph_count_dev(plan, packed.data_ptr(), S, regs.data_ptr(), counts.data_ptr()), "k1count", reps, warm)
        out["k1b"][name] = entry(ts, None if plan is plain else b1)
        if plan is plain:
            b1 = ts
        print("k1b", name, out["k1b"][name], flush=True)
    # the --multiset chain
    sig = torch.empty((NG, S), dtype=torch.float64, device="cuda")
    tw = torch.empty(NG, dtype=torch.float64, device="cuda")
    for name, plan in (("unwindowed", plain), (f"w{w_other}", wplan)):
        ts = launches(ctx, torch, lambda: ctx.bmh_sketch_dev(plan, packed.data_ptr(), S, sig.data_ptr(), tw.data_ptr()), "k3", k3_reps, 1)
        out["multiset"][name] = entry(ts, None if plan is plain else b3)
        out["multiset"][name]["total_weight"] = float(tw.sum().item())
        if plan is plain:
            b3 = ts
        print("multiset", name, out["multiset"][name], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minimizer_time.json"))
    ap.add_argument("--parent-root", help="checkout of the parent commit, library built")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k3-reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--windows", default="40,50,100,250")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warm)
    res = {"shape": {"genomes": NG, "len": L, "k": K, "S": S},
           "timer": f"D2G_TIME_K1 events, medians of {a.reps} launches after {a.warm} warm-up launches ({a.k3_reps} after 1 for the multiset chain); "
                    "one fresh process per measurement against the parent"}
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
        res["unwindowed_vs_parent"] = {"parent": got["parent"], "this": got["this"], "parent_range_of_medians": [min(pm), max(pm)],
                                       "this_range_of_medians": [min(tm), max(tm)], "this_median_of_medians": med(tm),
                                       "this_inside_or_below_parent_range": med(tm) <= max(pm)}
    res["windowed"] = windowed(a.reps, a.warm, [int(x) for x in a.windows.split(",")], 50, a.k3_reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
