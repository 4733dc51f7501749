#!/usr/bin/env python3
"""What the count-sketch chain (K3k: --multiset -c <cells>) costs (GPU box):
    python tools/countsketch_time.py [--parent-root DIR] [--out profiles/countsketch_time.json]

Shape: config 5 -- 1000 genomes x 5 Mbp of random packed bases, k = 21, S = 2048; HIP events (D2G_TIME_K1 / D2G_TIME_K3), medians of 20
calls after warm-up calls (5 for tables of 2^24 cells and more: a call zeroes and reads back up to 512 GB of table), one fresh process.

  (a) the chain     d2g_bmh_sketch_cs_dev at cells = 2^10, L, 2L, 2^20, 2^24, 2^27, split into add ("k3k": zeroing + k3k_add_kernel),
                    compact ("k3kcompact") and BagMinHash ("k3kbmh"); the groups of genomes of each, and "table_bytes": the largest table
                    the context has allocated SO FAR (d2g_countsketch_stats; the switch sweep before it reached 4 * 40960 * 1000)
  (b) the switch    the add alone in BOTH forms at every table size that fits LDS: D2G_CS_LDS_CELLS=40960 (LDS) and =0 (global).
                    L (K3K_LDS_CELLS, d2g_k3_countsketch.hip) is set where the LDS form stops winning here
  (c) beside it     the exact --multiset chain ("k3") and plain K1 ("k1"), same run, with the bytes both chains keep on the device
  (d) the parent    "k3" and "k1" of this tree against the parent commit: DIR is a checkout of the parent commit with its library built.
                    One fresh process per measurement, the two taking turns"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG, LEN, K, S = 1000, 5_000_000, 21, 2048


def med(x):
    return float(np.median(np.asarray(x, np.float64)))


def runs(ng, length):
    stride = ((length + 3) // 4 + 63) // 64 * 64
    return (np.arange(ng, dtype=np.uint64) * np.uint64(stride * 4), np.full(ng, length, np.uint32), np.arange(ng + 1, dtype=np.uint64), stride)


def setup(root, ng):
    sys.path.insert(0, root)
    import torch
    import dashing2_amd as D
    ctx = D.Context(0)
    ctx.set_timing(True)
    rs, rl, go, stride = runs(ng, LEN)
    torch.manual_seed(1)
    packed = torch.randint(0, 256, (ng * stride + 64,), dtype=torch.uint8, device="cuda")
    return D, torch, ctx, (rs, rl, go), packed


def calls(ctx, torch, call, events, reps, warm):
    """-> {event: [total ms of the event's launches in one call, per timed call]}"""
    out = {e: [] for e in events}
    for i in range(warm + reps):
        for e in events:
            ctx.kernel_ms(e)                                             # reset
        call()
        torch.cuda.synchronize()
        for e in events:
            n, avg, _ = ctx.kernel_ms(e)
            if i >= warm:
                out[e].append(n * avg)
    return out


def entry(ts):
    return {"ms": med(ts), "min_max": [min(ts), max(ts)]}


def exact_and_k1(D, torch, ctx, tables, packed, reps, warm, k3_reps):
    rs, rl, go = tables
    plan = ctx.oph_plan(rs, rl, go, K)
    regs = torch.empty((NG, D.oph_m(S)), dtype=torch.int64, device="cuda")
    sig = torch.empty((NG, S), dtype=torch.float64, device="cuda")
    tw = torch.empty(NG, dtype=torch.float64, device="cuda")
    k1 = calls(ctx, torch, lambda: ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr()), ["k1"], reps, warm)["k1"]
    k3 = calls(ctx, torch, lambda: ctx.bmh_sketch_dev(plan, packed.data_ptr(), S, sig.data_ptr(), tw.data_ptr()), ["k3"], k3_reps, 1)["k3"]
    return plan, sig, tw, k1, k3


def child(root, reps, warm, k3_reps):
    """one measurement of the exact chain and of plain K1 from the tree at `root`, in this (fresh) process: one JSON line"""
    D, torch, ctx, tables, packed = setup(root, NG)
    _, sig, tw, k1, k3 = exact_and_k1(D, torch, ctx, tables, packed, reps, warm, k3_reps)
    print(json.dumps({"k1_ms": med(k1), "k3_ms": med(k3), "total_weight": float(tw.sum().item()),
                      "checksum": int(sig.view(torch.int64).sum().item()) & 0xFFFFFFFF}), flush=True)


def this_tree(reps, warm, k3_reps, big_reps):
    D, torch, ctx, tables, packed = setup(ROOT, NG)
    plan, sig, tw, k1, k3 = exact_and_k1(D, torch, ctx, tables, packed, reps, warm, k3_reps)
    nk = plan.nkmers
    out = {"kmers": nk, "k1": entry(k1), "exact_chain": entry(k3)}
    out["exact_chain"].update(total_weight=float(tw.sum().item()), key_bytes_on_device=16 * nk,
                              note="K3 keeps keys [sum of k-mers] u64 twice (coarse and refined): 16 bytes per k-mer")
    print("k1", out["k1"], "exact", out["exact_chain"], flush=True)
    L = D.countsketch_lds_cells()
    ev = ["k3k", "k3kcompact", "k3kbmh"]
    # (b) the LDS/global switch: the add alone, both forms, same table
    sw = {}
    for cells in (1024, 2048, 4096, 8192, 16384, 32768, 40960):
        e = {}
        for form, limit in (("lds", 40960), ("global", 0)):
            os.environ["D2G_CS_LDS_CELLS"] = str(limit)
            ctx.reload_tuning()
            ts = calls(ctx, torch, lambda: ctx.bmh_sketch_cs_dev(plan, packed.data_ptr(), S, cells, sig.data_ptr(), tw.data_ptr()), ev, 7, 1)
            e[form] = entry(ts["k3k"])
        e["lds_over_global"] = e["lds"]["ms"] / e["global"]["ms"]
        sw[str(cells)] = e
        print("switch", cells, e, flush=True)
    os.environ.pop("D2G_CS_LDS_CELLS")
    ctx.reload_tuning()
    out["lds_global_switch"] = {"L_compiled": L, "add_ms_by_cells": sw}
    # (a) the chain as shipped
    chain = {}
    for cells in (1 << 10, L, 2 * L, 1 << 20, 1 << 24, 1 << 27):
        r = big_reps if cells >= (1 << 24) else reps
        b0, g0, n0 = ctx.countsketch_stats()
        ts = calls(ctx, torch, lambda: ctx.bmh_sketch_cs_dev(plan, packed.data_ptr(), S, cells, sig.data_ptr(), tw.data_ptr()), ev, r, 1)
        b1, g1, n1 = ctx.countsketch_stats()
        tot = [a + b + c for a, b, c in zip(ts["k3k"], ts["k3kcompact"], ts["k3kbmh"])]
        e = {"add": entry(ts["k3k"]), "compact": entry(ts["k3kcompact"]), "bagminhash": entry(ts["k3kbmh"]), "chain": entry(tot),
             "form": "lds" if cells <= L else "global", "table_bytes": b1, "groups_per_call": (g1 - g0) // (n1 - n0), "reps": r,
             "total_weight": float(tw.sum().item()), "over_exact_chain": med(tot) / med(k3), "kmers_per_s_add": nk / (med(ts["k3k"]) * 1e-3)}
        chain[str(cells)] = e
        print("chain", cells, e, flush=True)
    out["chain_by_cells"] = chain
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "countsketch_time.json"))
    ap.add_argument("--parent-root", help="checkout of the parent commit, library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k3-reps", type=int, default=20)
    ap.add_argument("--big-reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warm, a.k3_reps)
    res = {"shape": {"genomes": NG, "len": LEN, "k": K, "S": S},
           "timer": f"HIP events, medians of {a.reps} calls after warm-up ({a.big_reps} for tables of 2^24 cells and more, 7 per form in the switch sweep); "
                    "a call's figure is the sum of its launches of that stage over all groups; one fresh process per measurement against the parent"}
    if a.parent_root:
        sides = {"parent": os.path.abspath(a.parent_root), "this": ROOT}
        got = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, root in sides.items():                              # the two take turns
                env = dict(os.environ, D2G_LIB=os.path.join(root, "dashing2_amd", "libd2g.so"))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--reps", str(a.reps), "--warm", str(a.warm),
                                    "--k3-reps", str(a.k3_reps)], capture_output=True, text=True, env=env, timeout=400)
                if r.returncode:
                    raise SystemExit(f"{s}: {r.stderr[-2000:]}")
                got[s].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(s, got[s][-1], flush=True)
        cmp_ = {"parent": got["parent"], "this": got["this"]}
        for key in ("k1_ms", "k3_ms"):
            pm, tm = [x[key] for x in got["parent"]], [x[key] for x in got["this"]]
            cmp_[key] = {"parent_range_of_medians": [min(pm), max(pm)], "this_range_of_medians": [min(tm), max(tm)],
                         "this_median_of_medians": med(tm), "this_inside_or_below_parent_range": med(tm) <= max(pm)}
        cmp_["same_results"] = all(x["checksum"] == got["parent"][0]["checksum"] and x["total_weight"] == got["parent"][0]["total_weight"]
                                   for s in got for x in got[s])
        res["exact_chain_and_k1_vs_parent"] = cmp_
    res["this_tree"] = this_tree(a.reps, a.warm, a.k3_reps, a.big_reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
