#!/usr/bin/env python3
"""What exact k-mer sets cost (GPU box): python tools/kset_time.py [--parent-root DIR] [--out profiles/kset_time.json]

Inputs: 64 inputs x 5 Mbp of random packed bases on the device (dashing2_amd.synth's convention: 2 bits per base), k = 31, canonical;
inputs 1 .. 15 are copies of input 0 with about 1 % of their bytes redrawn (a family: their intersections are large), the rest
unrelated (their intersections are empty).

  sorted emission   d2g_kmer_sets_dev: "k3" events = the count chain (hist, scan, scatter, refine, count: the code of the parent's
                    d2g_kmer_count), "k3s" events = the sort behind it (hist, scan, scatter, LDS sort).  With --parent-root (a checkout of
                    the parent commit with its library built) the parent's d2g_kmer_count is timed on the same inputs in a fresh
                    process ("k3" events of its one launch chain); the ratio (k3 + k3s) / parent k3 is the cost of sorting
  pair kernel       d2g_kset_isz_ut_dev over all 2016 pairs, "kset" events; keys per second = the keys of both sets of every pair over
                    the time; achieved bytes = what the K2g section of DESIGN.md predicts the kernel reads (per 4 x 4 tile the slices of
                    eight sets once) over the time
  cpu               reference algorithm, restated: the two-cursor merge as NumPy's intersect1d over sorted arrays, one pair per process
                    thread, timed on a sample of pairs and scaled to all pairs over the CPUs this job is granted

Medians and ranges of `--reps` launches after `--warm` warm-up launches; nothing here asserts a threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG, L, K, FAMILY, TW = 64, 5_000_000, 31, 16, 4


def stats(x):
    x = np.asarray(x, np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def make_inputs(torch):
    stride = ((L + 3) // 4 + 63) // 64 * 64
    torch.manual_seed(7)
    packed = torch.randint(0, 256, (NG * stride + 64,), dtype=torch.uint8, device="cuda")
    g0 = packed[:stride]
    for g in range(1, FAMILY):
        cp = g0.clone()
        pos = torch.randint(0, stride, (stride // 100,), device="cuda")
        cp[pos] = torch.randint(0, 256, (pos.numel(),), dtype=torch.uint8, device="cuda")
        packed[g * stride:(g + 1) * stride] = cp
    rs = np.arange(NG, dtype=np.uint64) * np.uint64(stride * 4)
    return packed, rs, np.full(NG, L, np.uint32), np.arange(NG + 1, dtype=np.uint64)


def parent_child(root):
    """the parent's d2g_kmer_count on the same inputs, in this (fresh) process: one JSON line"""
    sys.path.insert(0, root)
    import torch
    import dashing2_amd as D
    ctx = D.Context(0)
    ctx.set_timing(True)
    packed, rs, rl, go = make_inputs(torch)
    host = packed.cpu().numpy()
    ts = []
    for i in range(3):
        ctx.kmer_count(host, rs, rl, go, K)
        ts.append(ctx.kernel_ms("k3")[2])
    print(json.dumps({"k3_ms": ts[1:], "first_ms": ts[0]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kset_time.json"))
    ap.add_argument("--parent-root")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--cpu-pairs", type=int, default=16)
    ap.add_argument("--parent-child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.parent_child:
        return parent_child(a.parent_child)
    sys.path.insert(0, ROOT)
    import torch
    import dashing2_amd as D
    res = {"shape": {"inputs": NG, "len": L, "k": K, "family": FAMILY},
           "timer": f"HIP events (d2g_set_timing), {a.reps} launches after {a.warm} warm-up launches, one process"}
    ctx = D.Context(0)
    ctx.set_timing(True)
    packed, rs, rl, go = make_inputs(torch)
    plan = ctx.oph_plan(rs, rl, go, K)
    cap = NG * (L - K + 1)
    keys, cnts = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
    off, cards = torch.empty(NG + 1, dtype=torch.int64, device="cuda"), torch.empty(2 * NG, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    k3, k3s = [], []
    for i in range(a.warm + a.reps):
        ctx.kmer_sets_dev(plan, packed.data_ptr(), keys.data_ptr(), cnts.data_ptr(), cap, off.data_ptr(), cards.data_ptr())
        t3, ts = ctx.kernel_ms("k3")[2], ctx.kernel_ms("k3s")[2]
        if i >= a.warm:
            k3.append(t3); k3s.append(ts)
    hoff = off.cpu().numpy().astype(np.int64)
    total = int(hoff[-1])
    res["sorted_emission"] = {"keys": total, "count_chain_k3_ms": stats(k3), "sort_k3s_ms": stats(k3s),
                              "sort_over_count_chain": float(np.median(k3s) / np.median(k3)),
                              "keys_per_s_sorted": total / (np.median(k3s) * 1e-3)}
    if a.parent_root:
        root = os.path.abspath(a.parent_root)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", root], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, D2G_LIB=os.path.join(root, "dashing2_amd", "libd2g.so")))
        if r.returncode:
            res["parent"] = {"error": r.stderr[-1500:]}
        else:
            p = json.loads(r.stdout.strip().splitlines()[-1])
            res["parent"] = {"kmer_count_k3_ms": stats(p["k3_ms"]), "first_launch_ms": p["first_ms"],
                             "this_k3_plus_k3s_over_parent_k3": float((np.median(k3) + np.median(k3s)) / np.median(p["k3_ms"]))}
    else:
        res["parent"] = "not measured (no --parent-root): the count chain above is the parent's code, timed in this process"
    for weighted in (False, True):
        ks = ctx.kset_dev(keys.data_ptr(), cnts.data_ptr() if weighted else None, off.data_ptr(), NG)
        out = torch.empty(NG * (NG - 1) // 2, dtype=torch.int64, device="cuda")
        ts = []
        for i in range(a.warm + a.reps):
            ks.isz_ut_dev(0, NG, out.data_ptr())
            ctx.sync()
            t = ctx.kernel_ms("kset")[2]
            if i >= a.warm:
                ts.append(t)
        sizes = np.diff(hoff)
        pair_keys = float(sum(int(sizes[i]) + int(sizes[j]) for i in range(NG) for j in range(i + 1, NG)))
        nt = (NG + TW - 1) // TW
        tiles = sum(1 for r in range(nt) for c in range(nt) if c >= r)       # 4 x 4 tiles on or above the diagonal (aligned: an upper bound)
        pred_bytes = tiles * 2 * TW * float(sizes.mean()) * (12 if weighted else 8)
        t = np.median(ts) * 1e-3
        res["pair_kernel_countdict" if weighted else "pair_kernel_set"] = {
            "pairs": NG * (NG - 1) // 2, "slice_bits": ks.slice_bits, "resident_bytes": ks.device_bytes, "kset_ms": stats(ts),
            "prepare_ms": ctx.kernel_ms("ksetprep")[2], "keys_per_s": pair_keys / t, "predicted_bytes": pred_bytes,
            "achieved_bytes_per_s_against_prediction": pred_bytes / t, "nonzero_pairs": int((out != 0).sum().item()),
            "largest_intersection": int(out.max().item())}
        ks.close()
    # CPU: reference algorithm, restated
    hk = keys[:total].cpu().numpy().view(np.uint64)
    rng = np.random.default_rng(3)
    pairs = [(0, 1), (0, 2)] + [tuple(sorted(rng.choice(NG, 2, replace=False))) for _ in range(a.cpu_pairs - 2)]
    ts = []
    for i, j in pairs:
        t0 = time.perf_counter()
        np.intersect1d(hk[hoff[i]:hoff[i + 1]], hk[hoff[j]:hoff[j + 1]], assume_unique=True)
        ts.append(time.perf_counter() - t0)
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    ncpu = min(ncpu, int(os.environ.get("OMP_NUM_THREADS", ncpu)))
    cpu_all = float(np.median(ts)) * (NG * (NG - 1) // 2) / ncpu
    res["cpu_baseline"] = {"label": "reference algorithm, restated (NumPy intersect1d of two sorted key arrays per pair; sampled pairs, scaled to all pairs over the granted CPUs)",
                           "pair_s": stats(ts), "cpus": ncpu, "all_pairs_s_scaled": cpu_all,
                           "over_gpu_pair_kernel_set": cpu_all / (res["pair_kernel_set"]["kset_ms"]["median"] * 1e-3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
