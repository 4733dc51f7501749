#!/usr/bin/env python3
"""What the amino-acid walker costs (GPU box): python tools/protein_time.py [--parent-root DIR] [--out profiles/protein_time.json]

Shape: the bench's sketch leg, the one tools/minimizer_time.py uses -- 1000 inputs x 5 M symbols in one run each, S = 1024;
D2G_TIME_K1 events, medians of 20 launches after 3 warm-up launches.

  (a) K1a against DNA K1   d2g_oph_sketch_dev over a byte-per-residue stream of 20 letters at k = 5 and k = 14, each against DNA K1 at
                           the SAME k over the same number of symbols -- the same number of k-mers -- in the same run; DNA K1 at
                           k = 31 beside them (the bench's k)
  (b) --parse-by-seq       10^5 records of 300 residues, one genome per record, k = 5, S = 256: k-mers/s beside the whole-file figure

  (c) DNA K1 unchanged     plain DNA K1 (k = 31) of this tree against the parent commit: DIR is a checkout of the parent commit with its
                           library built.  One fresh process per measurement, the two taking turns; the run-to-run range of a side is
                           the range of its medians.  The DNA kernels are the parent's instruction for instruction
                           (profiles/protein_resource_usage.txt), so anything but "inside the parent's range" is a finding"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG, L, S = 1000, 5_000_000, 1024
A20 = 2                                                                # D2G_ALPHABET_PROTEIN20


def med(x):
    return float(np.median(np.asarray(x, np.float64)))


def runs(ng, length, per_byte):
    """one run per genome, each at a 64-byte boundary of the stream -> (run_start, run_len, genome_run_off, bytes between starts)"""
    stride = ((length + per_byte - 1) // per_byte + 63) // 64 * 64
    return (np.arange(ng, dtype=np.uint64) * np.uint64(stride * per_byte), np.full(ng, length, np.uint32), np.arange(ng + 1, dtype=np.uint64), stride)


def launches(ctx, torch, call, reps, warm):
    ts = []
    for i in range(warm + reps):
        call()
        torch.cuda.synchronize()
        t = ctx.kernel_ms("k1")[2]
        if i >= warm:
            ts.append(t)
    return ts


def leg(ctx, torch, D, packed, regs, ng, length, k, s, alphabet, reps, warm):
    rs, rl, go, _ = runs(ng, length, 1 if alphabet else 4)
    plan = ctx.oph_plan(rs, rl, go, k, alphabet=alphabet)
    ts = launches(ctx, torch, lambda: ctx.oph_sketch_dev(plan, packed.data_ptr(), s, regs.data_ptr(), canon=not alphabet), reps, warm)
    e = {"ms": med(ts), "min_max": [min(ts), max(ts)], "kmers": plan.nkmers, "kmers_per_s": plan.nkmers / (med(ts) * 1e-3)}
    plan.close()
    return e


def child(root, reps, warm):
    """one measurement of plain DNA K1 from the tree at `root`, in this (fresh) process: one JSON line.  Only what the parent's
    binding has too is called"""
    sys.path.insert(0, root)
    import torch
    import dashing2_amd as D
    ctx = D.Context(0)
    ctx.set_timing(True)
    rs, rl, go, stride = runs(NG, L, 4)
    torch.manual_seed(1)
    packed = torch.randint(0, 256, (NG * stride + 64,), dtype=torch.uint8, device="cuda")
    regs = torch.empty((NG, D.oph_m(S)), dtype=torch.int64, device="cuda")
    plan = ctx.oph_plan(rs, rl, go, 31)
    ts = launches(ctx, torch, lambda: ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr()), reps, warm)
    print(json.dumps({"k1_ms": med(ts), "min_max": [min(ts), max(ts)], "checksum": int(regs.sum().item()) & 0xFFFFFFFF}), flush=True)


def against_parent(parent_root, rounds, reps, warm):
    sides = {"parent": os.path.abspath(parent_root), "this": ROOT}
    got = {s: [] for s in sides}
    for _ in range(rounds):
        for s, root in sides.items():                                  # the two take turns
            env = dict(os.environ, D2G_LIB=os.path.join(root, "dashing2_amd", "libd2g.so"))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--reps", str(reps), "--warmup", str(warm)],
                               capture_output=True, text=True, env=env, timeout=300)
            if r.returncode:
                raise SystemExit(f"{s}: {r.stderr[-2000:]}")
            got[s].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(s, got[s][-1], flush=True)
    pm, tm = [x["k1_ms"] for x in got["parent"]], [x["k1_ms"] for x in got["this"]]
    assert len({x["checksum"] for x in got["parent"] + got["this"]}) == 1, "the two trees computed different registers"
    return {"parent": got["parent"], "this": got["this"], "parent_range_of_medians": [min(pm), max(pm)],
            "this_range_of_medians": [min(tm), max(tm)], "this_median_of_medians": med(tm),
            "this_inside_parent_range": min(pm) <= med(tm) <= max(pm), "this_inside_or_below_parent_range": med(tm) <= max(pm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "protein_time.json"))
    ap.add_argument("--parent-root", help="checkout of the parent commit, library built")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    vs_parent = against_parent(a.parent_root, a.rounds, a.reps, a.warmup) if a.parent_root else None
    sys.path.insert(0, ROOT)
    import torch
    import dashing2_amd as D
    ctx = D.Context(0)
    ctx.set_timing(True)
    torch.manual_seed(1)
    out = {"shape": {"inputs": NG, "symbols_per_input": L, "S": S, "reps": a.reps, "warmup": a.warmup}, "k1": {}, "by_seq": {}}
    if vs_parent:
        out["dna_k31_vs_parent"] = vs_parent
    regs = torch.empty((NG, D.oph_m(S)), dtype=torch.int64, device="cuda")
    stride4, stride1 = runs(NG, L, 4)[3], runs(NG, L, 1)[3]
    dna = torch.randint(0, 256, (NG * stride4 + 64,), dtype=torch.uint8, device="cuda")
    for k in (31, 5, 14):
        out["k1"][f"dna_k{k}"] = leg(ctx, torch, D, dna, regs, NG, L, k, S, 0, a.reps, a.warmup)
        print(f"dna k{k}", out["k1"][f"dna_k{k}"], flush=True)
    del dna
    aa = torch.randint(0, 20, (NG * stride1 + 64,), dtype=torch.uint8, device="cuda")
    for k in (5, 14):
        e = leg(ctx, torch, D, aa, regs, NG, L, k, S, A20, a.reps, a.warmup)
        e["over_dna_same_k"] = e["ms"] / out["k1"][f"dna_k{k}"]["ms"]
        out["k1"][f"protein20_k{k}"] = e
        print(f"protein20 k{k}", e, flush=True)
    # --parse-by-seq: every record its own genome
    nrec, rlen, k, s = 100_000, 300, 5, 256
    regs2 = torch.empty((nrec, D.oph_m(s)), dtype=torch.int64, device="cuda")
    e = leg(ctx, torch, D, aa, regs2, nrec, rlen, k, s, A20, a.reps, a.warmup)
    e.update(records=nrec, residues_per_record=rlen, k=k, S=s, whole_file_kmers_per_s=out["k1"]["protein20_k5"]["kmers_per_s"])
    out["by_seq"] = e
    print("by-seq", e, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
