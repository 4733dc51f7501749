#!/usr/bin/env python3
"""What sketch -N costs (GPU box): python tools/oph_counts_time.py [--out profiles/oph_counts_time.json] [--no-cli]

  kernels   K1 ("k1") and its count pass ("k1count") on the bench's sketch-leg shape, the one tools/k1_time.py uses: 1000 genomes x
            5 Mbp of random packed bases, k = 31, S = 1024; D2G_TIME_K1 events, median of 20 launches after 3 warm-up launches
            (K1 alternating with the count pass), and K1 alone, launched back to back as tools/k1_time.py does
  sketcher  wall of d2g_sketcher_run_counts against d2g_sketcher_run (host arrays in, host arrays out) on 100 of those genomes
  exact     for comparison only: d2g_kmer_count, the exact-counter route the design declined ("k3" events and wall), and K1 + count
            pass on the same 20 genomes (its outputs hold one entry per k-mer, so it cannot take the full shape)
  cli       wall of `dashing2 sketch -o` plain, with -s and with -N on tools/e2e_cli.py's inputs (200 x 5 Mbp FASTA, -k 31 -S 1024), median of 7"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")


def med(x):
    return float(np.median(np.asarray(x, np.float64)))


def runs(ng, L):
    stride = ((L + 3) // 4 + 63) // 64 * 64
    return (np.arange(ng, dtype=np.uint64) * np.uint64(stride * 4), np.full(ng, L, np.uint32), np.arange(ng + 1, dtype=np.uint64), stride)


def kernel_times(ctx, D, torch, ng, L, k, S, reps=20, warm=3):
    rs, rl, go, stride = runs(ng, L)
    packed = torch.randint(0, 256, (ng * stride + 64,), dtype=torch.uint8, device="cuda")
    plan = ctx.oph_plan(rs, rl, go, k)
    m = D.oph_m(S)
    regs = torch.empty((ng, m), dtype=torch.int64, device="cuda")
    cnts = torch.empty((ng, m), dtype=torch.int32, device="cuda")
    t1, tc = [], []
    for i in range(warm + reps):
        ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr())
        ctx.oph_count_dev(plan, packed.data_ptr(), S, regs.data_ptr(), cnts.data_ptr())
        torch.cuda.synchronize()
        a, b = ctx.kernel_ms("k1")[2], ctx.kernel_ms("k1count")[2]
        if i >= warm:
            t1.append(a)
            tc.append(b)
    total = int(cnts.to(torch.int64).sum().item())
    plan.close()
    return {"genomes": ng, "len": L, "k": k, "S": S, "bases": ng * L, "k1_ms": med(t1), "k1_ms_min_max": [min(t1), max(t1)],
            "k1count_ms": med(tc), "k1count_ms_min_max": [min(tc), max(tc)], "k1count_over_k1": med(tc) / med(t1),
            "k1_bases_per_s": ng * L / med(t1) * 1e3, "k1count_bases_per_s": ng * L / med(tc) * 1e3, "sum_of_counts": total}


def k1_alone(ctx, D, torch, ng, L, k, S, reps=20, warm=3):
    """K1 launched back to back with nothing in between, as tools/k1_time.py launches it: what to hold against that tool's figure
    for the parent commit (in `kernel_times` K1 alternates with the count pass)"""
    rs, rl, go, stride = runs(ng, L)
    packed = torch.randint(0, 256, (ng * stride + 64,), dtype=torch.uint8, device="cuda")
    plan = ctx.oph_plan(rs, rl, go, k)
    regs = torch.empty((ng, D.oph_m(S)), dtype=torch.int64, device="cuda")
    ts = []
    for i in range(warm + reps):
        ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr())
        torch.cuda.synchronize()
        t = ctx.kernel_ms("k1")[2]
        if i >= warm:
            ts.append(t)
    plan.close()
    return {"k1_alone_ms": med(ts), "k1_alone_ms_min_max": [min(ts), max(ts)]}


def host_stream(ng, L, seed=5):
    rs, rl, go, stride = runs(ng, L)
    packed = np.random.default_rng(seed).integers(0, 256, ng * stride + 64, dtype=np.uint8)
    return packed, rs, rl, go


def sketcher_walls(ctx, D, ng, L, k, S, reps=5, warm=2):
    from dashing2_amd import capi
    packed, rs, rl, go = host_stream(ng, L)
    m = D.oph_m(S)
    regs, cnts = np.empty((ng, m), np.uint64), np.empty((ng, m), np.uint32)
    sk = ctx.sketcher()
    lib, p = capi.lib(), capi._np_ptr
    out = {}
    for name in ("d2g_sketcher_run", "d2g_sketcher_run_counts"):
        ts = []
        for i in range(warm + reps):
            t0 = time.perf_counter()
            args = [sk._h, p(packed), packed.size, p(rs), p(rl), rs.size, p(go), ng, k, 1, 0, S, p(regs)]
            ctx._check(getattr(lib, name)(*(args + ([p(cnts)] if name.endswith("counts") else []))))
            if i >= warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms"] = med(ts)
    sk.close()
    out.update(genomes=ng, len=L, counts_over_plain=out["d2g_sketcher_run_counts_ms"] / out["d2g_sketcher_run_ms"])
    return out


def exact_route(ctx, D, ng, L, k, S, reps=5, warm=1):
    """the library calls themselves (no sorting of the result, output arrays allocated and touched once, outside the clock)"""
    from dashing2_amd import capi
    packed, rs, rl, go = host_stream(ng, L, seed=6)
    lib, p = capi.lib(), capi._np_ptr
    cap = ng * (L - k + 1)
    keys, counts, off = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(ng + 1, np.uint64)
    m = D.oph_m(S)
    regs, cnts = np.zeros((ng, m), np.uint64), np.zeros((ng, m), np.uint32)
    ctx.set_timing(D.TIME_K1 | D.TIME_K3)
    ts, tk, k3, k1 = [], [], [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        ctx._check(lib.d2g_kmer_count(ctx._h, p(packed), packed.size, p(rs), p(rl), rs.size, p(go), ng, k, 1, 0, 0.0, p(keys), p(counts), cap, p(off)))
        t1 = time.perf_counter()
        ctx._check(lib.d2g_oph_sketch_counts(ctx._h, p(packed), packed.size, p(rs), p(rl), rs.size, p(go), ng, k, 1, 0, S, p(regs), p(cnts)))
        t2 = time.perf_counter()
        n3, a3, _ = ctx.kernel_ms("k3")
        ka, kb = ctx.kernel_ms("k1")[2], ctx.kernel_ms("k1count")[2]
        if i >= warm:
            ts.append((t1 - t0) * 1e3)
            tk.append((t2 - t1) * 1e3)
            k3.append(n3 * a3)
            k1.append(ka + kb)
    ctx.set_timing(False)
    return {"genomes": ng, "len": L, "bases": ng * L, "distinct_kmers": int(off[ng]), "d2g_kmer_count_wall_ms": med(ts), "d2g_kmer_count_k3_events_ms": med(k3),
            "d2g_oph_sketch_counts_wall_ms": med(tk), "k1_plus_k1count_events_ms": med(k1), "k3_over_k1_plus_k1count": med(k3) / med(k1),
            "note": "host arrays in and out; the exact counter returns one (key, count) per distinct k-mer (12 bytes each across PCIe), d2g_oph_sketch_counts 12 m bytes per genome"}


def cli_walls(workdir, genomes, L, threads, reps=7):
    from dashing2_amd import synth
    os.makedirs(workdir, exist_ok=True)
    paths = []
    for i in range(genomes):
        p = os.path.join(workdir, f"g{i:05d}.fa")
        if not os.path.exists(p):
            synth.write_fasta(p, f"g{i:05d}", synth.random_genome(i, L))
        paths.append(p)
    lst = os.path.join(workdir, "files.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    out = {"genomes": genomes, "len": L, "threads": threads, "reps": reps}
    variants = (("plain", []), ("save_kmers", ["-s"]), ("save_kmercounts", ["-N"]))
    ts = {name: [] for name, _ in variants}
    for rep in range(reps + 1):                                        # the variants take turns; the first round (cold page cache) is dropped
        for name, flags in variants:
            t0 = time.perf_counter()
            r = subprocess.run([EXE, "sketch", "-k", "31", "-S", "1024", "-p", str(threads), "-F", lst, "-o", os.path.join(workdir, "stack.bin")] + flags,
                               capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(r.stderr[-2000:])
            if rep:
                ts[name].append(time.perf_counter() - t0)
    for name, _ in variants:
        out[name + "_wall_s"] = med(ts[name])
        out[name + "_wall_s_min_max"] = [min(ts[name]), max(ts[name])]
    out["save_kmercounts_over_plain"] = out["save_kmercounts_wall_s"] / out["plain_wall_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oph_counts_time.json"))
    ap.add_argument("--workdir", default="/tmp/d2e2e")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    import torch
    import dashing2_amd as D
    ctx = D.Context(0)
    ctx.set_timing(D.TIME_K1)
    res = {"timer": "D2G_TIME_K1 events (k1, k1count), medians of 20 launches after 3 warm-up launches; host clocks for the walls",
           "kernels": kernel_times(ctx, D, torch, 1000, 5_000_000, 31, 1024)}
    res["kernels"].update(k1_alone(ctx, D, torch, 1000, 5_000_000, 31, 1024))
    print(json.dumps(res["kernels"]), flush=True)
    res["kernels_20_genomes"] = kernel_times(ctx, D, torch, 20, 5_000_000, 31, 1024)
    torch.cuda.empty_cache()
    ctx.set_timing(False)
    res["sketcher"] = sketcher_walls(ctx, D, 100, 5_000_000, 31, 1024)
    print(json.dumps(res["sketcher"]), flush=True)
    res["exact_counter_for_comparison"] = exact_route(ctx, D, 20, 5_000_000, 31, 1024)
    print(json.dumps(res["exact_counter_for_comparison"]), flush=True)
    ctx.close()
    if not a.no_cli:
        res["cli"] = cli_walls(a.workdir, 200, 5_000_000, a.threads)
        print(json.dumps(res["cli"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
