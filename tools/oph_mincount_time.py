#!/usr/bin/env python3
"""What sketch -m 2 costs (GPU box): python tools/oph_mincount_time.py [--out profiles/oph_mincount_time.json] [--no-cli]

  genomes   the 20 x 5 Mbp of random packed bases tools/oph_counts_time.py gives d2g_kmer_count (k = 31, S = 1024): nothing occurs twice,
            so the selection kernel counts everything and keeps nothing
  reads     one read-like input made here: a 5 Mbp random genome as 150-base records at 20-fold coverage, either strand, 1 % substitutions
            (666 667 runs of ONE input): the true k-mers occur ~15 times, the k-mers with an error once
  for each  on ONE sketcher, taking turns, medians of 20 after 3 warm-up rounds:
            "k3" events of d2g_sketcher_run_mincount (c = 2)   the chain with the selection kernel (k3_ophmin_kernel)
            "k3" events of d2g_sketcher_run_distinct           the same chain with k3_count_kernel in Distinct mode: no selection
            "k1" event of d2g_sketcher_run                     K1, for scale
            and the walls of the three calls (host arrays in and out)
  cli       wall of `dashing2 sketch -m 2 -o` beside plain `sketch -o` on those inputs as files (20 FASTA of 5 Mbp + the reads as one FASTA
            of 150-base records; -k 31 -S 1024), the variants taking turns, median of 5 after one dropped round"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K, S = 31, 1024


def med(x):
    return float(np.median(np.asarray(x, np.float64)))


def read_codes(L=5_000_000, read_len=150, coverage=20, err=0.01, seed=11):
    """-> base codes uint8 [nreads][read_len]"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, L, dtype=np.uint8)
    nreads = (L * coverage + read_len - 1) // read_len
    starts = rng.integers(0, L - read_len + 1, nreads)
    reads = np.lib.stride_tricks.sliding_window_view(genome, read_len)[starts]             # a copy: [nreads][read_len]
    flip = rng.random(nreads) < 0.5
    reads[flip] = (3 - reads[flip])[:, ::-1]
    sub = rng.random(reads.shape) < err
    reads[sub] = (reads[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
    return reads


def read_stream(reads):
    """the reads as one input of the packed run stream: one run per read, back to back"""
    n, rl = reads.shape
    flat = np.concatenate([reads.reshape(-1), np.zeros((-n * rl) % 4, np.uint8)]).reshape(-1, 4)
    packed = (flat[:, 0] | (flat[:, 1] << 2) | (flat[:, 2] << 4) | (flat[:, 3] << 6)).astype(np.uint8)
    packed = np.concatenate([packed, np.zeros(64, np.uint8)])
    return packed, np.arange(n, dtype=np.uint64) * np.uint64(rl), np.full(n, rl, np.uint32), np.array([0, n], np.uint64)


def chain_times(ctx, D, stream, reps=20, warm=3):
    from dashing2_amd import capi
    packed, rs, rl, go = stream
    n = go.size - 1
    lib, p = capi.lib(), capi._np_ptr
    m = D.oph_m(S)
    regs, nd = np.zeros((n, m), np.uint64), np.zeros(n, np.uint64)
    head = lambda sk: [sk._h, p(packed), packed.size, p(rs), p(rl), rs.size, p(go), n, K, 1, 0]
    sk = ctx.sketcher()
    ev = {"mincount": [], "distinct": [], "k1": []}
    wall = {"mincount": [], "distinct": [], "k1": []}
    kept = 0
    for i in range(warm + reps):
        t0 = time.perf_counter()
        ctx._check(lib.d2g_sketcher_run_mincount(*(head(sk) + [S, 2, p(regs), None])))
        t1 = time.perf_counter()
        a = ctx.kernel_ms("k3")
        kept = int((regs != np.uint64(0xFFFFFFFFFFFFFFFF)).sum())
        t2 = time.perf_counter()
        ctx._check(lib.d2g_sketcher_run_distinct(*(head(sk) + [p(nd)])))
        t3 = time.perf_counter()
        b = ctx.kernel_ms("k3")
        t4 = time.perf_counter()
        ctx._check(lib.d2g_sketcher_run(*(head(sk) + [S, p(regs)])))
        t5 = time.perf_counter()
        c = ctx.kernel_ms("k1")
        assert a[0] == b[0] == c[0] == 1
        if i >= warm:
            for name, e, w in (("mincount", a[2], t1 - t0), ("distinct", b[2], t3 - t2), ("k1", c[2], t5 - t4)):
                ev[name].append(e)
                wall[name].append(w * 1e3)
    sk.close()
    nk = int((rl.astype(np.int64) - K + 1).sum())
    out = {"inputs": n, "runs": int(rs.size), "kmers": nk, "distinct_kmers": int(nd.sum()), "registers_kept_under_c2": kept, "k": K, "S": S}
    for name, key in (("mincount", "k3_run_mincount_c2_ms"), ("distinct", "k3_run_distinct_ms"), ("k1", "k1_ms")):
        out[key] = med(ev[name])
        out[key + "_min_max"] = [min(ev[name]), max(ev[name])]
        out[key.replace("_ms", "_wall_ms")] = med(wall[name])
    out["mincount_over_distinct"] = out["k3_run_mincount_c2_ms"] / out["k3_run_distinct_ms"]
    out["mincount_over_k1"] = out["k3_run_mincount_c2_ms"] / out["k1_ms"]
    return out


def cli_walls(workdir, reads, threads, reps=5):
    from dashing2_amd import synth
    os.makedirs(workdir, exist_ok=True)
    paths = []
    for i in range(20):
        p = os.path.join(workdir, f"g{i:05d}.fa")
        if not os.path.exists(p):
            synth.write_fasta(p, f"g{i:05d}", synth.random_genome(i, 5_000_000))
        paths.append(p)
    rp = os.path.join(workdir, "reads150.fa")
    if not os.path.exists(rp):
        n, rl = reads.shape
        rec = np.empty((n, 3 + rl + 1), np.uint8)
        rec[:, :3] = np.frombuffer(b">r\n", np.uint8)
        rec[:, 3:3 + rl] = np.frombuffer(b"ACGT", np.uint8)[reads]
        rec[:, -1] = 10
        rec.tofile(rp)
    paths.append(rp)
    lst = os.path.join(workdir, "mincount_files.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    variants = (("plain", []), ("m2", ["-m", "2"]))
    ts = {name: [] for name, _ in variants}
    for rep in range(reps + 1):                                        # the first round (cold page cache) is dropped
        for name, flags in variants:
            t0 = time.perf_counter()
            r = subprocess.run([EXE, "sketch", "-k", str(K), "-S", str(S), "-p", str(threads), "-F", lst, "-o", os.path.join(workdir, "mc_stack.bin")] + flags,
                               capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(r.stderr[-2000:])
            if rep:
                ts[name].append(time.perf_counter() - t0)
    out = {"inputs": len(paths), "threads": threads, "reps": reps}
    for name, _ in variants:
        out[name + "_wall_s"] = med(ts[name])
        out[name + "_wall_s_min_max"] = [min(ts[name]), max(ts[name])]
    out["m2_over_plain"] = out["m2_wall_s"] / out["plain_wall_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oph_mincount_time.json"))
    ap.add_argument("--workdir", default="/tmp/d2e2e")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    import dashing2_amd as D
    from oph_counts_time import host_stream
    ctx = D.Context(0)
    ctx.set_timing(D.TIME_K1 | D.TIME_K3)
    res = {"timer": "D2G_TIME_K3 / D2G_TIME_K1 events (the whole K3 chain of one call; the K1 kernel), medians of 20 after 3 warm-up rounds, "
                    "the three calls taking turns on one sketcher; host clocks for the walls"}
    res["genomes_20x5Mbp"] = chain_times(ctx, D, host_stream(20, 5_000_000, seed=6))
    print(json.dumps(res["genomes_20x5Mbp"]), flush=True)
    reads = read_codes()
    res["reads_150b_20x_1pct"] = chain_times(ctx, D, read_stream(reads))
    print(json.dumps(res["reads_150b_20x_1pct"]), flush=True)
    ctx.close()
    if not a.no_cli:
        res["cli"] = cli_walls(a.workdir, reads, a.threads)
        print(json.dumps(res["cli"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
