#!/usr/bin/env python3
"""What the screen of `dashing2 contain` costs (GPU box): python tools/screen_time.py [--parent-root DIR] [--out profiles/screen_time.json]

HIP events (D2G_TIME_SCREEN / D2G_TIME_K1), medians of 20 launches after 3 warm-up launches, one MI355X.

  (a) genomes     K1's usual shape -- 1000 genomes x 5 Mbp of random packed bases, k = 31 -- screened against databases of 100, 10 000
                  and 100 000 references x S = 1024 random keys (miss-dominated: a random key is a k-mer of the query with probability
                  ~0).  Per database: distinct keys, table bytes, the build ("screenbuild" events and the wall time of
                  d2g_screen_create, host sort included), screen_count_kernel's time and k-mers/s, the hit rate, screen_reduce_kernel.
                  Beside it, in the same process: K1 with a k-mer filter of the SAME table size attached (tools/filter_time.py's
                  measurement) -- it issues the same one random sector per k-mer and does strictly more behind it.
  (b) reads       150-base reads, 20-fold over a 5 Mbp genome, 1 % substitutions (as tools/oph_mincount_time.py), against 100 references
                  x 1024 of which the first samples the genome itself.
  (c) unchanged   K1 without a screen, this tree against the parent commit in fresh processes taking turns (tools/filter_time.py's child);
                  DIR is a checkout of the parent commit with its library built.
  (d) end to end  `dashing2 contain` wall time on the reads of (b) as a FASTA file, database written by `sketch -s` (--cli).
  (e) CPU         the reference's algorithm RESTATED on the host (tools/screen_cpu_baseline.cpp, compiled here with g++ -O3 -fopenmp: a hash
                  map key -> reference ids, one lookup of maskfn(kmer) per k-mer, one OpenMP thread per file, the granted CPUs) on the
                  reads and database of (b), the reads cut into as many FASTA files as there are threads.  Labelled as what it is: not a
                  dashing2 binary.  Its hit count must equal the GPU's.  --no-cpu skips it."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import filter_time as FT                                                # noqa: E402  (runs(), med(), the K1 loop and the fresh-process child)

NG, L, K, S = FT.NG, FT.L, FT.K, FT.S
NROWS = 4                                                               # 1.25e9 k-mers a row: below the 2^32 guard


def wang64(k):
    k = np.asarray(k, np.uint64)
    u = np.uint64
    with np.errstate(over="ignore"):
        k = ~k + (k << u(21)); k ^= k >> u(24); k = k + (k << u(3)) + (k << u(8)); k ^= k >> u(14)
        k = k + (k << u(2)) + (k << u(4)); k ^= k >> u(28); k += k << u(31)
    return k


def screen_launches(ctx, torch, sc, plan, packed, rows, reps, warm):
    ts = []
    for i in range(warm + reps):
        sc.reset()                                                      # counters are additive: every launch starts a fresh tally
        sc.add_dev(plan, packed.data_ptr(), rows)
        torch.cuda.synchronize()
        t = ctx.kernel_ms("screen")[2]
        if i >= warm:
            ts.append(t)
    return ts


def measure_db(D, torch, ctx, plan, packed, rows, nkmers, keys, reps, warm, with_filter, regs):
    nrefs = keys.shape[0]
    e = {"references": nrefs, "S": keys.shape[1]}
    ctx.kernel_ms("screenbuild")
    t0 = time.perf_counter()
    sc = ctx.screen(keys, K, canon=True, xormask=0, nrows=int(max(rows)) + 1)
    e["create_wall_s"] = time.perf_counter() - t0
    nd, tb, cb = sc.info()
    e.update(distinct=nd, table_bytes=tb, counter_bytes=cb, screenbuild_ms=ctx.kernel_ms("screenbuild")[2])
    ts = screen_launches(ctx, torch, sc, plan, packed, rows, reps, warm)
    e.update(screen_ms=FT.med(ts), min_max=[min(ts), max(ts)], kmers=int(nkmers), kmers_per_s=nkmers / (FT.med(ts) * 1e-3))
    hits = sum(int(sc.key_counts(r)[1].sum(dtype=np.uint64)) for r in range(int(max(rows)) + 1))
    e.update(hits=hits, hit_rate=hits / nkmers)
    rts = []
    for i in range(warm + reps):
        sc.result()
        t = ctx.kernel_ms("screenreduce")[2]
        if i >= warm:
            rts.append(t)
    e["screenreduce_ms"] = FT.med(rts)
    e["screenreduce_pairs"] = (int(max(rows)) + 1) * nrefs
    sc.close()
    if with_filter:                                                     # K1 with a filter of the same table size
        frs, frl, fgo, fstride = FT.runs(1, max(int(nd), K))
        torch.manual_seed(2)
        fpacked = torch.randint(0, 256, (fstride + 64,), dtype=torch.uint8, device="cuda")
        fplan = ctx.oph_plan(frs, frl, fgo, K)
        f = ctx.kmer_filter_dev(fplan, fpacked.data_ptr(), canon=True)
        _, fdist, fbytes = f.info()
        plan.set_filter(f)
        fts = FT.k1_launches(ctx, torch, plan, packed, regs, reps, warm)
        plan.set_filter(None)
        e["k1_with_filter_of_that_size"] = {"filter_distinct": fdist, "filter_table_bytes": fbytes, "k1_ms": FT.med(fts), "min_max": [min(fts), max(fts)],
                                            "screen_over_filtered_k1": e["screen_ms"] / FT.med(fts)}
        f.close(); fplan.close()
        del fpacked
        torch.cuda.empty_cache()
    print(json.dumps(e), flush=True)
    return e


def reads_input(rng, depth=20, rlen=150, sub=0.01):
    """-> (genome codes u8 [L], reads codes u8 [n][rlen])"""
    g = rng.integers(0, 4, L, dtype=np.uint8)
    n = L * depth // rlen
    pos = rng.integers(0, L - rlen, n)
    reads = g[pos[:, None] + np.arange(rlen)[None, :]]
    flip = rng.random(reads.shape) < sub
    reads = np.where(flip, (reads + rng.integers(1, 4, reads.shape, dtype=np.uint8)) & 3, reads).astype(np.uint8)
    return g, reads


def pack2(codes):
    """base p at bits [2 (p % 4), +2) of byte p / 4, 64 bytes of pad"""
    c = np.concatenate([codes.ravel(), np.zeros((-codes.size) % 4, np.uint8)]).reshape(-1, 4)
    b = (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)
    return np.concatenate([b, np.zeros(64, np.uint8)])


def sampled_keys(g, rng, n):
    """masked canonical 31-mers of the genome at n random positions"""
    pos = rng.integers(0, g.size - K, n)
    w = g[pos[:, None] + np.arange(K)[None, :]].astype(np.uint64)
    fwd = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for j in range(K):
        fwd = (fwd << np.uint64(2)) | w[:, j]
        rc = (rc << np.uint64(2)) | (np.uint64(3) - w[:, K - 1 - j])
    return wang64(np.minimum(fwd, rc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_time.json"))
    ap.add_argument("--parent-root", help="checkout of the parent commit, library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--refs", default="100,10000,100000")
    ap.add_argument("--no-cpu", action="store_true", help="skip the host restatement of the reference algorithm")
    ap.add_argument("--cli", action="store_true", help="also time `dashing2 contain` end to end on the read-like query")
    a = ap.parse_args()
    res = {"shape": {"genomes": NG, "len": L, "k": K, "S": S, "rows": NROWS},
           "timer": f"D2G_TIME_SCREEN / D2G_TIME_K1 events, medians of {a.reps} launches after {a.warm} warm-up launches",
           }
    if a.parent_root:                                                   # (c) first: fresh processes, nothing of ours on the GPU yet
        sides = {"parent": os.path.abspath(a.parent_root), "this": ROOT}
        got = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, root in sides.items():
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "filter_time.py"), "--child", root, "--reps", str(a.reps), "--warm", str(a.warm)],
                                   capture_output=True, text=True, timeout=300, env=dict(os.environ, D2G_LIB=os.path.join(root, "dashing2_amd", "libd2g.so")))
                if r.returncode:
                    raise SystemExit(f"{s}: {r.stderr[-2000:]}")
                got[s].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(s, got[s][-1], flush=True)
        pm, tm = [x["k1_ms"] for x in got["parent"]], [x["k1_ms"] for x in got["this"]]
        res["k1_unchanged_vs_parent"] = {"parent": got["parent"], "this": got["this"], "parent_range_of_medians": [min(pm), max(pm)],
                                         "this_range_of_medians": [min(tm), max(tm)], "this_inside_or_below_parent_range": FT.med(tm) <= max(pm)}
    D, torch, ctx, plan, packed, regs = FT.setup(ROOT)
    ctx.set_timing(True)
    rng = np.random.default_rng(7)
    base = FT.k1_launches(ctx, torch, plan, packed, regs, a.reps, a.warm)
    res["k1_unfiltered_ms"] = FT.med(base)
    rows = (np.arange(NG) % NROWS).astype(np.uint32)
    nkmers = NG * (L - K + 1)
    res["genomes"] = []
    for nrefs in [int(x) for x in a.refs.split(",")]:
        keys = rng.integers(0, 1 << 63, (nrefs, S), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        res["genomes"].append(measure_db(D, torch, ctx, plan, packed, rows, nkmers, keys, a.reps, a.warm, True, regs))
        del keys
    plan.close()
    del packed
    torch.cuda.empty_cache()
    # (b) reads
    g, reads = reads_input(rng)
    n, rlen = reads.shape
    rpacked = torch.from_numpy(pack2(reads)).cuda()
    rplan = ctx.oph_plan(np.arange(n, dtype=np.uint64) * np.uint64(rlen), np.full(n, rlen, np.uint32), np.array([0, n], np.uint64), K)
    keys = rng.integers(0, 1 << 63, (100, S), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    keys[0] = sampled_keys(g, rng, S)
    e = measure_db(D, torch, ctx, rplan, rpacked, np.zeros(1, np.uint32), n * (rlen - K + 1), keys, a.reps, a.warm, False, regs)
    e.update(reads=int(n), read_len=int(rlen), depth=20, substitutions=0.01)
    res["reads"] = e
    rplan.close()
    lut = np.frombuffer(b"ACGT", np.uint8)
    rec = np.empty((n, rlen + 4), np.uint8)                             # the reads as FASTA records: ">r\n", the bases, "\n"
    rec[:, :3] = np.frombuffer(b">r\n", np.uint8); rec[:, 3:3 + rlen] = lut[reads]; rec[:, -1] = 10
    if not a.no_cpu:                                                    # (e)
        nth = int(os.environ.get("OMP_NUM_THREADS", "16"))
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "screen_cpu_baseline")
            subprocess.run(["g++", "-O3", "-std=c++17", "-fopenmp", os.path.join(ROOT, "tools", "screen_cpu_baseline.cpp"), "-o", exe], check=True)
            dbp = os.path.join(d, "db.kmer64")
            with open(dbp, "wb") as f:
                f.write(np.array([1 << 8, S, K, K], np.uint32).tobytes() + np.array([0], np.uint64).tobytes() + np.ascontiguousarray(keys).tobytes())
            files = []
            for i, part in enumerate(np.array_split(rec, nth)):
                files.append(os.path.join(d, f"reads{i}.fa"))
                part.tofile(files[-1])
            runs = [json.loads(subprocess.run([exe, dbp] + files, check=True, capture_output=True, text=True,
                                              env=dict(os.environ, OMP_NUM_THREADS=str(nth))).stdout) for _ in range(3)]
        best = min(runs, key=lambda x: x["query_s"])
        if best["hits"] != e["hits"] or best["kmers"] != e["kmers"]:
            raise SystemExit(f"CPU restatement and GPU disagree: {best} against hits {e['hits']}, k-mers {e['kmers']}")
        res["cpu_restatement"] = {"what": "the reference's algorithm restated on the host (tools/screen_cpu_baseline.cpp: std::unordered_map, one lookup per "
                                          "k-mer, one OpenMP thread per file; reading and parsing the FASTA files included); NOT a dashing2 binary",
                                  "query": f"the reads of 'reads' in {nth} FASTA files", "runs": runs, "query_s_median": FT.med([x["query_s"] for x in runs]),
                                  "kmers_per_s_median": FT.med([x["kmers_per_s"] for x in runs]), "hits_equal_the_gpus": True,
                                  "gpu_kernel_over_cpu": (e["screen_ms"] * 1e-3) / FT.med([x["query_s"] for x in runs])}
        print(json.dumps(res["cpu_restatement"]), flush=True)
    if a.cli:                                                           # (d)
        exe = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
        with tempfile.TemporaryDirectory() as d:
            rec.tofile(os.path.join(d, "reads.fa"))
            paths = []
            for i in range(100):
                codes = g if i == 0 else rng.integers(0, 4, 50_000, dtype=np.uint8)
                p = os.path.join(d, f"g{i}.fa")
                with open(p, "wb") as f:
                    f.write(b">g\n" + lut[codes].tobytes() + b"\n")
                paths.append(p)
            db = os.path.join(d, "db")
            subprocess.run([exe, "sketch", "-s", "-k", str(K), "-S", str(S), "-o", db] + paths, check=True, capture_output=True)
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "contain", "-o", os.path.join(d, "out.txt"), db + ".kmer64", os.path.join(d, "reads.fa")], check=True, capture_output=True)
                walls.append(time.perf_counter() - t0)
            first = open(os.path.join(d, "out.txt")).read().split("\n")[3].split("\t")[1]
            res["cli_end_to_end"] = {"query": f"{n} reads x {rlen} bases, FASTA, {os.path.getsize(os.path.join(d, 'reads.fa'))} bytes", "references": 100,
                                     "wall_s": walls, "wall_s_median": FT.med(walls), "entry_of_the_sampled_genome": first}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
