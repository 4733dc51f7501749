#!/usr/bin/env python3
"""What exact edit distances cost (GPU box): python tools/edit_time.py [--out profiles/edit_time.json] [--reps 20] [--budget 45]

One process, the device-resident entry point d2g_edit_ut_dev over the whole upper triangle of each shape, HIP events ("edit"), medians:

  reads150     10 000 records x 150 DNA symbols
  genes1500     2 000 x 1 500 DNA
  long10000       500 x 10 000 DNA          (queries of several strips)
  protein300   20 000 x about 300 (250 .. 350) over 20 letters
  ragged        3 000 records, lengths log-uniform 50 .. 5 000, DNA

Records of a shape are mutated copies of a few ancestors, as reads of one amplicon or genes of one family are.  `--reps` launches after
one warm-up; a shape whose warm-up shows that they would take more than `--budget` seconds gets fewer (at least 3; "n" says how many).

Reported per shape: milliseconds, pairs/s, cells/s (cells = the sum of m n over the pairs), the fraction of the VALU bound of DESIGN.md
section 3 K2h (VALU_PER_WORD_STEP instructions per 32 rows x 64 lanes, 4 cycles each, 4 SIMDs per CU), the packing factors B/P and
n/(n + P - 1) of the mean record, and the CPU baseline: tools/edit_cpu_baseline.cpp -- this repository's own restatement of block Myers
with 64-bit words, one thread per row, on the CPUs this job is granted -- timed on every `step`-th row and scaled by cells.  The sum of
its distances over those rows must equal the GPU's.  It is not edlib and not a dashing2 binary.  Nothing here asserts a threshold."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALU_PER_WORD_STEP = 35          # read from the ISA listing of the inner loop (profiles/edit_resource_usage.txt)
CLOCK_HZ = 2.4e9


def stats(x):
    x = np.asarray(x, np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def family(rng, n, lens, letters, ancestors=8, rate=0.05):
    alphabet = np.frombuffer(letters, np.uint8)
    top = int(max(lens))
    anc = [rng.choice(alphabet, top) for _ in range(ancestors)]
    recs = []
    for i in range(n):
        x = anc[i % ancestors][:int(lens[i])].copy()
        pos = rng.integers(0, x.size, max(1, int(x.size * rate)))
        x[pos] = rng.choice(alphabet, pos.size)
        recs.append(x.tobytes())
    return recs


def shapes(rng):
    yield "reads150", family(rng, 10000, np.full(10000, 150), b"ACGT")
    yield "genes1500", family(rng, 2000, np.full(2000, 1500), b"ACGT")
    yield "long10000", family(rng, 500, np.full(500, 10000), b"ACGT")
    yield "protein300", family(rng, 20000, rng.integers(250, 351, 20000), b"ACDEFGHIKLMNPQRSTVWY")
    yield "ragged", family(rng, 3000, np.exp(rng.uniform(np.log(50), np.log(5000), 3000)).astype(np.int64), b"ACGT")


def cpu_baseline(exe, recs, step, threads, gpu_tri, N):
    lens = np.array([len(r) for r in recs], np.uint64)
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(np.uint64(N).tobytes() + off.tobytes() + b"".join(recs))
        path = f.name
    try:
        j = json.loads(subprocess.check_output([exe, path, "0", str(N), str(step), str(threads)], text=True))
    finally:
        os.unlink(path)
    rowstart = np.concatenate([[0], np.cumsum(N - 1 - np.arange(N))]).astype(np.int64)
    want = sum(int(gpu_tri[rowstart[r]:rowstart[r + 1]].sum(dtype=np.int64)) for r in range(0, N, step))
    j["step"] = step
    j["sum_equals_gpu"] = bool(j["sum"] == want)
    return j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=float, default=45.0, help="seconds of launches per shape")
    ap.add_argument("--cpu-seconds", type=float, default=8.0, help="aim of the CPU baseline's sample per shape")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    import dashing2_amd as D
    exe = os.path.join(tempfile.gettempdir(), "edit_cpu_baseline")
    subprocess.check_call(["g++", "-O3", "-march=native", "-fopenmp", "-o", exe, os.path.join(ROOT, "tools", "edit_cpu_baseline.cpp")])
    threads = min(16, len(os.sched_getaffinity(0)))
    ctx = D.Context(0)
    ctx.set_timing(D.TIME_EDIT)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    bound = ncu * 4 * CLOCK_HZ / (VALU_PER_WORD_STEP * 4) * 64 * 32
    res = {"device": torch.cuda.get_device_name(0), "cus": ncu, "valu_per_word_step": VALU_PER_WORD_STEP, "clock_hz": CLOCK_HZ,
           "valu_bound_cells_per_s": bound, "cpu_threads": threads, "shapes": {}}
    rng = np.random.default_rng(7500)
    for name, recs in shapes(rng):
        if a.only and name not in a.only.split(","):
            continue
        N = len(recs)
        lens = np.array([len(r) for r in recs], np.float64)
        suffix = np.concatenate([np.cumsum(lens[::-1])[::-1][1:], [0.0]])
        cells, pairs = float((lens * suffix).sum()), N * (N - 1) // 2
        ss = ctx.seqset(recs)
        prep_ms = ctx.kernel_ms("editprep")[2]
        out = torch.zeros(pairs, dtype=torch.int32, device="cuda")
        ss.edit_ut_dev(0, N, out.data_ptr())
        ctx.sync()
        t1 = ctx.kernel_ms("edit")[2] * 1e-3
        reps = int(max(3, min(a.reps, a.budget / max(t1, 1e-6))))
        print(f"[edit_time] {name}: N={N} mean length {lens.mean():.0f} warm-up {t1 * 1e3:.1f} ms, {reps} launches", flush=True)
        ts = []
        for _ in range(reps):
            ss.edit_ut_dev(0, N, out.data_ptr())
            ctx.sync()
            ts.append(ctx.kernel_ms("edit")[2])
        tri = out.cpu().numpy().view(np.uint32)
        t = float(np.median(ts)) * 1e-3
        m = float(lens.mean())
        B = int(np.ceil(m / 32))
        strip = ss.strip_blocks
        P = 64 if B > strip else 1 << int(np.ceil(np.log2(max(B, 1))))
        Bs = min(B, strip)
        cpu_rate_guess = 2e9 * threads
        step = int(max(1, min(N // (2 * threads) or 1, cells / cpu_rate_guess / a.cpu_seconds)))
        cpu = cpu_baseline(exe, recs, step, threads, tri, N)
        cpu_all = cpu["seconds"] * cells / max(cpu["cells"], 1.0)
        res["shapes"][name] = {
            "records": N, "mean_length": m, "max_length": int(lens.max()), "alphabet": ss.alphabet_size, "pairs": pairs, "cells": cells,
            "resident_bytes": ss.device_bytes, "prepare_ms": prep_ms, "edit_ms": stats(ts), "pairs_per_s": pairs / t, "cells_per_s": cells / t,
            "fraction_of_valu_bound": cells / t / bound,
            "packing": {"blocks": B, "lanes_per_pair": P, "B_over_P": Bs / P, "n_over_n_plus_P_minus_1": m / (m + Bs - 1), "strips": int(np.ceil(B / strip))},
            "cpu_baseline": {"what": "tools/edit_cpu_baseline.cpp: this repository's block Myers, 64-bit words, one thread per row", "sampled": cpu,
                             "seconds_all_rows_scaled_by_cells": cpu_all, "cells_per_s": cpu["cells"] / cpu["seconds"], "over_gpu": cpu_all / t},
        }
        print(f"[edit_time] {name}: {t * 1e3:.1f} ms, {cells / t:.3e} cells/s = {cells / t / bound:.3f} of the bound; CPU x{cpu_all / t:.0f} "
              f"(sum equal: {cpu['sum_equals_gpu']})", flush=True)
        ss.close()
        del out
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: {"ms": v["edit_ms"]["median"], "cells_per_s": v["cells_per_s"], "bound": v["fraction_of_valu_bound"], "cpu_over_gpu": v["cpu_baseline"]["over_gpu"]}
                      for k, v in res["shapes"].items()}))


if __name__ == "__main__":
    main()
