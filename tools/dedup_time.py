#!/usr/bin/env python3
"""Times `--greedy 0.5` on one GPU at N = 10 000 and N = 50 000, S = 1024, on the benchmark's matrix (synth.synthetic_registers as
bench.py draws it, densified), split into the count walk ("k2" events), the per-row kernel and the in-order step ("dedup" events;
"dedup_resolve" is the in-order step alone) and the D2H copy of the assignment: median of 20 runs after 3 warm-ups.  Beside it, the
only route to the same answer without the flag: `dashing2 cmp --presketched --square --binary-output` of the same sketches (wall time,
bytes written; clustering that matrix comes on top), and the wall time of `cmp --presketched --greedy 0.5 --binary-output` -- same
machine, same session.  Writes profiles/dedup_time.json.

    python tools/dedup_time.py [--n 10000 50000] [--s 1024] [--t 0.5] [--out profiles/dedup_time.json] [--tmp DIR]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dashing2_amd as D  # noqa: E402
from dashing2_amd import synth  # noqa: E402

EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")


def api_split(ctx, sig, T, runs, warm):
    """d2g_cmp_dedup_dev over the whole set + D2H, timed apart"""
    N, S = sig.shape
    lut = D.epilogue_lut(S, D.SIMILARITY, 31, False)
    cls = np.zeros(S + 1, np.uint32)
    for e in range(1, S + 1):
        cls[e] = cls[e - 1] if lut[e] == lut[e - 1] else e
    hit = np.nonzero(lut >= np.float32(T))[0]
    min_count = int(hit[0]) if hit.size else S + 1
    cs = ctx.cmp_set(sig.view(np.uint64))
    d_cls = ctx.malloc(cls.nbytes)
    ctx.h2d(d_cls, cls)
    d_assign = ctx.malloc(N * 4)
    assign = np.empty(N, np.uint32)
    rec = {k: [] for k in ("count_walk_ms", "per_row_ms", "resolve_ms", "device_wall_ms", "d2h_ms")}
    bands = 0
    try:
        for it in range(warm + runs):
            ctx.set_timing(D.TIME_K2 | D.TIME_DEDUP)
            ctx.kernel_ms("k2"), ctx.kernel_ms("dedup")
            t0 = time.perf_counter()
            cs.dedup_dev(d_assign, min_count, cls_dev_ptr=d_cls)
            ctx.sync()
            t1 = time.perf_counter()
            k2, res, both = ctx.kernel_ms("k2"), ctx.kernel_ms("dedup_resolve", reset=False), ctx.kernel_ms("dedup")
            ctx.set_timing(False)
            t2 = time.perf_counter()
            ctx.d2h(assign, d_assign)
            t3 = time.perf_counter()
            if it >= warm:
                bands = res[0]
                for k, v in (("count_walk_ms", k2[0] * k2[1]), ("per_row_ms", both[0] * both[1] - res[0] * res[1]), ("resolve_ms", res[0] * res[1]),
                             ("device_wall_ms", (t1 - t0) * 1e3), ("d2h_ms", (t3 - t2) * 1e3)):
                    rec[k].append(v)
    finally:
        for p in (d_cls, d_assign):
            ctx.free(p)
    out = {k: statistics.median(v) for k, v in rec.items()}
    out.update({"runs": runs, "warmup": warm, "min_count": min_count, "bands": bands, "clusters": int((assign == np.arange(N)).sum()),
                "algo": {D.CMP_BITSLICE: "bitslice", D.CMP_DIRECT: "direct"}.get(cs.algo, "?"), "bytes_to_host": int(assign.nbytes),
                "counts_walked": N * (N + 1) / 2 + 0.0,           # at least: every band walks its rows x the columns up to its last row
                "resolve_us_per_row": 1e3 * out["resolve_ms"] / N, "resolve_over_count_walk": out["resolve_ms"] / out["count_walk_ms"]})
    cs.close()
    return out


def cli_wall(args, repeats):
    ws = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = subprocess.run([EXE] + args, capture_output=True)
        ws.append(time.perf_counter() - t0)
        if r.returncode != 0:
            raise RuntimeError(r.stderr.decode()[-1500:])
    return statistics.median(ws), ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 50_000])
    ap.add_argument("--s", type=int, default=1024)
    ap.add_argument("--t", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="directory for the sketch stack and the CLI outputs (default: a temporary one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_time.json"))
    a = ap.parse_args()
    S, T = a.s, a.t
    tmp = tempfile.mkdtemp(prefix="d2g_dedup_", dir=a.tmp)
    res = {"S": S, "threshold": T, "measure": "similarity",
           "timer": "D2G_TIME_K2 / D2G_TIME_DEDUP events summed over the bands; host clocks for D2H and the CLI; medians", "rows": []}
    ctx = D.Context(0)
    try:
        for N in a.n:
            regs = synth.synthetic_registers(N, S, nclusters=max(8, N // 150), seed=20260929 if N == 50000 else 20260928)   # bench.py's matrix
            sig, cards = D.oph_finalize(regs, S, nthreads=16)
            del regs
            sig, _ = D.densify(sig, nthreads=16)
            row = {"N": N, "api": api_split(ctx, sig, T, a.runs, a.warmup)}
            stack = os.path.join(tmp, f"stack{N}.bin")
            with open(stack, "wb") as f:
                np.array(sig.shape, np.uint64).tofile(f)
                cards.tofile(f)
                sig.tofile(f)
            del sig
            g_out, sq_out = os.path.join(tmp, "greedy.bin"), os.path.join(tmp, "square.bin")
            w, ws = cli_wall(["cmp", "--presketched", "--greedy", repr(T), "--binary-output", "--cmpout", g_out, "-p", "16", stack], a.cli_repeats)
            row["cli_greedy"] = {"wall_s": w, "walls_s": ws, "bytes_written": os.path.getsize(g_out)}
            # the dense route: the whole square matrix to a file, or -- where it would not fit the disk -- to /dev/null (no file system cost: in the dense route's favour)
            sq_bytes = 4 * N * N
            to_file = shutil.disk_usage(tmp).free > sq_bytes + (2 << 30)
            w, ws = cli_wall(["cmp", "--presketched", "--square", "--binary-output", "--cmpout", sq_out if to_file else "/dev/null", "-p", "16", stack], a.cli_repeats)
            row["cli_square"] = {"wall_s": w, "walls_s": ws, "bytes_written": sq_bytes, "written_to": "file" if to_file else "/dev/null"}
            if to_file:
                assert os.path.getsize(sq_out) == sq_bytes
                os.remove(sq_out)
            os.remove(stack)
            row["square_over_greedy_wall"] = row["cli_square"]["wall_s"] / row["cli_greedy"]["wall_s"]
            row["square_over_greedy_bytes_to_host"] = sq_bytes / row["api"]["bytes_to_host"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    finally:
        ctx.close()
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
