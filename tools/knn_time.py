#!/usr/bin/env python3
"""Times `--topk 10` on one GPU at N = 10 000 and N = 50 000, S = 1024, on the benchmark's matrix (synth.synthetic_registers as
bench.py draws it, densified), split into the count walk ("k2" events), the selection kernel ("knn" events), the D2H copy of the
candidate lists and the host finish (d2g_knn_finish): median of 20 runs after 3 warm-ups.  Beside it, what the dense outputs offer
for the same question: `dashing2 cmp --presketched --square --binary-output` of the same sketches (wall time, bytes written), and
the wall time of `cmp --presketched --topk 10 --binary-output` -- same machine, same session.  Writes profiles/knn_time.json.

    python tools/knn_time.py [--n 10000 50000] [--s 1024] [--k 10] [--out profiles/knn_time.json] [--tmp DIR]
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


def api_split(ctx, sig, K, runs, warm):
    """d2g_cmp_knn_dev over all rows + D2H + d2g_knn_finish, timed apart"""
    N, S = sig.shape
    lut = D.epilogue_lut(S, D.SIMILARITY, 31, False)
    cls = np.zeros(S + 1, np.uint32)
    for e in range(1, S + 1):
        cls[e] = cls[e - 1] if lut[e] == lut[e - 1] else e
    min_count = int(np.nonzero(lut != 0)[0][0])
    cs = ctx.cmp_set(sig.view(np.uint64))
    d_cls = ctx.malloc(cls.nbytes)
    ctx.h2d(d_cls, cls)
    d_cnt = ctx.malloc(N * 4)
    cs.knn_dev(d_cnt, None, None, 0, K=K, min_count=min_count, cls_dev_ptr=d_cls)      # counting only: how long is the longest list?
    rowcnt = np.empty(N, np.uint32)
    ctx.d2h(rowcnt, d_cnt)
    cap = max(2 * K, K + 32)                                   # the default of d2g_cmp_set_knn
    longest = int(rowcnt.max())
    if cap < longest <= 512:
        cap = longest
    d_ids, d_cts = ctx.malloc(N * cap * 4), ctx.malloc(N * cap * 4)
    ids, cts = np.empty(N * cap, np.uint32), np.empty(N * cap, np.uint32)
    rec = {k: [] for k in ("count_walk_ms", "selection_ms", "device_wall_ms", "d2h_ms", "finish_ms")}
    launches = 0
    try:
        for it in range(warm + runs):
            ctx.set_timing(D.TIME_K2 | D.TIME_KNN)
            ctx.kernel_ms("k2"), ctx.kernel_ms("knn")
            t0 = time.perf_counter()
            cs.knn_dev(d_cnt, d_ids, d_cts, cap, K=K, min_count=min_count, cls_dev_ptr=d_cls)
            ctx.sync()
            t1 = time.perf_counter()
            k2, knn = ctx.kernel_ms("k2"), ctx.kernel_ms("knn")
            ctx.set_timing(False)
            t2 = time.perf_counter()
            ctx.d2h(rowcnt, d_cnt), ctx.d2h(ids, d_ids), ctx.d2h(cts, d_cts)
            t3 = time.perf_counter()
            csr = D.knn_finish(np.minimum(rowcnt, cap), ids, cts, cap, lut, False)
            t4 = time.perf_counter()
            if it >= warm:
                launches = knn[0]
                for k, v in (("count_walk_ms", k2[0] * k2[1]), ("selection_ms", knn[0] * knn[1]), ("device_wall_ms", (t1 - t0) * 1e3),
                             ("d2h_ms", (t3 - t2) * 1e3), ("finish_ms", (t4 - t3) * 1e3)):
                    rec[k].append(v)
    finally:
        for p in (d_cls, d_cnt, d_ids, d_cts):
            ctx.free(p)
    out = {k: statistics.median(v) for k, v in rec.items()}
    band_bytes = 4.0 * N * N                                   # every band, once
    out.update({"runs": runs, "warmup": warm, "cap": cap, "longest_list": longest, "rows_beyond_cap": int((rowcnt > cap).sum()),
                "neighbours": int(csr[1].size), "bands": launches, "algo": {D.CMP_BITSLICE: "bitslice", D.CMP_DIRECT: "direct"}.get(cs.algo, "?"),
                "bytes_to_host": int(rowcnt.nbytes + ids.nbytes + cts.nbytes), "band_bytes_all_rows": band_bytes,
                # the histogram form reads a row three times (histogram, count, write), the first time from wherever the count walk left it
                "selection_GBps_one_read": band_bytes / out["selection_ms"] / 1e6, "selection_GBps_three_reads": 3 * band_bytes / out["selection_ms"] / 1e6})
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="directory for the sketch stack and the CLI outputs (default: a temporary one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_time.json"))
    a = ap.parse_args()
    S, K = a.s, a.k
    tmp = tempfile.mkdtemp(prefix="d2g_knn_", dir=a.tmp)
    res = {"S": S, "topk": K, "measure": "similarity", "timer": "D2G_TIME_K2 / D2G_TIME_KNN events summed over the bands; host clocks for D2H, finish and the CLI; medians",
           "rows": []}
    ctx = D.Context(0)
    try:
        for N in a.n:
            regs = synth.synthetic_registers(N, S, nclusters=max(8, N // 150), seed=20260929 if N == 50000 else 20260928)   # bench.py's matrix
            sig, cards = D.oph_finalize(regs, S, nthreads=16)
            del regs
            sig, _ = D.densify(sig, nthreads=16)
            row = {"N": N, "api": api_split(ctx, sig, K, a.runs, a.warmup)}
            stack = os.path.join(tmp, f"stack{N}.bin")
            with open(stack, "wb") as f:
                np.array(sig.shape, np.uint64).tofile(f)
                cards.tofile(f)
                sig.tofile(f)
            del sig
            knn_out, sq_out = os.path.join(tmp, "knn.bin"), os.path.join(tmp, "square.bin")
            w, ws = cli_wall(["cmp", "--presketched", "--topk", str(K), "--binary-output", "--cmpout", knn_out, "-p", "16", stack], a.cli_repeats)
            row["cli_topk"] = {"wall_s": w, "walls_s": ws, "bytes_written": os.path.getsize(knn_out)}
            # the dense route: the whole square matrix to a file, or -- where it would not fit the disk -- to /dev/null (no file system cost: in the dense route's favour)
            sq_bytes = 4 * N * N
            to_file = shutil.disk_usage(tmp).free > sq_bytes + (2 << 30)
            w, ws = cli_wall(["cmp", "--presketched", "--square", "--binary-output", "--cmpout", sq_out if to_file else "/dev/null", "-p", "16", stack], a.cli_repeats)
            row["cli_square"] = {"wall_s": w, "walls_s": ws, "bytes_written": sq_bytes, "written_to": "file" if to_file else "/dev/null"}
            if to_file:
                assert os.path.getsize(sq_out) == sq_bytes
                os.remove(sq_out)
            os.remove(stack)
            row["square_over_topk_wall"] = row["cli_square"]["wall_s"] / row["cli_topk"]["wall_s"]
            row["square_over_topk_bytes_to_host"] = sq_bytes / row["api"]["bytes_to_host"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    finally:
        ctx.close()
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
