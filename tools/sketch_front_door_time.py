#!/usr/bin/env python3
"""The sketch entry layer against the parent commit's library (GPU box):
    python tools/sketch_front_door_time.py --parent-lib PATH/libd2g.so [--parts k1,sketcher,oneshot,bench] [--rounds 5] [--bench-rounds 1]

Every measurement is a fresh process that loads one of the two libraries (D2G_LIB); the two take turns, parent first.
  k1        tools/k1_time.py at its default shape (1000 x 5 Mbp, k = 31, S = 1024): the K1 kernel's event time
  sketcher  the sketcher leg of tools/oph_counts_time.py: wall of d2g_sketcher_run and d2g_sketcher_run_counts, 100 x 5 Mbp
  oneshot   one d2g_oph_sketch (Context.oph_sketch_seqpack) of 500 x 200 kbp at S = 1024, the batch bench.py's K1-built collection
            sends through it: wall of the second of two calls.  Recorded, not judged: the one-shots now live on a sketcher of their own
  bench     one bench.py run each with its sketch (K1) and multiset (K3) legs and nothing else beside the headline (--full without the
            config-4, matrix, CPU-baseline and counter parts: a plain run measures the headline only)
What is judged: this library's median against the parent's own min-max range over the same rounds.  Results are merged into --out."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(what):
    import dashing2_amd as D
    ctx = D.Context(0)
    if what == "sketcher":
        import oph_counts_time
        out = oph_counts_time.sketcher_walls(ctx, D, 100, 5_000_000, 31, 1024)
    else:
        from dashing2_amd import synth
        sp = D.SeqPack(31)
        for i in range(500):
            sp.add_fastx(synth.fasta_bytes_fast(f"g{i}", synth.random_genome(9000 + i, 200_000)))
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            regs = ctx.oph_sketch_seqpack(sp, 1024)
            ts.append((time.perf_counter() - t0) * 1e3)
        out = {"genomes": 500, "len": 200_000, "first_call_ms": ts[0], "second_call_ms": ts[1], "chk": int(regs.sum(dtype=np.uint64) & np.uint64(0xFFFFFFFF))}
    ctx.close()
    print(json.dumps(out))


def run(cmd, lib, limit):
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, D2G_LIB=lib), timeout=limit, cwd=ROOT)
    if r.returncode:
        raise SystemExit(f"{cmd} with {lib}: exit {r.returncode}\n{r.stderr[-2000:]}")     # nothing more is started after a failure
    return r.stdout.strip().splitlines()[-1]


def judge(parent, this):
    m = float(np.median(this))
    return {"parent": parent, "this": this, "parent_min_max": [min(parent), max(parent)], "parent_median": float(np.median(parent)), "this_median": m,
            "this_median_inside_parent_range": bool(min(parent) <= m <= max(parent)), "this_median_below_parent_range": bool(m < min(parent))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parts", default="k1,sketcher,oneshot,bench")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-rounds", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch_front_door.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    sides = (("parent", os.path.abspath(a.parent_lib)), ("this", os.path.join(ROOT, "dashing2_amd", "libd2g.so")))
    me = [sys.executable, os.path.abspath(__file__)]
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res["method"] = "one fresh process per measurement, the parent commit's library and this one taking turns (parent first) on one MI355X in one session"
    parts = a.parts.split(",")
    if "k1" in parts:
        got = {s: [] for s, _ in sides}
        for _ in range(a.rounds):
            for s, lib in sides:
                line = run([sys.executable, os.path.join(ROOT, "tools", "k1_time.py")], lib, 300)
                got[s].append(float(re.search(r": ([0-9.]+) ms", line).group(1)))
                print("k1", s, line, flush=True)
        res["k1_event_ms"] = dict(judge(got["parent"], got["this"]), what="tools/k1_time.py, default shape: mean of 4 launches after 2")
    if "sketcher" in parts:
        got = {s: [] for s, _ in sides}
        for _ in range(a.rounds):
            for s, lib in sides:
                got[s].append(json.loads(run(me + ["--child", "sketcher"], lib, 300)))
                print("sketcher", s, got[s][-1], flush=True)
        for name in ("d2g_sketcher_run_ms", "d2g_sketcher_run_counts_ms"):
            res[name] = dict(judge([x[name] for x in got["parent"]], [x[name] for x in got["this"]]),
                             what="tools/oph_counts_time.py sketcher_walls: 100 x 5 Mbp host arrays in, host arrays out; median of 5 calls after 2")
    if "oneshot" in parts:
        res["oph_sketch_seqpack_500x200kbp"] = {s: json.loads(run(me + ["--child", "oneshot"], lib, 300)) for s, lib in sides}
        res["oph_sketch_seqpack_500x200kbp"]["note"] = "information, not a gate: this one-shot creates a sketcher (a stream, pinned staging) per call"
        print("oneshot", res["oph_sketch_seqpack_500x200kbp"], flush=True)
    if "bench" in parts:
        legs = {s: [] for s, _ in sides}
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--no-config4", "--no-matrices", "--no-cpu-baseline", "--no-traffic"]
        for _ in range(a.bench_rounds):
            for s, lib in sides:
                line = json.loads(run(cmd, lib, 900))
                got = {"headline_pairs_per_s": line["value"]}
                for leg in ("sketch", "multiset_sketch"):
                    if not isinstance(line.get(leg), dict) or "value" not in line[leg]:
                        raise SystemExit(f"bench.py ({s}) gave no {leg} leg: {str(line.get(leg))[:500]}")
                    got[leg] = {"value": line[leg]["value"], "unit": line[leg]["unit"], "ms_per_step": line[leg]["ms_per_step"],
                                "kernel_ms": line[leg]["roofline"].get("kernel_ms")}
                pi = line["sketch"]["parse_inclusive"]       # FASTA in host memory -> registers on the host, through a sketcher's stage
                got["sketch"].update(parse_inclusive_k0_bases_per_s=pi["value"], parse_inclusive_host_parser_bases_per_s=pi["host_parser"]["value"])
                legs[s].append(got)
                print("bench", s, got, flush=True)
        res.pop("bench_default_run", None)
        res["bench_legs"] = dict(legs, cmd=" ".join(cmd[1:]).replace(ROOT + os.sep, ""))
        for leg in ("sketch", "multiset_sketch") if a.bench_rounds > 1 else ():      # one round has no range to judge against
            res["bench_legs"][leg + "_ms_per_step"] = judge([x[leg]["ms_per_step"] for x in legs["parent"]], [x[leg]["ms_per_step"] for x in legs["this"]])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
