#!/usr/bin/env python3
"""Times greedy clustering by edit distance (K2j, d2g_edit_dedup_dev) on one MI355X and writes profiles/edit_dedup_time.json.

One process, device-resident entry points, HIP events (the library's own brackets), medians of `--reps` (20) calls after a warm-up call,
with the range beside each median.  `--budget SECONDS` (a quick look; not for the committed file) lets a slow measurement run fewer calls.

Per shape and bound:
  dispatcher_ms  d2g_edit_dedup_dev as the library routes it (D2G_EDIT_DEDUP_ROUTE unset)                     ["editdedup", one bracket per band, summed]
  route1_ms      the list kernel wherever it exists (D2G_EDIT_DEDUP_ROUTE=1)
  route2_ms      d2g_edit_near_dev over all columns for every row, then the best key per row (D2G_EDIT_DEDUP_ROUTE=2)
  resolve_share, list_share   of the dispatcher's time: the in-order step ["editdedup_resolve"], the two kernels that compact the
                 representative list ["editdedup_list"]
  yardstick_ms   the parent commit's code only: d2g_edit_near_dev over all rows x all columns in bands of 256 rows ["editnear" + "edit"]:
                 what any clustering without a representative list pays before it decides anything
  clusters       of the dispatcher's result (the three routes' results are compared word for word)
  dispatcher_ok  dispatcher median <= the faster forced route's median + that route's own max - min
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DNA = np.frombuffer(b"ACGT", np.uint8)
BAND = 256


def stats(x):
    x = np.asarray(x, np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def from_templates(rng, n, length, ntemplates, rate=None, one_error=False):
    """n records of `length` symbols: a template each, with substitutions at `rate` per symbol, or (one_error) with one substitution in
    half of the records.  -> (bytes u8 [n * length], off u64 [n + 1])"""
    t = rng.choice(DNA, (ntemplates, length))
    x = t if ntemplates == n else t[rng.integers(0, ntemplates, n)]      # ntemplates == n: one template per record, none twice
    if one_error:
        hit = np.zeros((n, length), bool)
        rows = np.nonzero(rng.random(n) < 0.5)[0]
        hit[rows, rng.integers(0, length, rows.size)] = True
    else:
        hit = rng.random((n, length)) < rate
    x = np.where(hit, rng.choice(DNA, (n, length)), x)
    return np.ascontiguousarray(x, np.uint8).reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length)


def shapes(rng, scale):
    n100, n20 = max(512, int(100000 * scale)), max(512, int(20000 * scale))
    yield "umis12_100k", "100 000 UMIs of 12 symbols from 2 000 templates, at most one error", from_templates(rng, n100, 12, 2000, one_error=True), [1]
    yield "reads150_100k", "100 000 reads x 150 from 1 000 templates at 1 % errors", from_templates(rng, n100, 150, 1000, 0.01), [3, 15]
    yield "genes1500_20k", "20 000 x 1 500 from 200 templates at 1 % errors", from_templates(rng, n20, 1500, 200, 0.01), [31]
    yield "unrelated150_20k", "20 000 x 150, all unrelated (C = N: the worst case for the list)", from_templates(rng, n20, 150, n20, 0.0), [3]
    one = from_templates(rng, 1, 150, 1, 0.0)[0]
    yield "copies150_20k", "20 000 copies of one read (C = 1)", (np.tile(one, n20), np.arange(n20 + 1, dtype=np.uint64) * np.uint64(150)), [3]


class Bench:
    def __init__(self, a):
        import torch
        import dashing2_amd as D
        self.torch, self.D, self.a = torch, D, a
        self.ctx = D.Context(0)
        self.ctx.set_timing(D.TIME_EDIT | D.TIME_EDIT_NEAR | D.TIME_EDIT_DEDUP)

    def route(self, r):
        if r:
            os.environ["D2G_EDIT_DEDUP_ROUTE"] = str(r)
        else:
            os.environ.pop("D2G_EDIT_DEDUP_ROUTE", None)
        self.ctx.reload_tuning()

    def timed(self, launch, names):
        """per name, the brackets of one call summed; the first call is the warm-up and sizes the number of calls"""
        def once():
            for n in names:
                self.ctx.kernel_ms(n)
            launch()
            self.ctx.sync()
            out = {}
            for n in names:
                c, avg, _ = self.ctx.kernel_ms(n)
                out[n] = c * avg
            return out
        first = once()
        reps = self.a.reps
        if self.a.budget > 0:
            reps = int(max(3, min(reps, self.a.budget / max(sum(first.values()) * 1e-3, 1e-6))))
        runs = [once() for _ in range(reps)]
        return {n: stats([r[n] for r in runs]) for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_dedup_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=float, default=0.0, help="seconds of calls per measurement; 0 = no limit, always --reps calls")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every shape's N (a quick look; not for the committed file)")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    b = Bench(a)
    torch, ctx = b.torch, b.ctx
    res = {"device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "band_rows": BAND,
           "reps": a.reps, "budget_s": a.budget, "scale": a.scale, "shapes": {}}

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    rng = np.random.default_rng(7700)
    for name, what, (data, off), bounds in shapes(rng, a.scale):
        if a.only and name not in a.only.split(","):
            continue
        N = off.size - 1
        ss = ctx.seqset(data=data, off=off)
        assign = torch.zeros(N, dtype=torch.int32, device="cuda")
        band = torch.zeros(BAND * N, dtype=torch.int32, device="cuda")
        for T in bounds:
            e = {"what": what, "N": N, "T": T}
            got = {}
            for r, key in ((0, "dispatcher_ms"), (1, "route1_ms"), (2, "route2_ms")):
                b.route(r)
                t = b.timed(lambda: ss.dedup_dev(assign.data_ptr(), T), ["editdedup", "editdedup_resolve", "editdedup_list"])
                e[key] = t["editdedup"]
                got[r] = assign.cpu().numpy().copy()
                if r == 0:
                    e["resolve_share"] = t["editdedup_resolve"]["median"] / t["editdedup"]["median"]
                    e["list_share"] = t["editdedup_list"]["median"] / t["editdedup"]["median"]
            b.route(0)
            assert (got[0] == got[1]).all() and (got[0] == got[2]).all(), "the routes disagree"
            e["clusters"] = int((got[0] == np.arange(N)).sum())
            assert name != "unrelated150_20k" or e["clusters"] == N, "the unrelated shape must have a cluster per record"

            def yard():
                for a0 in range(0, N, BAND):
                    ss.near_dev(T, band.data_ptr(), a0, min(a0 + BAND, N))
            y = b.timed(yard, ["editnear", "edit"])
            ym = y["editnear"]["median"] + y["edit"]["median"]
            e["yardstick_ms"] = {"editnear": y["editnear"], "edit": y["edit"], "sum_of_medians": ym}
            e["ratio_yardstick_over_dispatcher"] = ym / e["dispatcher_ms"]["median"]
            e["ratio_route2_over_route1"] = e["route2_ms"]["median"] / e["route1_ms"]["median"]
            fast = min((e["route1_ms"], e["route2_ms"]), key=lambda s: s["median"])
            e["dispatcher_ok"] = e["dispatcher_ms"]["median"] <= fast["median"] + (fast["max"] - fast["min"])
            res["shapes"][f"{name}_T{T}"] = e
            print(f"[edit_dedup_time] {name} T {T}: dispatcher {e['dispatcher_ms']['median']:.2f} ms, route 1 {e['route1_ms']['median']:.2f}, route 2 "
                  f"{e['route2_ms']['median']:.2f}, yardstick {ym:.2f} ms, {e['clusters']} clusters, resolve {e['resolve_share']:.2f}, list {e['list_share']:.2f}, "
                  f"ok {e['dispatcher_ok']}", flush=True)
            save()
        ss.close()
    save()


if __name__ == "__main__":
    main()
