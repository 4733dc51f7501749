#!/usr/bin/env python3
"""What neighbours within a bound on the edit distance cost (GPU box):
python tools/edit_within_time.py [--out profiles/edit_within_time.json] [--reps 20] [--budget 20]

One process, device-resident entry points, HIP events (the library's "editnear", "edit" and "knn" brackets), medians of `--reps` launches
after one warm-up; a launch whose warm-up shows that they would take more than `--budget` seconds gets fewer (at least 3; "n" says how
many).  The shapes are those of tools/edit_time.py, drawn as mutated families so that the lists are not empty:

  reads150     10 000 records x 150 DNA symbols        T = 3, 15, 31
  genes1500     2 000 x 1 500 DNA                       T = 31
  ragged        3 000 records, lengths log-uniform 50 .. 5 000, DNA     T = 15  (the length filter)

Per shape and bound, all rows x all columns:
  band_ms        d2g_edit_near_dev with the band route forced (D2G_EDIT_NEAR_ROUTE=1): edit_near_kernel                       ["editnear"]
  yardstick_ms   what gave these lists before: d2g_edit_rect_dev over rows x ALL columns ["edit"], then the clamp ["editnear" of the
                 forced full route: the same kernel over the same rows x N words]
  full_ms        the full route as the dispatcher runs it (D2G_EDIT_NEAR_ROUTE=2): the pair kernel over the window of columns the
                 lengths leave, then the clamp
  ratio          yardstick_ms / band_ms
  select_ms      d2g_edit_within_dev's selection launches of all rows (K = 0, 256 slots per row, lists written)              ["knn"]
  nnz, list_bytes = 8 nnz + 4 N (ids, closeness, row counts) against matrix_bytes = 4 N^2
The band's output is compared with the full route's, word for word, before anything is timed.

"rate": 10 000 x 150 of ONE letter at T = 31: every distance is 0, no lane leaves early, so the lane-steps are counted exactly; against
the VALU bound of DESIGN.md section 3 K2i (VALU_PER_LANE_STEP instructions, CYCLES_PER_VALU cycles each, 4 SIMDs per CU, 64 lanes).  A
SIMD retires a wave64 VALU instruction every 2 cycles when several waves feed it; 4 cycles is what ONE wave's stream can issue, and the
figure at 4 cycles ("one_wave_issue_lane_steps_per_s", K2h's convention) is kept beside the bound only for comparison: this kernel
runs 7 waves per SIMD and exceeds it.
"crossover": 10 000 reads of 8, 16, 32, 33 and 64 symbols at T = 3 .. 7 (up to 32 symbols), 15 and 31, band against full, and what the dispatcher picks: K2h's
kernel (32-bit words, one lane per 32 rows, so one lane per pair up to 32 symbols) is ahead on queries of one block once the bound is
too wide for the early exit: EDIT_NEAR_FULL_MAX_LEN, EDIT_NEAR_SHORT_T_FACTOR and EDIT_NEAR_TINY_LEN of d2g_edit_near.hip come from here.
Nothing here asserts a threshold."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALU_PER_LANE_STEP = 47          # read from the ISA listing of the inner loop (profiles/edit_within_resource_usage.txt): all issued on every step
CYCLES_PER_VALU = 2              # a SIMD's throughput of wave64 VALU instructions with more than one wave resident (one wave alone issues one per 4)
CLOCK_HZ = 2.4e9
SELECT_CAP = 256                 # slots per row of the timed d2g_edit_within_dev (the lists are written, not only counted)


def stats(x):
    x = np.asarray(x, np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


def family(rng, n, lens, letters, per_ancestor, edits):
    """records i of one ancestor: a prefix of it with `edits` substitutions"""
    alphabet = np.frombuffer(letters, np.uint8)
    top = int(max(lens))
    nanc = max(1, n // per_ancestor)
    anc = [rng.choice(alphabet, top) for _ in range(nanc)]
    recs = []
    for i in range(n):
        x = anc[i % nanc][:int(lens[i])].copy()
        pos = rng.integers(0, x.size, edits)
        x[pos] = rng.choice(alphabet, pos.size)
        recs.append(x.tobytes())
    return recs


def shapes(rng):
    yield "reads150", family(rng, 10000, np.full(10000, 150), b"ACGT", 10, 1), [3, 15, 31]
    yield "genes1500", family(rng, 2000, np.full(2000, 1500), b"ACGT", 10, 8), [31]
    yield "ragged", family(rng, 3000, np.exp(rng.uniform(np.log(50), np.log(5000), 3000)).astype(np.int64), b"ACGT", 3000, 2), [15]


class Bench:
    def __init__(self, a):
        import torch
        import dashing2_amd as D
        self.torch, self.D, self.a = torch, D, a
        self.ctx = D.Context(0)
        self.ctx.set_timing(D.TIME_EDIT | D.TIME_EDIT_NEAR | D.TIME_KNN)

    def route(self, r):
        os.environ["D2G_EDIT_NEAR_ROUTE"] = str(r)
        self.ctx.reload_tuning()

    def timed(self, launch, names):
        """median per name over the launches: every name's brackets of one launch are summed"""
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
        reps = int(max(3, min(self.a.reps, self.a.budget / max(sum(first.values()) * 1e-3, 1e-6))))
        runs = [once() for _ in range(reps)]
        return {n: stats([r[n] for r in runs]) for n in names}

    def near(self, ss, T, route, out):
        self.route(route)
        return self.timed(lambda: ss.near_dev(T, out.data_ptr()), ["editnear", "edit"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_within_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=float, default=20.0, help="seconds of launches per measurement")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    b = Bench(a)
    torch, ctx = b.torch, b.ctx
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    bound = ncu * 4 * CLOCK_HZ / (VALU_PER_LANE_STEP * CYCLES_PER_VALU) * 64
    res = {"device": torch.cuda.get_device_name(0), "cus": ncu, "valu_per_lane_step": VALU_PER_LANE_STEP, "cycles_per_valu": CYCLES_PER_VALU,
           "clock_hz": CLOCK_HZ, "valu_bound_lane_steps_per_s": bound, "one_wave_issue_lane_steps_per_s": ncu * 4 * CLOCK_HZ / (VALU_PER_LANE_STEP * 4) * 64,
           "band_max": b.D.EDIT_BAND_MAX, "shapes": {}, "crossover": {}}

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    rng = np.random.default_rng(7600)
    for name, recs, bounds in shapes(rng):
        if a.only and name not in a.only.split(","):
            continue
        N = len(recs)
        lens = np.array([len(r) for r in recs], np.float64)
        ss = ctx.seqset(recs)
        out = torch.zeros(N * N, dtype=torch.int32, device="cuda")
        ref = torch.zeros(N * N, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
        for T in bounds:
            band = b.near(ss, T, 1, out)
            full = b.near(ss, T, 2, ref)
            equal = bool(torch.equal(out, ref))
            b.route(0)
            rect = b.timed(lambda: ss.edit_rect_dev(0, N, 0, N, ref.data_ptr()), ["edit"])
            ids = torch.zeros(N * SELECT_CAP, dtype=torch.int32, device="cuda")
            cls = torch.zeros(N * SELECT_CAP, dtype=torch.int32, device="cuda")
            sel = b.timed(lambda: ss.within_dev(cnt.data_ptr(), ids.data_ptr(), cls.data_ptr(), SELECT_CAP, K=0, T=T), ["knn", "editnear", "edit"])
            nnz = int(cnt.to(torch.int64).sum().item())
            widest = int(cnt.max().item())
            c = out.view(N, N)
            steps = float(N * lens.sum())                                    # lane-steps without the filter and the early exit: one per column symbol and pair
            passed = int((c > 0).sum().item())
            band_ms = band["editnear"]["median"]
            yard_ms = rect["edit"]["median"] + full["editnear"]["median"]
            key = f"{name}_T{T}"
            res["shapes"][key] = {
                "records": N, "mean_length": float(lens.mean()), "max_length": int(lens.max()), "T": T, "band_equals_full": equal,
                "band_ms": band["editnear"], "full_ms": {"pair_kernel_over_window": full["edit"], "clamp": full["editnear"]},
                "yardstick_ms": {"rect_all_columns": rect["edit"], "clamp": full["editnear"], "sum_of_medians": yard_ms},
                "ratio_yardstick_over_band": yard_ms / band_ms, "ratio_full_over_band": (full["edit"]["median"] + full["editnear"]["median"]) / band_ms,
                "select_ms": sel["knn"], "select_cap": SELECT_CAP, "widest_row": widest, "within_dev_ms": {k: v for k, v in sel.items()},
                "nnz": nnz, "pairs_inside_bound_with_self": passed, "list_bytes": 8 * nnz + 4 * N, "matrix_bytes": 4 * N * N,
                "lane_steps_unfiltered": steps, "unfiltered_lane_steps_per_s": steps / (band_ms * 1e-3),
                "fraction_of_valu_bound_if_no_lane_left_early": steps / (band_ms * 1e-3) / bound,
            }
            print(f"[edit_within_time] {key}: band {band_ms:.2f} ms, yardstick {yard_ms:.2f} ms (x{yard_ms / band_ms:.1f}), select {sel['knn']['median']:.2f} ms, "
                  f"nnz {nnz}, equal {equal}", flush=True)
            save()
        ss.close()
        del out, ref, cnt
    if not a.only or "rate" in a.only.split(","):
        # one letter: every distance is 0, no lane leaves early, every lane-step of the count is executed
        N, L, T = 10000, 150, 31
        ss = ctx.seqset([b"A" * L] * N)
        out = torch.zeros(N * N, dtype=torch.int32, device="cuda")
        band = b.near(ss, T, 1, out)
        steps = float(N) * N * L
        ms = band["editnear"]["median"]
        res["rate"] = {"what": "10 000 x 150 of one letter at T = 31: no early exit", "band_ms": band["editnear"], "lane_steps": steps,
                       "lane_steps_per_s": steps / (ms * 1e-3), "fraction_of_valu_bound": steps / (ms * 1e-3) / bound}
        print(f"[edit_within_time] rate: {ms:.2f} ms, {steps / (ms * 1e-3):.3e} lane-steps/s = {steps / (ms * 1e-3) / bound:.3f} of the bound", flush=True)
        save()
        ss.close()
        del out
    if not a.only or "crossover" in a.only.split(","):
        N = 10000
        for L in (8, 16, 32, 33, 64):
            recs = family(rng, N, np.full(N, L), b"ACGT", 10, 1)
            ss = ctx.seqset(recs)
            out = torch.zeros(N * N, dtype=torch.int32, device="cuda")
            for T in ((3, 4, 5, 6, 7, 15, 31) if L <= 32 else (3, 7, 15, 31)):
                band = b.near(ss, T, 1, out)
                full = b.near(ss, T, 2, out)
                auto = b.near(ss, T, 0, out)
                fm = full["edit"]["median"] + full["editnear"]["median"]
                am = auto["edit"]["median"] + auto["editnear"]["median"]
                res["crossover"][f"len{L}_T{T}"] = {"band_ms": band["editnear"], "full_ms": {"pair_kernel": full["edit"], "clamp": full["editnear"], "sum_of_medians": fm},
                                                     "ratio_full_over_band": fm / band["editnear"]["median"], "dispatcher_ms": am,
                                                     "dispatcher_route": "full" if auto["edit"]["median"] > 0 else "band",
                                                     "dispatcher_over_faster_route": am / min(fm, band["editnear"]["median"])}
                print(f"[edit_within_time] crossover len {L} T {T}: band {band['editnear']['median']:.2f} ms, full {fm:.2f} ms, dispatcher {am:.2f} ms", flush=True)
                save()
            ss.close()
            del out
    b.route(0)
    print(json.dumps({k: {"band_ms": v["band_ms"]["median"], "yardstick_ms": v["yardstick_ms"]["sum_of_medians"], "ratio": v["ratio_yardstick_over_band"],
                          "select_ms": v["select_ms"]["median"], "nnz": v["nnz"]} for k, v in res["shapes"].items()}))


if __name__ == "__main__":
    main()
