"""Times the interval kernels (K1i) and writes profiles/bed_time.json: python tools/bed_time.py [out.json] [--quick]
  kernels   HIP events (D2G_TIME_K1 / D2G_TIME_K3), medians of 20 launches after 3 warm-up launches, all in THIS process:
            K1 ("k1") on 1000 genomes x 5 Mbp (the shape of tools/k1_time.py), K1i ("k1i") on 1000 files x 5 000 000 positions in lines
            of 500, and K1i on lines of ONE position -- one lane per position, the worst case.  The one-position tables cost 32 bytes per
            position on the device, so that leg runs on 8 files x 2 500 000 lines and is compared per position.
  multiset  d2g_interval_bmh_sketch on 100 files x 5 000 000 covered positions (lines of 500, every fifth line covered twice) against
            the --multiset k-mer chain (d2g_bmh_sketch_dev, "k3") on 100 genomes x 5 Mbp: walls and event times, medians of 5.
  e2e       `dashing2 sketch --bed -o` on 200 files x 5 000 000 positions in the page cache, against the reference algorithm restated in
            NumPy on 16 processes, one file per process at a time (tests/bed_ref.py's oph_registers: Wang hash + minimum per position) --
            labelled as such: it is not the reference binary.  Medians of 5 (CLI) and 3 (NumPy, on 32 of the files, scaled per file)."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import dashing2_amd as d2  # noqa: E402

QUICK = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else os.path.join(ROOT, "profiles", "bed_time.json")
S = 1024
med = statistics.median


def launches(ctx, call, which, reps, warm):
    ts = []
    for i in range(warm + reps):
        ctx.kernel_ms(which)
        call()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(ctx.kernel_ms(which)[2])
    return ts


def interval_tables(nfiles, per_file, length, seed=0):
    """nfiles x (per_file / length) disjoint lines of `length` positions on 24 chromosomes"""
    n = per_file // length
    rng = np.random.default_rng(seed)
    h = rng.integers(1, 1 << 63, 24, dtype=np.uint64)
    start = (np.arange(n, dtype=np.uint64) * np.uint64(length + 37))
    hh = np.tile(h[np.arange(n) % 24], nfiles)
    ss = np.tile(start, nfiles) + np.repeat(np.arange(nfiles, dtype=np.uint64) * np.uint64(1000), n)
    return hh, ss, ss + np.uint64(length), np.arange(nfiles + 1, dtype=np.uint64) * np.uint64(n)


def cpu_file(path):
    import bed_ref as R
    h, a, b, _ = R.tables([open(path, "rb").read()])
    return R.oph_registers(list(zip(h.tolist(), a.tolist(), b.tolist())), S)


def main():
    ctx = d2.Context(0)
    ctx.set_timing(True)
    reps, warm = (5, 1) if QUICK else (20, 3)
    res = {"timer": "HIP events, medians of %d launches after %d warm-up launches; host clocks for the walls" % (reps, warm), "sketchsize": S}
    # ---- K1 on the bench's sketch-leg shape
    ng, L = (100, 5_000_000) if QUICK else (1000, 5_000_000)
    stride = ((L + 3) // 4 + 63) // 64 * 64
    packed = torch.randint(0, 256, (ng * stride + 64,), dtype=torch.uint8, device="cuda")
    plan = ctx.oph_plan(np.arange(ng, dtype=np.uint64) * np.uint64(stride * 4), np.full(ng, L, np.uint32), np.arange(ng + 1, dtype=np.uint64), 31)
    regs = torch.empty((ng, d2.oph_m(S)), dtype=torch.int64, device="cuda")
    t1 = launches(ctx, lambda: ctx.oph_sketch_dev(plan, packed.data_ptr(), S, regs.data_ptr()), "k1", reps, warm)
    res["k1"] = {"genomes": ng, "bases_each": L, "k": 31, "ms": med(t1), "ms_min_max": [min(t1), max(t1)], "elements_per_s": ng * (L - 30) / med(t1) * 1e3}
    plan.close()
    del packed
    # ---- K1i, lines of 500 and of 1
    for name, nf, per, length in (("k1i_lines_of_500", ng, 5_000_000, 500), ("k1i_lines_of_1", 2 if QUICK else 8, 2_500_000, 1)):
        p = ctx.interval_plan(*interval_tables(nf, per, length))
        r = torch.empty((nf, d2.oph_m(S)), dtype=torch.int64, device="cuda")
        t = launches(ctx, lambda: ctx.interval_oph_sketch_dev(p, S, r.data_ptr()), "k1i", reps, warm)
        res[name] = {"files": nf, "positions_each": per, "line_length": length, "ms": med(t), "ms_min_max": [min(t), max(t)],
                     "elements_per_s": p.npositions / med(t) * 1e3}
        p.close()
    res["k1i_over_k1_per_element"] = res["k1"]["elements_per_s"] / res["k1i_lines_of_500"]["elements_per_s"]
    res["k1i_lines_of_1_over_lines_of_500_per_element"] = res["k1i_lines_of_500"]["elements_per_s"] / res["k1i_lines_of_1"]["elements_per_s"]
    # ---- the multiset chains
    nf = 10 if QUICK else 100
    h, a, b, off = interval_tables(nf, 5_000_000, 500, seed=1)
    n = int(off[1])
    dup = np.arange(h.size) % 5 == 0                                       # every fifth line once more: depth 2
    order = np.argsort(np.concatenate([np.arange(h.size), np.arange(h.size)[dup]]), kind="stable")
    hh, aa, bb = (np.concatenate([x, x[dup]])[order] for x in (h, a, b))
    off2 = np.arange(nf + 1, dtype=np.uint64) * np.uint64(n + n // 5)
    p = ctx.interval_plan(hh, aa, bb, off2)
    walls, ex, bm = [], [], []
    for i in range(1 + (2 if QUICK else 5)):
        for w in ("k1iexpand", "k1ibmh"):
            ctx.kernel_ms(w)
        t0 = time.perf_counter()
        sig, tw = ctx.interval_bmh_sketch(p, S)
        if i:
            walls.append((time.perf_counter() - t0) * 1e3)
            e, m = ctx.kernel_ms("k1iexpand"), ctx.kernel_ms("k1ibmh")
            ex.append(e[0] * e[1]); bm.append(m[0] * m[1])
    res["multiset_intervals"] = {"files": nf, "covered_positions_each": 5_000_000, "wall_ms": med(walls), "k1iexpand_ms": med(ex), "k1ibmh_ms": med(bm),
                                 "note": "the wall includes the host sweep (one thread) and the waits of the BagMinHash passes"}
    p.close()
    packed = torch.randint(0, 256, (nf * stride + 64,), dtype=torch.uint8, device="cuda")
    plan = ctx.oph_plan(np.arange(nf, dtype=np.uint64) * np.uint64(stride * 4), np.full(nf, L, np.uint32), np.arange(nf + 1, dtype=np.uint64), 31)
    sigd, twd = torch.empty((nf, S), dtype=torch.float64, device="cuda"), torch.empty(nf, dtype=torch.float64, device="cuda")
    walls, k3 = [], []
    for i in range(1 + (2 if QUICK else 5)):
        ctx.kernel_ms("k3")
        t0 = time.perf_counter()
        ctx.bmh_sketch_dev(plan, packed.data_ptr(), S, sigd.data_ptr(), twd.data_ptr())
        torch.cuda.synchronize()
        if i:
            walls.append((time.perf_counter() - t0) * 1e3)
            e = ctx.kernel_ms("k3")
            k3.append(e[0] * e[1])
    res["multiset_kmers"] = {"genomes": nf, "bases_each": L, "k": 31, "wall_ms": med(walls), "k3_ms": med(k3)}
    res["multiset_intervals_over_kmers_wall"] = res["multiset_intervals"]["wall_ms"] / res["multiset_kmers"]["wall_ms"]
    plan.close()
    del packed
    ctx.close()
    # ---- end to end
    nfiles = 20 if QUICK else 200
    exe = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
    with tempfile.TemporaryDirectory() as d:
        h, a, b, off = interval_tables(nfiles, 5_000_000, 500, seed=2)
        names = [b"chr%d" % (c + 1) for c in range(24)]
        paths = []
        for f in range(nfiles):
            lo, hi = int(off[f]), int(off[f + 1])
            path = os.path.join(d, "f%d.bed" % f)
            with open(path, "wb") as fp:
                fp.write(b"".join(b"%s\t%d\t%d\n" % (names[j % 24], int(a[lo + j]), int(b[lo + j])) for j in range(hi - lo)))
            paths.append(path)
        lst = os.path.join(d, "paths.txt")
        open(lst, "w").write("\n".join(paths) + "\n")
        cli = []
        for i in range(1 + (2 if QUICK else 5)):
            t0 = time.perf_counter()
            subprocess.run([exe, "sketch", "--bed", "-S", str(S), "-F", lst, "-o", os.path.join(d, "o.bin")], check=True, capture_output=True)
            if i:
                cli.append(time.perf_counter() - t0)
        import multiprocessing as mp
        sub = paths[:8 if QUICK else 32]
        cpu = []
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(cpu_file, sub[:16])                                     # start the workers, import numpy
            for _ in range(3):
                t0 = time.perf_counter()
                pool.map(cpu_file, sub, chunksize=1)
                cpu.append(time.perf_counter() - t0)
        res["e2e"] = {"files": nfiles, "positions_each": 5_000_000, "bytes_each": os.path.getsize(paths[0]),
                      "cli_sketch_bed_wall_s": med(cli), "cli_files_per_s": nfiles / med(cli),
                      "numpy_16_processes_files": len(sub), "numpy_16_processes_wall_s": med(cpu), "numpy_files_per_s": len(sub) / med(cpu),
                      "cli_over_numpy_files_per_s": (nfiles / med(cli)) / (len(sub) / med(cpu)),
                      "baseline": "the reference algorithm restated in NumPy (tests/bed_ref.py), 16 processes, one file each at a time; not the reference binary"}
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
