// d2g_intervals.h -- the host side of interval inputs (BED; K1i, d2g_k1i.hip): the launch plan over interval tables and the sweep
// behind --multiset.  Plain host arithmetic like d2g_plan.h: no HIP header and no d2g_ctx, so it runs under the host sanitizers
// (selftest/bed_selftest.cpp) as it runs in libd2g.
#pragma once
#include "d2g_plan.h"                 // K1_THREADS, K1_CHUNK, K1_BLOCK_CHUNKS: K1i keeps K1's geometry

// n files as the caller's HOST arrays (a view): line j covers positions [start[j], stop[j]) of the chromosome hashed to chrhash[j]
struct IntervalTables {
    const uint64_t *chrhash, *start, *stop;         // [nint]
    size_t nint;
    const uint64_t *file_off;                       // [n + 1] file f owns lines [file_off[f], file_off[f + 1])
    size_t n;
};

// launch plan: the lines that cover something (in line order), chunks of K1_CHUNK positions per line, <= K1_BLOCK_CHUNKS chunks of ONE
// file per workgroup.  The kernel indexes with what this writes and checks nothing.
struct IntervalPlanHost {
    std::vector<uint64_t> hash, start, stop;        // [nkept] the kept lines
    std::vector<uint64_t> chunk_off, bc0;           // [nkept + 1] exclusive prefix of chunks per kept line; per workgroup its first chunk,
    std::vector<uint32_t> bf, bn, blo, bhi;         // its file, its chunks and the kept lines [blo, bhi) that own one of them
    std::vector<uint64_t> file_positions;           // [n]
    uint64_t npositions = 0;
};
int d2g_interval_plan_build(const IntervalTables &in, IntervalPlanHost &p, std::string &err);

// --multiset: the maximal runs of one file's lines [j0, j1), chromosome hashes ascending, positions ascending; the weight of a run is
// 0.0 + inc(j) over its covering lines in ascending j, inc = 1 or 1.0 / (double)(stop - start) -- the sum the reference's map
// holds after `+= inc` line by line.  Adjacent pieces of bit-equal weight are one run.  Appends to the four vectors.
void d2g_interval_sweep(const IntervalTables &in, size_t j0, size_t j1, bool normalize, std::vector<uint64_t> &hash,
                        std::vector<uint64_t> &lo, std::vector<uint64_t> &hi, std::vector<double> &w);

// --multiset on the device (d2g_interval_bmh_sketch): the files' (id, weight) lists go in groups of consecutive files whose covered
// positions fit `budget`.  The greedy cut of one group that starts at file f0 < n: `covered(f)` is asked for f0, f0 + 1, ... in order,
// once each (the caller sweeps the file there), and the first file that would pass the budget ends the group and starts the next one;
// a file that covers nothing always rides along.  -> f1, the group is [f0, f1): the last file asked was f1 where f1 < n, and its runs
// are the caller's to drop.  f1 == f0: file f0 alone is over the budget, which no group can hold.
template <class Covered> size_t d2g_interval_group(size_t f0, size_t n, uint64_t budget, Covered &&covered) {
    uint64_t used = 0;                                      // <= budget; a file covers <= 2^44 positions
    size_t f1 = f0;
    for (; f1 < n; ++f1) {
        const uint64_t c = covered(f1);
        if (c > budget || used > budget - c) break;
        used += c;
    }
    return f1;
}
