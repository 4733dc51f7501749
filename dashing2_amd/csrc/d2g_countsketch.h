// d2g_countsketch.h -- the host arithmetic of K3k (--multiset -c <cells>, d2g_k3_countsketch.hip) and of the list stage (d2g_k3_lists.hip): the exact remainder by a run-time divisor,
// the groups of genomes whose table rows fit a byte budget, and the workgroup tables of BagMinHash over (id, weight) lists.  No HIP header
// and no d2g_ctx in here, so that what the kernels trust runs under the host sanitizers (selftest/countsketch_selftest.cpp) as it runs
// in libd2g.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define D2G_CS_HD __host__ __device__
#else
#define D2G_CS_HD
#endif

constexpr uint64_t D2G_CS_MAX_CELLS = 1ull << 31;     // a cell number is the id BagMinHash sees and fits the walkers' 32-bit cell index
constexpr uint64_t D2G_CS_MAX_KMERS = 1ull << 31;     // k-mers of one input: a cell is an int32 and may take them all with one sign
constexpr uint32_t D2G_CS_LDS_MAX = 40960;            // cells of the 160 KiB of LDS of one workgroup (the upper bound of the LDS form)
constexpr uint32_t D2G_WS_CHUNK = 2048;               // elements of an (id, weight) list that one workgroup of k3_bmh_sets_kernel walks

D2G_CS_HD inline uint64_t d2g_cs_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
D2G_CS_HD inline bool d2g_cs_pow2(uint64_t cells) { return (cells & (cells - 1)) == 0; }
// floor(2^64 / cells) for a divisor that is NOT a power of two (2 < cells < 2^64): 2^64 is then no multiple of it, so
// floor((2^64 - 1) / cells) is the same number.  Not used for a power of two (a mask).
inline uint64_t d2g_cs_recip(uint64_t cells) { return ~0ull / cells; }
// hv % cells, exactly (Schismatic<uint64_t>::mod, src/counter.h:75).  With M = floor(2^64 / cells) > 2^64 / cells - 1:
// hv M / 2^64 lies in (hv / cells - 1, hv / cells], so q = floor(hv M / 2^64) is the quotient or one below it and
// hv - q cells lies in [0, 2 cells): ONE conditional subtraction ends it.  Nothing wraps: q cells <= hv.
D2G_CS_HD inline uint64_t d2g_cs_mod(uint64_t hv, uint64_t cells, uint64_t recip) {
    if (d2g_cs_pow2(cells)) return hv & (cells - 1);
    const uint64_t q = d2g_cs_mulhi(hv, recip);
    uint64_t r = hv - q * cells;
    if (r >= cells) r -= cells;
    return r;
}

// A genome takes a table row of `cells` int32 when it owns a workgroup of the launch plan (gblk[g + 1] > gblk[g]); one without k-mers
// takes none.  The batch goes in groups of consecutive genomes whose rows fit `budget_bytes` -- a group always takes its first row,
// fitting or not (the caller has refused a single row that cannot be allocated).  -> the group boundaries, [0, ..., n]; `row` [n]: the
// row of genome g inside its group, ~0 for a genome without one.
inline std::vector<size_t> d2g_cs_groups(const uint32_t *gblk, size_t n, uint64_t cells, uint64_t budget_bytes, std::vector<uint32_t> &row) {
    const uint64_t fit = budget_bytes / (cells * sizeof(int32_t)), per = fit ? fit : 1;      // rows of one group
    std::vector<size_t> cut{0};
    row.assign(n, ~0u);
    uint64_t rows = 0;
    for (size_t g = 0; g < n; ++g) {
        if (gblk[g + 1] == gblk[g]) continue;
        if (rows >= per) { cut.push_back(g); rows = 0; }
        row[g] = (uint32_t)rows++;
    }
    if (n) cut.push_back(n);
    return cut;
}

// the workgroup tables of k3_bmh_sets_kernel over sets given by set_off [nsets + 1]: D2G_WS_CHUNK elements of one set per workgroup
struct d2g_ws_blocks {
    std::vector<uint32_t> set, cnt;     // per workgroup: its set, its elements
    std::vector<uint64_t> lo;           // ... and its first element
};
inline void d2g_ws_plan_blocks(const uint64_t *set_off, size_t nsets, d2g_ws_blocks &b) {
    b.set.clear(); b.cnt.clear(); b.lo.clear();
    for (size_t i = 0; i < nsets; ++i)
        for (uint64_t e = set_off[i]; e < set_off[i + 1]; e += D2G_WS_CHUNK) {
            const uint64_t left = set_off[i + 1] - e;
            b.set.push_back((uint32_t)i); b.lo.push_back(e); b.cnt.push_back((uint32_t)(left < D2G_WS_CHUNK ? left : D2G_WS_CHUNK));
        }
}
// the compacted lists of a group come back per ROW; a genome without a row has an empty list where the next one begins
inline void d2g_cs_expand_set_off(const uint32_t *row, size_t g0, size_t g1, const uint64_t *row_off, const uint64_t *row_total,
                                  uint64_t *set_off, uint64_t *total) {
    uint64_t at = 0;
    for (size_t g = g0; g < g1; ++g) {
        set_off[g - g0] = at;
        total[g - g0] = 0;
        if (row[g] != ~0u) { at = row_off[row[g] + 1]; total[g - g0] = row_total[row[g]]; }
    }
    set_off[g1 - g0] = at;
}
