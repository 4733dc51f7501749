// countsketch_selftest.cpp -- the host arithmetic of the count-sketch chain (K3k, d2g_countsketch.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make sanitize` in dashing2_amd/csrc).  No GPU, no HIP.  Exit code 0 = no finding.
//   1. d2g_cs_mod against `%`: powers of two, odd divisors, the largest divisors, hashes at both ends of the range and next to
//      multiples of the divisor (where a quotient one too small shows)
//   2. d2g_cs_groups: rows only for genomes that own a workgroup, groups cut by the byte budget, a budget below one row
//   3. d2g_ws_plan_blocks and d2g_cs_expand_set_off: every element in exactly one workgroup of its set; empty sets and genomes
//      without a row
#include "../d2g_countsketch.h"
#include <cstdio>
#include <random>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "countsketch selftest failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static int check_mod() {
    const uint64_t divisors[] = {1, 2, 3, 5, 7, 64, 1000, 1024, 8191, 8192, 8193, 65535, 65537, (1ull << 20) + 1, 1000000007ull,
                                 (1ull << 31) - 1, 1ull << 31, (1ull << 31) - 19, 3ull << 29, (1ull << 30) + 1};
    std::mt19937_64 rng(20);
    for (uint64_t c : divisors) {
        REQUIRE(c >= 1 && c <= D2G_CS_MAX_CELLS);
        const uint64_t m = d2g_cs_recip(c);
        if (!d2g_cs_pow2(c)) REQUIRE((unsigned __int128)m * c <= ((unsigned __int128)1 << 64) && (unsigned __int128)(m + 1) * c > ((unsigned __int128)1 << 64));
        std::vector<uint64_t> hv = {0, 1, c - 1, c, c + 1, ~0ull, ~0ull - 1, ~0ull - c, 1ull << 63, (1ull << 63) - 1, (~0ull / c) * c, (~0ull / c) * c - 1};
        for (int i = 0; i < 20000; ++i) {
            const uint64_t r = rng();
            hv.push_back(r);
            const uint64_t q = r / c;
            hv.push_back(q * c); hv.push_back(q * c + (c - 1));             // first and last hash of a quotient
        }
        for (uint64_t h : hv) REQUIRE(d2g_cs_mod(h, c, m) == h % c);
    }
    REQUIRE(d2g_cs_mulhi(~0ull, ~0ull) == ~0ull - 1 && d2g_cs_mulhi(1ull << 32, 1ull << 32) == 1 && d2g_cs_mulhi(5, 7) == 0);
    return 0;
}

static int check_groups() {
    // genomes 0, 1, 3 own workgroups; genome 2 has no k-mers
    const uint32_t gblk[5] = {0, 1, 3, 3, 7};
    std::vector<uint32_t> row;
    const uint64_t cells = 1000, rb = cells * 4;
    std::vector<size_t> cut = d2g_cs_groups(gblk, 4, cells, 100 * rb, row);
    REQUIRE((cut == std::vector<size_t>{0, 4}) && (row == std::vector<uint32_t>{0, 1, ~0u, 2}));
    cut = d2g_cs_groups(gblk, 4, cells, rb, row);                           // one row at a time: the rowless genome rides with its neighbour
    REQUIRE((cut == std::vector<size_t>{0, 1, 3, 4}) && (row == std::vector<uint32_t>{0, 0, ~0u, 0}));
    cut = d2g_cs_groups(gblk, 4, cells, 2 * rb + 5, row);
    REQUIRE((cut == std::vector<size_t>{0, 3, 4}) && (row == std::vector<uint32_t>{0, 1, ~0u, 0}));
    cut = d2g_cs_groups(gblk, 4, cells, 1, row);                            // a budget below one row still takes one
    REQUIRE((cut == std::vector<size_t>{0, 1, 3, 4}));
    const uint32_t none[4] = {0, 0, 0, 0};
    cut = d2g_cs_groups(none, 3, cells, rb, row);
    REQUIRE((cut == std::vector<size_t>{0, 3}) && (row == std::vector<uint32_t>{~0u, ~0u, ~0u}));
    cut = d2g_cs_groups(none, 0, cells, rb, row);
    REQUIRE(cut == std::vector<size_t>{0} && row.empty());
    // every genome with a workgroup gets a row below the group's row count, groups are consecutive and cover [0, n)
    std::mt19937_64 rng(21);
    for (int it = 0; it < 200; ++it) {
        const size_t n = 1 + rng() % 40;
        std::vector<uint32_t> gb(n + 1, 0);
        for (size_t g = 0; g < n; ++g) gb[g + 1] = gb[g] + (uint32_t)(rng() % 3);
        const uint64_t per = 1 + rng() % 5;
        cut = d2g_cs_groups(gb.data(), n, cells, per * rb, row);
        REQUIRE(cut.front() == 0 && cut.back() == n && row.size() == n);
        for (size_t j = 0; j + 1 < cut.size(); ++j) {
            REQUIRE(cut[j] < cut[j + 1]);
            uint32_t next = 0;
            for (size_t g = cut[j]; g < cut[j + 1]; ++g) {
                if (gb[g + 1] == gb[g]) REQUIRE(row[g] == ~0u);
                else REQUIRE(row[g] == next++);
            }
            REQUIRE(next <= per);
        }
    }
    return 0;
}

static int check_blocks() {
    const uint64_t C = D2G_WS_CHUNK;
    const std::vector<uint64_t> off = {0, 0, 1, 1 + C, 1 + C, 2 + 3 * C, 2 + 3 * C + (C - 1)};
    d2g_ws_blocks b;
    d2g_ws_plan_blocks(off.data(), off.size() - 1, b);
    REQUIRE(b.set.size() == b.lo.size() && b.set.size() == b.cnt.size());
    std::vector<int> seen(off.back(), 0);
    for (size_t i = 0; i < b.set.size(); ++i) {
        REQUIRE(b.cnt[i] >= 1 && b.cnt[i] <= C && b.lo[i] >= off[b.set[i]] && b.lo[i] + b.cnt[i] <= off[b.set[i] + 1]);
        for (uint64_t e = b.lo[i]; e < b.lo[i] + b.cnt[i]; ++e) ++seen[e];
    }
    for (int s : seen) REQUIRE(s == 1);
    REQUIRE(b.set.size() == 0 + 1 + 1 + 0 + 3 + 1);
    d2g_ws_plan_blocks(off.data(), 0, b);
    REQUIRE(b.set.empty());
    // rows back to genomes: genomes 4 .. 8 of a batch, rows for 4, 6, 7
    const std::vector<uint32_t> row = {9, 9, 9, 9, 0, ~0u, 1, 2, ~0u};
    const uint64_t row_off[4] = {0, 5, 5, 12}, row_total[3] = {50, 0, 70};
    uint64_t so[6], tot[5];
    d2g_cs_expand_set_off(row.data(), 4, 9, row_off, row_total, so, tot);
    const uint64_t want_so[6] = {0, 5, 5, 5, 12, 12}, want_tot[5] = {50, 0, 0, 70, 0};
    for (int i = 0; i < 6; ++i) REQUIRE(so[i] == want_so[i]);
    for (int i = 0; i < 5; ++i) REQUIRE(tot[i] == want_tot[i]);
    return 0;
}

int main() {
    if (check_mod() || check_groups() || check_blocks()) return 1;
    std::printf("countsketch selftest OK\n");
    return 0;
}
