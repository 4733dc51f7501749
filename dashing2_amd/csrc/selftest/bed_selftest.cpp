// bed_selftest.cpp -- the host side of interval inputs (d2g_intervals.cpp) under ASan + UBSan, no GPU:
//   1. d2g_xxh3_64 against the recorded digests of tests/golden/xxh3_names.json (argv[1]): every length 0 .. 240, the usual names
//   2. d2g_bed_parse on hand-made lines: the reference's rules (bedsketch.cpp:36-46) case by case, and its three refusals
//   3. d2g_interval_plan_build: every position of every line in exactly one chunk of one workgroup of its file; the refusals
//   4. d2g_interval_sweep against a map filled line by line, bit for bit, with and without --normalize-intervals
//   5. d2g_interval_group, the cut of --multiset's files into groups under a budget of covered positions: budgets around one file,
//      files that cover nothing at every place of a group, the file no group can hold
#include "../d2g_intervals.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <random>
#include <string>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "bed selftest failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static int check_golden(const char *path) {
    std::ifstream f(path);
    REQUIRE(bool(f));
    size_t n = 0;
    bool len_seen[241] = {};
    for (std::string l; std::getline(f, l);) {
        const size_t a = l.find("\"hex\": \""), b = l.find("\"xxh3_64\": \"");
        if (a == std::string::npos || b == std::string::npos) continue;
        const size_t a0 = a + 8, a1 = l.find('"', a0), b0 = b + 12;
        REQUIRE(a1 != std::string::npos && (a1 - a0) % 2 == 0);
        std::string name;
        for (size_t i = a0; i < a1; i += 2) name.push_back((char)std::stoi(l.substr(i, 2), nullptr, 16));
        const uint64_t want = std::strtoull(l.c_str() + b0, nullptr, 10);
        REQUIRE(name.size() <= D2G_XXH3_MAX_LEN);
        REQUIRE(d2g_xxh3_64(name.data(), name.size()) == want);
        // the digest must not depend on where the bytes lie: an exact-size heap copy (ASan sees any read past it)
        std::vector<char> copy(name.begin(), name.end());
        REQUIRE(d2g_xxh3_64(copy.data(), copy.size()) == want);
        len_seen[name.size()] = true;
        ++n;
    }
    for (int i = 0; i <= 240; ++i) REQUIRE(len_seen[i]);
    REQUIRE(n >= 241 + 75);
    const std::string longname(241, 'a');
    REQUIRE(d2g_xxh3_64(longname.data(), longname.size()) == 0);
    return 0;
}

struct Parsed { int rc; std::vector<uint64_t> h, a, b; std::string err; };
static Parsed parse(const std::string &buf, int trim = 1) {
    Parsed p;
    size_t n = 0;
    char err[400] = "";
    p.rc = d2g_bed_parse(buf.data(), buf.size(), trim, nullptr, nullptr, nullptr, 0, &n, err, sizeof err);   // count only
    p.err = err;
    if (p.rc) return p;
    p.h.resize(n); p.a.resize(n); p.b.resize(n);
    size_t n2 = 0;
    p.rc = d2g_bed_parse(buf.data(), buf.size(), trim, p.h.data(), p.a.data(), p.b.data(), n, &n2, err, sizeof err);
    if (n2 != n) p.rc = -100;
    return p;
}
static uint64_t H(const char *s) { return d2g_xxh3_64(s, std::strlen(s)); }

static int check_parse() {
    Parsed p = parse("#track\n\nchr1\t5\t10\nchr1\t7\t12\n");
    REQUIRE(p.rc == D2G_OK && p.h.size() == 2 && p.h[0] == H("1") && p.h[1] == H("1") && p.a[0] == 5 && p.b[0] == 10 && p.a[1] == 7 && p.b[1] == 12);
    p = parse("chr1\t5\t10");                                            // no line feed at the end
    REQUIRE(p.rc == D2G_OK && p.h.size() == 1 && p.b[0] == 10);
    p = parse("chr1\t5\t10\r\nchr2\t1\t2\r\n");                          // CRLF: the CR ends strtoul's digits
    REQUIRE(p.rc == D2G_OK && p.h.size() == 2 && p.b[0] == 10 && p.h[1] == H("2") && p.b[1] == 2);
    p = parse("\r\n");                                                   // a line that holds only a CR is not empty and has no tab
    REQUIRE(p.rc == D2G_ERR_INVALID && p.err == "Malformed line: \r");
    p = parse("chr1\t5\n");                                              // a missing stop reads 0: nothing is covered
    REQUIRE(p.rc == D2G_OK && p.a[0] == 5 && p.b[0] == 0);
    p = parse("chr1\t\n");                                               // both missing
    REQUIRE(p.rc == D2G_OK && p.a[0] == 0 && p.b[0] == 0);
    p = parse("chr1\t  5 \t 10\textra\t+\n");                            // leading blanks, further columns
    REQUIRE(p.rc == D2G_OK && p.a[0] == 5 && p.b[0] == 10);
    p = parse("chr1\t+5\t+9\n");
    REQUIRE(p.rc == D2G_OK && p.a[0] == 5 && p.b[0] == 9);
    p = parse("chr1\t-1\t3\n");                                          // strtoul negates modulo 2^64
    REQUIRE(p.rc == D2G_OK && p.a[0] == ~0ull && p.b[0] == 3);
    p = parse("chr1\tx5\t9\n");                                          // no digits: 0, and the second call starts at the same place
    REQUIRE(p.rc == D2G_OK && p.a[0] == 0 && p.b[0] == 0);
    p = parse("Chr1\t1\t2\nCHR1\t1\t2\nch1\t1\t2\nchr\t1\t2\n\t1\t2\nchrchr1\t1\t2\n");
    REQUIRE(p.rc == D2G_OK && p.h.size() == 6);
    REQUIRE(p.h[0] == H("1") && p.h[1] == H("CHR1") && p.h[2] == H("ch1") && p.h[3] == H("") && p.h[4] == H("") && p.h[5] == H("chr1"));
    p = parse("chr1\t1\t2\nChr1\t1\t2\n", 0);                            // trim_chr off
    REQUIRE(p.rc == D2G_OK && p.h[0] == H("chr1") && p.h[1] == H("Chr1"));
    p = parse("chr1\t10\t5\n");                                          // start > stop: parsed as it stands
    REQUIRE(p.rc == D2G_OK && p.a[0] == 10 && p.b[0] == 5);
    p = parse("chr1\t4294967295\t4294967297\nchr1\t18446744073709551615\t18446744073709551616\n");   // at and above 2^32; saturation
    REQUIRE(p.rc == D2G_OK && p.a[0] == 4294967295ull && p.b[0] == 4294967297ull && p.a[1] == ~0ull && p.b[1] == ~0ull);
    p = parse("chr1 5 10\n");
    REQUIRE(p.rc == D2G_ERR_INVALID && p.err == "Malformed line: chr1 5 10");
    p = parse("chr1\t1\t2\nbad\n");
    REQUIRE(p.rc == D2G_ERR_INVALID && p.err == "Malformed line: bad");
    p = parse(std::string("\x1f\x8b\x08\x00", 4) + "abc\t1\t2\n");
    REQUIRE(p.rc == D2G_ERR_INVALID && p.err.find("gzip") != std::string::npos);
    p = parse("chr" + std::string(240, 'q') + "\t1\t2\n");               // 240 bytes after the trim: hashed
    REQUIRE(p.rc == D2G_OK && p.h[0] == d2g_xxh3_64(std::string(240, 'q').data(), 240));
    p = parse(std::string(241, 'q') + "\t1\t2\n");
    REQUIRE(p.rc == D2G_ERR_INVALID && p.err.find("241 bytes") != std::string::npos);
    // a smaller capacity than lines: the count is whole, nothing is written past cap
    uint64_t h[2] = {7, 7}, a[2] = {7, 7}, b[2] = {7, 7};
    size_t n = 0;
    REQUIRE(d2g_bed_parse("1\t1\t2\n2\t3\t4\n3\t5\t6\n", 18, 1, h, a, b, 1, &n, nullptr, 0) == D2G_OK && n == 3 && a[0] == 1 && h[1] == 7 && a[1] == 7 && b[1] == 7);
    REQUIRE(d2g_bed_parse(nullptr, 0, 1, nullptr, nullptr, nullptr, 0, &n, nullptr, 0) == D2G_OK && n == 0);
    REQUIRE(d2g_bed_parse("x", 1, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == D2G_ERR_INVALID);
    return 0;
}

static int check_plan_case(const std::vector<uint64_t> &h, const std::vector<uint64_t> &a, const std::vector<uint64_t> &b, const std::vector<uint64_t> &off) {
    const IntervalTables in{h.data(), a.data(), b.data(), h.size(), off.data(), off.size() - 1};
    IntervalPlanHost p;
    std::string err;
    REQUIRE(d2g_interval_plan_build(in, p, err) == D2G_OK);
    const size_t nk = p.hash.size(), nb = p.bf.size();
    REQUIRE(p.chunk_off.size() == nk + 1 && p.start.size() == nk && p.stop.size() == nk && p.file_positions.size() == in.n);
    REQUIRE(p.bc0.size() == nb && p.bn.size() == nb && p.blo.size() == nb && p.bhi.size() == nb);
    // the kernel's walk, on the host: what every workgroup covers, per file
    std::vector<std::map<std::pair<uint64_t, uint64_t>, int>> seen(in.n);
    uint64_t npos = 0;
    for (size_t blk = 0; blk < nb; ++blk) {
        REQUIRE(p.bf[blk] < in.n && p.bn[blk] >= 1 && p.bn[blk] <= (uint32_t)K1_BLOCK_CHUNKS && p.blo[blk] < p.bhi[blk] && p.bhi[blk] <= nk);
        for (uint32_t ci = 0; ci < p.bn[blk]; ++ci) {
            const uint64_t c = p.bc0[blk] + ci;
            uint32_t lo = p.blo[blk], hi = p.bhi[blk];
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (p.chunk_off[mid] <= c) lo = mid; else hi = mid; }
            REQUIRE(p.chunk_off[lo] <= c && c < p.chunk_off[lo + 1]);
            const uint64_t pos = p.start[lo] + (c - p.chunk_off[lo]) * K1_CHUNK;
            REQUIRE(pos < p.stop[lo]);
            const uint64_t left = p.stop[lo] - pos, n = left < (uint64_t)K1_CHUNK ? left : K1_CHUNK;
            for (uint64_t e = 0; e < n; ++e) ++seen[p.bf[blk]][{p.hash[lo], pos + e}];
            npos += n;
        }
    }
    REQUIRE(npos == p.npositions);
    for (size_t f = 0; f < in.n; ++f) {
        std::map<std::pair<uint64_t, uint64_t>, int> want;
        uint64_t fp = 0;
        for (size_t j = off[f]; j < off[f + 1]; ++j) for (uint64_t i = a[j]; i < b[j]; ++i) { ++want[{h[j], i}]; ++fp; }
        REQUIRE(want == seen[f] && fp == p.file_positions[f]);
    }
    return 0;
}

static int check_plan() {
    const uint64_t B = (uint64_t)K1_BLOCK_CHUNKS * K1_CHUNK, big = 1ull << 33;
    if (check_plan_case({}, {}, {}, {0})) return 1;
    if (check_plan_case({}, {}, {}, {0, 0, 0})) return 1;
    if (check_plan_case({1, 1, 2, 1, 1, 3}, {5, 9, 0, 100, 7, big - 3}, {5, 3, 1, 100 + K1_CHUNK + 1, 7 + K1_CHUNK - 1, big + 70}, {0, 2, 2, 6})) return 1;
    for (int d = -1; d <= 1; ++d)                                          // one workgroup's positions, and that +- 1, beside an empty file
        if (check_plan_case({9, 9}, {0, 10}, {B / 2, 10 + B / 2 + d}, {0, 0, 2})) return 1;
    {   // many one-base lines: more lines than a workgroup has chunks
        std::vector<uint64_t> h(3000, 4), a(3000), b(3000);
        for (size_t i = 0; i < 3000; ++i) { a[i] = 2 * i; b[i] = 2 * i + 1; }
        if (check_plan_case(h, a, b, {0, 1000, 3000})) return 1;
    }
    {   // one long line: several workgroups of one line
        if (check_plan_case({4}, {17}, {17 + 3 * B + 5}, {0, 1})) return 1;
    }
    IntervalPlanHost p;
    std::string err;
    const uint64_t h1[2] = {1, 1}, a1[2] = {0, 0}, b1[2] = {1ull << 43, (1ull << 43) + 1}, off1[2] = {0, 2}, offbad[3] = {0, 2, 1}, offshort[2] = {0, 1};
    REQUIRE(d2g_interval_plan_build({h1, a1, b1, 2, off1, 1}, p, err) == D2G_ERR_UNSUPPORTED && err.find("2^44") != std::string::npos);
    p = IntervalPlanHost();
    const uint64_t bneg[2] = {~0ull, 5};                                   // "-1" as a stop
    REQUIRE(d2g_interval_plan_build({h1, a1, bneg, 2, off1, 1}, p, err) == D2G_ERR_UNSUPPORTED);
    p = IntervalPlanHost();
    REQUIRE(d2g_interval_plan_build({h1, a1, b1, 2, offbad, 2}, p, err) == D2G_ERR_INVALID);
    p = IntervalPlanHost();
    REQUIRE(d2g_interval_plan_build({h1, a1, b1, 2, offshort, 1}, p, err) == D2G_ERR_INVALID);
    p = IntervalPlanHost();
    REQUIRE(d2g_interval_plan_build({nullptr, a1, b1, 2, off1, 1}, p, err) == D2G_ERR_INVALID);
    p = IntervalPlanHost();
    REQUIRE(d2g_interval_plan_build({h1, a1, b1, 2, nullptr, 1}, p, err) == D2G_ERR_INVALID);
    return 0;
}

static int check_sweep() {
    std::mt19937_64 rng(20);
    for (int rep = 0; rep < 200; ++rep) {
        const bool normalize = rep & 1;
        const size_t nl = rep < 4 ? rep : 1 + rng() % 12;
        std::vector<uint64_t> h(nl), a(nl), b(nl);
        for (size_t j = 0; j < nl; ++j) {
            h[j] = 1 + rng() % 3;
            a[j] = (rep % 5 == 0 ? (1ull << 32) - 8 : 0) + rng() % 24;
            const uint64_t len = rng() % 4 == 0 ? 0 : (rng() % 3 == 0 ? 7 : rng() % 2 ? 3 : 1 + rng() % 9);
            b[j] = rng() % 16 == 0 ? a[j] - std::min<uint64_t>(a[j], 2) : a[j] + len;
        }
        if (nl >= 2 && rep % 3 == 0) { h[1] = h[0]; a[1] = a[0]; b[1] = b[0]; }     // a duplicate line
        const uint64_t off[2] = {0, nl};
        const IntervalTables in{h.data(), a.data(), b.data(), nl, off, 1};
        std::map<std::pair<uint64_t, uint64_t>, double> want;                      // the reference's `ctr.add(chrhash ^ i, inc)`, keyed by the pair
        for (size_t j = 0; j < nl; ++j) {
            const double inc = normalize ? 1. / (double)(b[j] - a[j]) : 1.;
            for (uint64_t i = a[j]; i < b[j]; ++i) want[{h[j], i}] += inc;
        }
        std::vector<uint64_t> rh, rlo, rhi;
        std::vector<double> rw;
        d2g_interval_sweep(in, 0, nl, normalize, rh, rlo, rhi, rw);
        std::map<std::pair<uint64_t, uint64_t>, double> got;
        for (size_t r = 0; r < rh.size(); ++r) {
            REQUIRE(rlo[r] < rhi[r] && rw[r] > 0.);
            if (r) {
                REQUIRE(rh[r - 1] < rh[r] || (rh[r - 1] == rh[r] && rhi[r - 1] <= rlo[r]));                    // ascending, disjoint
                REQUIRE(!(rh[r - 1] == rh[r] && rhi[r - 1] == rlo[r] && std::memcmp(&rw[r - 1], &rw[r], 8) == 0));   // maximal
            }
            for (uint64_t i = rlo[r]; i < rhi[r]; ++i) { REQUIRE(!got.count({rh[r], i})); got[{rh[r], i}] = rw[r]; }
        }
        REQUIRE(got.size() == want.size());
        for (const auto &kv : want) {
            const auto it = got.find(kv.first);
            REQUIRE(it != got.end() && std::memcmp(&it->second, &kv.second, 8) == 0);                          // bit for bit
        }
    }
    return 0;
}

// the groups of files that cover `cov` positions each under `budget`, cut as d2g_interval_bmh_sketch cuts them: -> 0, and the
// boundaries [0, ..., n] in `cut`; -> 1 + f where file f alone is over the budget (cut: the groups before it).  Every file must be
// asked about once per group that looks at it, in order, and the last one asked is the one that ends the group.
static size_t groups(const std::vector<uint64_t> &cov, uint64_t budget, std::vector<size_t> &cut, bool *order_ok) {
    cut.assign(1, 0);
    *order_ok = true;
    for (size_t f0 = 0; f0 < cov.size();) {
        size_t next = f0;
        const size_t f1 = d2g_interval_group(f0, cov.size(), budget, [&](size_t f) { *order_ok = *order_ok && f == next; ++next; return cov[f]; });
        *order_ok = *order_ok && f1 <= cov.size() && next == std::min(f1 + 1, cov.size());
        if (f1 == f0) return 1 + f0;
        cut.push_back(f1);
        f0 = f1;
    }
    return 0;
}

static int check_groups() {
    using V = std::vector<size_t>;
    std::vector<size_t> cut;
    bool ok = false;
    const std::vector<uint64_t> three{5, 7, 5};
    REQUIRE(groups(three, 17, cut, &ok) == 0 && ok && cut == V({0, 3}));                   // everything fits: one group
    REQUIRE(groups(three, 16, cut, &ok) == 0 && ok && cut == V({0, 2, 3}));
    REQUIRE(groups(three, 12, cut, &ok) == 0 && ok && cut == V({0, 2, 3}));                // exactly two files
    REQUIRE(groups(three, 11, cut, &ok) == 0 && ok && cut == V({0, 1, 2, 3}));             // one position short of two
    REQUIRE(groups(three, 7, cut, &ok) == 0 && ok && cut == V({0, 1, 2, 3}));              // exactly the largest file: it passes, alone
    REQUIRE(groups(three, 6, cut, &ok) == 2 && ok && cut == V({0, 1}));                    // one position short of it: file 1 fits no group
    REQUIRE(groups(three, 4, cut, &ok) == 1 && ok && cut == V({0}));                       // below every file
    REQUIRE(groups(three, 0, cut, &ok) == 1 && ok);
    REQUIRE(groups({}, 5, cut, &ok) == 0 && ok && cut == V({0}));
    // files that cover nothing: first, last, on both sides of a border; they never open a group of their own behind a full one
    const std::vector<uint64_t> holes{0, 4, 0, 0, 4, 0};
    REQUIRE(groups(holes, 8, cut, &ok) == 0 && ok && cut == V({0, 6}));
    REQUIRE(groups(holes, 4, cut, &ok) == 0 && ok && cut == V({0, 4, 6}));                 // the empty files at the border ride with the group in front
    REQUIRE(groups(holes, 7, cut, &ok) == 0 && ok && cut == V({0, 4, 6}));
    REQUIRE(groups(holes, 3, cut, &ok) == 2 && ok && cut == V({0, 1}));                    // the empty first file is a group; the next file fits none
    REQUIRE(groups({0, 0, 0}, 0, cut, &ok) == 0 && ok && cut == V({0, 3}));                // nothing to hold: any budget does
    REQUIRE(groups({0, 9}, 8, cut, &ok) == 2 && ok && cut == V({0, 1}));
    // positions near the top of the range: no wrap-around lets a file in
    const uint64_t big = 1ull << 63;
    REQUIRE(groups({big, big, 1}, ~0ull, cut, &ok) == 0 && ok && cut == V({0, 1, 3}));
    REQUIRE(groups({big, big}, big - 1, cut, &ok) == 1 && ok);
    // random files against the rule stated from the groups' side: a group holds at most the budget, and the file behind it would not fit
    std::mt19937_64 rng(11);
    for (int it = 0; it < 2000; ++it) {
        std::vector<uint64_t> cov(rng() % 12);
        uint64_t most = 0;
        for (auto &c : cov) { c = rng() % 4 ? rng() % 20 : 0; most = std::max(most, c); }
        const uint64_t budget = most + rng() % 25;
        REQUIRE(groups(cov, budget, cut, &ok) == 0 && ok && cut.back() == cov.size());
        for (size_t g = 0; g + 1 < cut.size(); ++g) {
            REQUIRE(cut[g] < cut[g + 1]);
            uint64_t sum = 0;
            for (size_t f = cut[g]; f < cut[g + 1]; ++f) sum += cov[f];
            REQUIRE(sum <= budget && (cut[g + 1] == cov.size() || sum + cov[cut[g + 1]] > budget));
        }
        if (most) {
            const size_t first = std::find(cov.begin(), cov.end(), most) - cov.begin();
            const size_t bad = groups(cov, most - 1, cut, &ok);
            REQUIRE(ok && bad == 1 + first);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: bed_selftest <tests/golden/xxh3_names.json>\n"); return 2; }
    if (check_golden(argv[1]) || check_parse() || check_plan() || check_sweep() || check_groups()) return 1;
    std::printf("bed selftest OK\n");
    return 0;
}
