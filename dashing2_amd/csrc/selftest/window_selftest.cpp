// window_selftest.cpp -- the host side of the windowed walker (K1w, -w > k) under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make sanitize` in dashing2_amd/csrc).  No GPU, no HIP.  Exit code 0 = no finding.
//   1. the windowed launch plan (d2g_plan.cpp) against a direct count of emissions: every chunk is found, by the walker's own binary
//      search over the block's runs, in the run that owns it; runs shorter than w own none; the cap; w <= k changes nothing
//   2. the register queue of the walker (d2g_minq.h, the code the kernels run) in the walker's own loop -- push, expire, the re-roll
//      when the queue has run dry -- against a brute-force minimum per window
//   3. the .w<w> part of the --set / --countdict file names (host/exact_files.h; fastxmerge.cpp:87-90)
#include "../../../include/d2g.h"
#include "../d2g_minq.h"
#include "../d2g_plan.h"
#include "../../host/exact_files.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "window selftest failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

struct Runs {
    std::vector<uint64_t> rs, go;
    std::vector<uint32_t> rl;
    Runs(std::vector<uint32_t> lens, std::vector<uint64_t> off) : go(std::move(off)), rl(std::move(lens)) {
        uint64_t at = 0;
        for (uint32_t l : rl) { rs.push_back(at); at += l + 1; }          // an N between runs
    }
    PackedRuns view(int k, int w) const { return {nullptr, 0, rs.data(), rl.data(), rl.size(), go.data(), go.size() - 1, k, 1, w}; }
};

static uint64_t direct_emissions(uint32_t len, int k, int w) {           // counted, not computed: the positions whose window fits
    const int span = w > k ? w : k;
    uint64_t e = 0;
    for (uint64_t i = 0; i + span <= len; ++i) ++e;
    return e;
}

static int check_plan(const Runs &t, int k, int w) {
    const PackedRuns in = t.view(k, w);
    PlanHost p;
    std::string err;
    REQUIRE(d2g_plan_build(in, p, err) == D2G_OK && err.empty());
    const size_t nrun = in.nrun, nblk = p.bg.size();
    REQUIRE(p.chunk_off.size() == nrun + 1 && p.chunk_off[0] == 0);
    uint64_t total = 0;
    std::vector<uint64_t> em(nrun);
    for (size_t r = 0; r < nrun; ++r) {
        em[r] = direct_emissions(t.rl[r], k, w);
        REQUIRE(em[r] == d2g_run_emissions(t.rl[r], k, w));
        REQUIRE(p.chunk_off[r + 1] - p.chunk_off[r] == (em[r] + K1_CHUNK - 1) / K1_CHUNK);
        total += em[r];
    }
    REQUIRE(p.nkmers == total);
    size_t b = 0;
    uint64_t walked = 0;
    for (size_t g = 0; g < in.n; ++g) {
        uint64_t c = p.chunk_off[t.go[g]];
        const uint64_t cend = p.chunk_off[t.go[g + 1]];
        for (; c < cend; ++b) {
            REQUIRE(b < nblk && p.bg[b] == g && p.bc0[b] == c && p.bn[b] >= 1 && p.bn[b] <= (uint32_t)K1_BLOCK_CHUNKS && c + p.bn[b] <= cend);
            REQUIRE(p.blo[b] < p.bhi[b] && p.bhi[b] <= nrun);
            for (uint64_t ch = c; ch < c + p.bn[b]; ++ch) {               // the walker's lookup (d2g_kmers.h)
                uint32_t lo = p.blo[b], hi = p.bhi[b];
                while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (p.chunk_off[mid] <= ch) lo = mid; else hi = mid; }
                REQUIRE(lo >= t.go[g] && lo < t.go[g + 1]);
                REQUIRE(p.chunk_off[lo] <= ch && ch < p.chunk_off[lo + 1]);
                const uint64_t ci = ch - p.chunk_off[lo];
                REQUIRE(ci * K1_CHUNK < em[lo]);                          // at least one position: the lane reads inside its run
                const uint64_t n = std::min<uint64_t>(K1_CHUNK, em[lo] - ci * K1_CHUNK);
                const uint64_t span = (uint64_t)(w > k ? w : k);
                REQUIRE(ci * K1_CHUNK + n - 1 + span <= t.rl[lo]);        // ... and its last window ends inside it
                walked += n;
            }
            c += p.bn[b];
        }
        REQUIRE(c == cend);
    }
    REQUIRE(b == nblk && walked == total);
    return 0;
}

static bool same_plan(const PlanHost &a, const PlanHost &b) {
    return a.chunk_off == b.chunk_off && a.bc0 == b.bc0 && a.bg == b.bg && a.bn == b.bn && a.blo == b.blo && a.bhi == b.bhi && a.nkmers == b.nkmers &&
           a.nbases == b.nbases;
}

static int test_plans() {
    const int E[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 65535, 65536, 65537};
    const int KW[][2] = {{21, 22}, {21, 36}, {21, 37}, {31, 94}, {31, 95}, {5, 7}, {32, 33}, {32, 100}, {15, 1038}, {31, 31 + 4095}};
    for (const auto &kw : KW) {
        const int k = kw[0], w = kw[1];
        std::vector<uint32_t> lens;
        for (int e : E) lens.push_back((uint32_t)(e + w - 1));             // e emissions; e = 0: one base short of a window
        lens.push_back((uint32_t)k);                                       // as short as the packer lets a run be
        // genome 0: every length; genome 1: only runs shorter than w; genome 2: no run; genome 3: a zero-emission run between two others
        std::vector<uint32_t> all = lens;
        all.push_back((uint32_t)k); all.push_back((uint32_t)(w - 1));
        all.push_back((uint32_t)(w + 70)); all.push_back((uint32_t)(w - 1)); all.push_back((uint32_t)(w - 1)); all.push_back((uint32_t)(w + 5));
        const uint64_t n0 = lens.size();
        const Runs t(all, {0, n0, n0 + 2, n0 + 2, n0 + 6});
        if (check_plan(t, k, w)) return 1;
        PlanHost p;
        std::string err;
        REQUIRE(d2g_plan_build(t.view(k, w), p, err) == D2G_OK);
        for (size_t b = 0; b < p.bg.size(); ++b) REQUIRE(p.bg[b] == 0 || p.bg[b] == 3);      // genomes 1 and 2 own no workgroup
        // an input of empty genomes only: no workgroup at all
        const Runs none({(uint32_t)k, (uint32_t)(w - 1)}, {0, 1, 1, 2});
        PlanHost pe;
        REQUIRE(d2g_plan_build(none.view(k, w), pe, err) == D2G_OK && pe.bg.empty() && pe.nkmers == 0 && pe.nbases == (uint64_t)k + w - 1);
        // w <= k is no window: the plan of the same input is the plan it was
        PlanHost p0, pk, pless;
        REQUIRE(d2g_plan_build(t.view(k, 0), p0, err) == D2G_OK && d2g_plan_build(t.view(k, k), pk, err) == D2G_OK);
        REQUIRE(d2g_plan_build(t.view(k, k > 1 ? k - 1 : 1), pless, err) == D2G_OK);
        REQUIRE(same_plan(p0, pk) && same_plan(p0, pless) && !same_plan(p0, p));
        if (check_plan(t, k, 0)) return 1;
        // the count-range check adds the same numbers
        REQUIRE(d2g_plan_check_count_range(t.view(k, w), err) == D2G_OK);
    }
    // the cap: q = w - k + 1 = D2G_WINDOW_MAX_Q builds, one more is refused with a message
    const Runs t({10000}, {0, 1});
    PlanHost p;
    std::string err;
    REQUIRE(d2g_plan_build(t.view(31, 31 + D2G_WINDOW_MAX_Q - 1), p, err) == D2G_OK && err.empty());
    PlanHost p2;
    REQUIRE(d2g_plan_build(t.view(31, 31 + D2G_WINDOW_MAX_Q), p2, err) == D2G_ERR_UNSUPPORTED && !err.empty());
    // a run shorter than k is refused as it was, window or not
    const Runs bad({20}, {0, 1});
    PlanHost p3;
    REQUIRE(d2g_plan_build(bad.view(21, 30), p3, err) == D2G_ERR_INVALID);
    // emissions in closed form at the edges
    REQUIRE(d2g_run_emissions(0, 21, 30) == 0 && d2g_run_emissions(29, 21, 30) == 0 && d2g_run_emissions(30, 21, 30) == 1);
    REQUIRE(d2g_run_emissions(21, 21, 0) == 1 && d2g_run_emissions(21, 21, 21) == 1 && d2g_run_emissions(20, 21, 5) == 0);
    REQUIRE(d2g_run_emissions(0xFFFFFFFFull, 1, 0) == 0xFFFFFFFFull);
    return 0;
}

// the walker's loop over one lane's chunk (d2g_for_each_minimizer_its), on scores instead of packed bases
template <int D>
static void walk_chunk(const std::vector<uint64_t> &score, size_t first_pos, int n, int q, std::vector<uint64_t> &out, uint64_t &rerolls) {
    D2gMinQueue<D> mq;
    mq.clear();
    const int steps = q - 1 + n;
    for (int t = 0; t < steps; ++t) {
        mq.push(score[first_pos + t], t);
        const int first = t - (q - 1);
        if (first < 0) continue;
        mq.expire(first);
        if (mq.empty()) {
            ++rerolls;
            mq.clear();
            for (int u = first; u <= t; ++u) mq.push(score[first_pos + u], u);
        }
        out.push_back(mq.front());
    }
}

template <int D>
static int check_queue(const std::vector<uint64_t> &score, int q, uint64_t *rerolls_out = nullptr) {
    if (score.size() < (size_t)q) return 0;
    const size_t np = score.size() - q + 1;
    std::vector<uint64_t> got;
    uint64_t rerolls = 0;
    for (size_t p = 0; p < np; p += K1_CHUNK) walk_chunk<D>(score, p, (int)std::min<size_t>(K1_CHUNK, np - p), q, got, rerolls);
    REQUIRE(got.size() == np);
    for (size_t i = 0; i < np; ++i) REQUIRE(got[i] == *std::min_element(score.begin() + i, score.begin() + i + q));
    if (rerolls_out) *rerolls_out = rerolls;
    return 0;
}

static int test_queue() {
    std::mt19937_64 rng(12345);
    const int Q[] = {2, 3, 7, 8, 9, 16, 17, 63, 64, 65, 100, 1024};
    for (int q : Q) {
        const size_t n = (size_t)q + 300;
        std::vector<std::vector<uint64_t>> seqs;
        std::vector<uint64_t> s(n);
        for (auto &v : s) v = rng();
        seqs.push_back(s);                                                 // random
        for (size_t i = 0; i < n; ++i) s[i] = 1000 + i;
        seqs.push_back(s);                                                 // rising: the exact queue would hold q entries -- the dropped ones
        for (size_t i = 0; i < n; ++i) s[i] = 100000 - i;
        seqs.push_back(s);                                                 // falling: one entry
        std::fill(s.begin(), s.end(), 42);
        seqs.push_back(s);                                                 // one value: the leaving minimum is replaced by its equal
        for (size_t i = 0; i < n; ++i) s[i] = ~0ull - (i & 1);
        seqs.push_back(s);                                                 // the largest scores there are
        for (int per : {q - 1, q, q + 1}) {
            if (per < 1) continue;
            std::vector<uint64_t> unit(per);
            for (auto &v : unit) v = rng() % 50;                           // small alphabet: ties everywhere
            for (size_t i = 0; i < n; ++i) s[i] = unit[i % per];
            seqs.push_back(s);                                             // periodic: the minimum leaves once per period
        }
        for (size_t i = 0; i < n; ++i) s[i] = (i % 23) * 1000 + (rng() % 7);
        seqs.push_back(s);                                                 // sawtooth: rising stretches longer than the queue
        for (const auto &v : seqs) {
            if (check_queue<8>(v, q)) return 1;                            // the kernels' depth
            if (check_queue<1>(v, q)) return 1;                            // every step drops or re-rolls
            if (check_queue<3>(v, q)) return 1;
        }
    }
    // a sequence shorter than a window emits nothing
    const std::vector<uint64_t> shorty(5, 1);
    REQUIRE(check_queue<8>(shorty, 6) == 0);
    return 0;
}

static int test_names() {
    using d2h::ExactNameOpts;
    const ExactNameOpts none{21, true, 0, 0, ""}, eq{21, true, 0, 0, "", 21}, less{21, true, 0, 0, "", 20}, win{21, true, 0, 0, "", 30},
        full{21, false, 13, 2, "out", 22};
    const std::string plain = "g.fa.rc_canon.k21.FullMmerSet.DNA.kmerset64";
    REQUIRE(d2h::exact_key_file(none, "g.fa") == plain && d2h::exact_key_file(eq, "g.fa") == plain && d2h::exact_key_file(less, "g.fa") == plain);
    REQUIRE(d2h::exact_key_file(win, "g.fa") == "g.fa.rc_canon.k21.w30.FullMmerSet.DNA.kmerset64");
    REQUIRE(d2h::exact_key_file(full, "dir/g.fa") == "out/g.fa.seed13.k21.w22.ct_threshold2.FullMmerSet.DNA.kmerset64");
    REQUIRE(d2h::exact_count_file(d2h::exact_key_file(win, "g.fa")) == "g.fa.rc_canon.k21.w30.FullMmerSet.DNA.kmercounts.f64");
    return 0;
}

int main() {
    if (test_names()) return 1;
    if (test_plans()) return 1;
    if (test_queue()) return 1;
    std::printf("window selftest OK\n");
    return 0;
}
