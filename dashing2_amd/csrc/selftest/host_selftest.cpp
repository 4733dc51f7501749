// host_selftest.cpp -- exercises the x86 host half of libd2g (d2g_seqpack.cpp: seqpack ingest; d2g_host.cpp: x87 finalisation,
// densify, partition; d2g_epilogue.cpp: epilogues) under AddressSanitizer + UndefinedBehaviorSanitizer (`make sanitize` in
// dashing2_amd/csrc; the reference has the same kind of target: Makefile:102-103).  No GPU, no HIP: only the
// functions that never touch a device.  Exit code 0 = no finding (the sanitizers abort on any).
// Also the sketch side's input checks and launch plan (d2g_plan.cpp): the grid arithmetic whose indices the kernels trust.
#include "../../../include/d2g.h"
#include "../d2g_plan.h"
#include "../d2g_limits.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "selftest failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// ---- the launch plan, by brute force against its own tables.  Runs lie back to back from base 0.
struct Runs {
    std::vector<uint64_t> rs, go;
    std::vector<uint32_t> rl;
    Runs(std::vector<uint32_t> lens, std::vector<uint64_t> off) : go(std::move(off)), rl(std::move(lens)) {
        uint64_t at = 0;
        for (uint32_t l : rl) { rs.push_back(at); at += l; }
    }
    PackedRuns view(int k, size_t packed_bytes = 0) const { return {nullptr, packed_bytes, rs.data(), rl.data(), rl.size(), go.data(), go.size() - 1, k, 1}; }
};

static int check_plan(const Runs &t, int k) {
    const PackedRuns in = t.view(k);
    PlanHost p;
    std::string err;
    REQUIRE(d2g_plan_build(in, p, err) == D2G_OK && err.empty());
    const size_t nrun = in.nrun, nblk = p.bg.size();
    REQUIRE(p.chunk_off.size() == nrun + 1 && p.chunk_off[0] == 0);
    REQUIRE(p.bc0.size() == nblk && p.bn.size() == nblk && p.blo.size() == nblk && p.bhi.size() == nblk);
    uint64_t nk = 0, nb = 0;
    for (size_t r = 0; r < nrun; ++r) {
        const uint64_t rk = (uint64_t)t.rl[r] - k + 1;
        REQUIRE(p.chunk_off[r + 1] - p.chunk_off[r] == (rk + K1_CHUNK - 1) / K1_CHUNK);
        nk += rk; nb += t.rl[r];
    }
    REQUIRE(p.nkmers == nk && p.nbases == nb);
    size_t b = 0;
    for (size_t g = 0; g < in.n; ++g) {                              // a genome's blocks tile its chunks in order: no gap, no overlap
        uint64_t c = p.chunk_off[t.go[g]];
        const uint64_t cend = p.chunk_off[t.go[g + 1]];
        for (; c < cend; ++b) {
            REQUIRE(b < nblk && p.bg[b] == g && p.bc0[b] == c);
            REQUIRE(p.bn[b] >= 1 && p.bn[b] <= (uint32_t)K1_BLOCK_CHUNKS && c + p.bn[b] <= cend);
            for (size_t r = 0; r < nrun; ++r) {                      // [run_lo, run_hi) = the runs that own one of its chunks
                const bool owns = p.chunk_off[r] < c + p.bn[b] && p.chunk_off[r + 1] > c;
                REQUIRE(owns == (r >= p.blo[b] && r < p.bhi[b]));
            }
            c += p.bn[b];
        }
        REQUIRE(c == cend);
    }
    REQUIRE(b == nblk);
    // the tables through the one layout: an exactly-sized arena (a write past a piece's end into the next is a wrong read-back,
    // past the last an ASan report)
    const PlanLayout l = d2g_plan_layout(nrun, nblk);
    std::vector<uint8_t> arena(l.total, 0xEE);
    d2g_plan_fill(arena.data(), l, in, p);
    auto same = [&](size_t at, const void *src, size_t bytes) { return bytes == 0 || std::memcmp(arena.data() + at, src, bytes) == 0; };
    REQUIRE(same(l.run_start, t.rs.data(), nrun * 8) && same(l.run_len, t.rl.data(), nrun * 4) && same(l.run_chunk_off, p.chunk_off.data(), (nrun + 1) * 8));
    REQUIRE(same(l.blk_chunk0, p.bc0.data(), nblk * 8) && same(l.blk_genome, p.bg.data(), nblk * 4) && same(l.blk_nchunks, p.bn.data(), nblk * 4));
    REQUIRE(same(l.blk_run_lo, p.blo.data(), nblk * 4) && same(l.blk_run_hi, p.bhi.data(), nblk * 4));
    return 0;
}

static int check_layout(size_t nrun, size_t nblk) {
    const PlanLayout l = d2g_plan_layout(nrun, nblk);
    const std::pair<size_t, size_t> pieces[8] = {{l.run_start, nrun * 8}, {l.run_chunk_off, (nrun + 1) * 8}, {l.blk_chunk0, nblk * 8}, {l.run_len, nrun * 4},
                                                 {l.blk_genome, nblk * 4}, {l.blk_nchunks, nblk * 4}, {l.blk_run_lo, nblk * 4}, {l.blk_run_hi, nblk * 4}};
    size_t end = 0;
    for (const auto &pc : pieces) {                                  // 256-byte aligned, ascending, disjoint, inside total
        REQUIRE(pc.first % 256 == 0 && pc.first >= end);
        end = pc.first + pc.second;
    }
    REQUIRE(l.run_start == 0 && end <= l.total);
    return 0;
}

static int plan_selftest() {
    const int k = 31;
    const uint32_t one = k, wg = K1_BLOCK_CHUNKS * K1_CHUNK;         // a run of one k-mer; the k-mers of a full workgroup
    std::vector<Runs> seams = {
        Runs({one}, {0, 1}),                                         // a run of exactly k bases
        Runs({64 + k - 1, 65 + k - 1}, {0, 1, 2}),                   // 64 and 65 k-mers: one chunk, and one k-mer into a second
        Runs({wg + k - 1, wg + 1 + k - 1}, {0, 1, 2}),               // exactly K1_BLOCK_CHUNKS chunks, and K1_BLOCK_CHUNKS + 1
        Runs(std::vector<uint32_t>(3000, one), {0, 3000}),           // blocks of many runs; the last one short
        Runs({1000 * 64 + k - 1, 100 * 64 + k - 1, one}, {0, 2, 3}), // the second run straddles two blocks
        Runs({500, 77}, {0, 0, 1, 1, 2, 2}),                         // genomes without a run: first, in the middle, last
        Runs({}, {0}),                                               // n = 0, nrun = 0
        Runs({}, {0, 0, 0}),
    };
    for (const Runs &t : seams) if (check_plan(t, k)) return 1;
    for (int kk : {1, 32}) {
        if (check_plan(Runs({(uint32_t)kk, 32, 64 + (uint32_t)kk - 1, 64 + (uint32_t)kk, wg + (uint32_t)kk}, {0, 2, 2, 5}), kk)) return 1;
    }
    {   // the seams really are where the comments say
        PlanHost p; std::string err;
        REQUIRE(d2g_plan_build(seams[2].view(k), p, err) == D2G_OK && p.bg.size() == 3 && p.bn[0] == 1024 && p.bn[1] == 1024 && p.bn[2] == 1);
        PlanHost q;
        REQUIRE(d2g_plan_build(seams[3].view(k), q, err) == D2G_OK && q.bg.size() == 3 && q.bhi[0] - q.blo[0] == 1024 && q.bn[2] == 3000 - 2048);
        PlanHost s;
        REQUIRE(d2g_plan_build(seams[4].view(k), s, err) == D2G_OK && s.bg.size() == 3 && s.bhi[0] == 2 && s.blo[1] == 1 && s.bg[2] == 1);
    }
    // refusals
    {
        const Runs t({100, 50}, {0, 1, 2});
        PlanHost p; std::string err;
        for (int bad : {0, 33, -1}) REQUIRE(d2g_plan_build(t.view(bad), p, err) == D2G_ERR_UNSUPPORTED && !err.empty());
        REQUIRE(d2g_plan_build(Runs({100, 30}, {0, 1, 2}).view(31), p, err) == D2G_ERR_INVALID);     // a run shorter than k
        REQUIRE(d2g_plan_build(Runs({100, 50}, {0, 1, 1}).view(31), p, err) == D2G_ERR_INVALID);     // genome_run_off[n] != nrun
        REQUIRE(d2g_plan_build(Runs({100, 50}, {0, 1, 3}).view(31), p, err) == D2G_ERR_INVALID);
        REQUIRE(d2g_plan_build(Runs({100, 50}, {0, 2, 1, 2}).view(31), p, err) == D2G_ERR_INVALID);  // not monotone
        PackedRuns in = t.view(31);
        in.genome_run_off = nullptr;
        REQUIRE(d2g_plan_build(in, p, err) == D2G_ERR_INVALID);
        in = t.view(31); in.run_len = nullptr;
        REQUIRE(d2g_plan_build(in, p, err) == D2G_ERR_INVALID);
        in = t.view(31); in.run_start = nullptr;
        REQUIRE(d2g_plan_build(in, p, err) == D2G_ERR_INVALID);
        const Runs none({}, {0, 0});                                                                 // no run: no run table is needed
        in = none.view(31); in.run_len = nullptr; in.run_start = nullptr;
        PlanHost e;
        REQUIRE(d2g_plan_build(in, e, err) == D2G_OK && e.bg.empty());
    }
    // the tail pad: 64 bytes behind the byte of the last base, wherever in its byte that base lies; the LONGEST reach counts
    for (uint32_t len : {41u, 42u, 44u}) {                           // last base at 0, 1, 3 modulo 4
        const Runs t({len}, {0, 1});
        const size_t need = (len + 3) / 4 + 64;
        std::string err;
        REQUIRE(d2g_plan_check_tail(t.view(1, need), err) == D2G_OK && err.empty());
        REQUIRE(d2g_plan_check_tail(t.view(1, need - 1), err) == D2G_ERR_INVALID && !err.empty());
        Runs back({8, len}, {0, 2});                                 // the run that reaches furthest is listed first
        back.rs = {len, 0};
        REQUIRE(d2g_plan_check_tail(back.view(1, (len + 8 + 3) / 4 + 64), err) == D2G_OK);
        REQUIRE(d2g_plan_check_tail(back.view(1, (len + 8 + 3) / 4 + 63), err) == D2G_ERR_INVALID);
    }
    {
        std::string err;
        REQUIRE(d2g_plan_check_tail(Runs({}, {0, 0}).view(31, 0), err) == D2G_OK);
    }
    // the count range: 2^32 - 1 k-mers in a genome pass, 2^32 are refused; tables the builder rejects are left to it
    {
        std::string err;
        const uint32_t half = 1u << 31;
        REQUIRE(d2g_plan_check_count_range(Runs({half, half - 1}, {0, 2}).view(1), err) == D2G_OK && err.empty());
        REQUIRE(d2g_plan_check_count_range(Runs({half, half}, {0, 2}).view(1), err) == D2G_ERR_UNSUPPORTED && err.find("2^32") != std::string::npos);
        REQUIRE(d2g_plan_check_count_range(Runs({half, half}, {0, 1, 2}).view(1), err) == D2G_OK);   // two genomes of 2^31
        const Runs big({half, half}, {0, 2});
        PackedRuns in = big.view(1);
        in.run_len = nullptr;
        REQUIRE(d2g_plan_check_count_range(in, err) == D2G_OK);
        in.genome_run_off = nullptr;
        REQUIRE(d2g_plan_check_count_range(in, err) == D2G_OK);
    }
    for (size_t nrun : {0, 1, 31, 32, 33, 3000})
        for (size_t nblk : {0, 1, 63, 64, 65, 1030}) if (check_layout(nrun, nblk)) return 1;
    return 0;
}

// the limits that cut a large call into pieces (d2g_limits.h): unset, every one is the production constant; a switch takes a whole
// number of its range and nothing else
static int limits_selftest() {
    auto with = [](std::initializer_list<std::pair<const char *, const char *>> kv) {
        d2g_tuning t;
        for (const auto &p : kv) t.kv.emplace_back(p.first, p.second);
        return d2g_limits_tuning_resolve(t);
    };
    auto same = [](const d2g_limits_tuning &a, const d2g_limits_tuning &b) {
        return a.knn_chunk_slots == b.knn_chunk_slots && a.edit_knn_chunk_slots == b.edit_knn_chunk_slots &&
               a.interval_list_positions == b.interval_list_positions && a.screen_result_pairs == b.screen_result_pairs &&
               a.edit_grid_max == b.edit_grid_max && a.edit_dedup_chunk == b.edit_dedup_chunk && a.edit_dedup_max_chunks == b.edit_dedup_max_chunks;
    };
    const d2g_limits_tuning def = with({});
    REQUIRE(def.knn_chunk_slots == ((size_t)1 << 24) && def.knn_chunk_slots == KNN_CHUNK_SLOTS);
    REQUIRE(def.edit_knn_chunk_slots == ((size_t)1 << 24) && def.edit_knn_chunk_slots == NEAR_CHUNK_SLOTS);
    REQUIRE(def.interval_list_positions == 0);                      // 0: a third of the free device memory, asked per group
    REQUIRE(def.screen_result_pairs == (1ull << 30));
    REQUIRE(def.edit_grid_max == 0x7fffffffu);
    REQUIRE(def.edit_dedup_chunk == 1024 && def.edit_dedup_chunk == EDD_CHUNK && def.edit_dedup_max_chunks == 1024 && EDD_MAX_CHUNKS == 1024);
    REQUIRE(same(def, d2g_limits_tuning()));
    static const char *const names[] = {"D2G_KNN_CHUNK_SLOTS", "D2G_EDIT_KNN_CHUNK_SLOTS", "D2G_INTERVAL_LIST_POSITIONS", "D2G_SCREEN_RESULT_PAIRS",
                                        "D2G_EDIT_GRID_MAX", "D2G_EDIT_DEDUP_CHUNK", "D2G_EDIT_DEDUP_MAX_CHUNKS"};
    // not a whole number, below the range, beyond 64 bits: the default, whichever switch
    for (const char *n : names)
        for (const char *bad : {"", "0", "-1", "-256", "+4", " 4", "4 ", "1e3", "0x100", "12x", "x", "1.5", "18446744073709551616", "99999999999999999999999"})
            REQUIRE(same(def, with({{n, bad}})));
    // each switch moves its own limit and no other
    d2g_limits_tuning v = with({{"D2G_KNN_CHUNK_SLOTS", "1"}}), w = def;
    w.knn_chunk_slots = 1; REQUIRE(same(v, w));
    v = with({{"D2G_EDIT_KNN_CHUNK_SLOTS", "500"}}); w = def; w.edit_knn_chunk_slots = 500; REQUIRE(same(v, w));
    v = with({{"D2G_INTERVAL_LIST_POSITIONS", "1"}}); w = def; w.interval_list_positions = 1; REQUIRE(same(v, w));
    v = with({{"D2G_SCREEN_RESULT_PAIRS", "7"}}); w = def; w.screen_result_pairs = 7; REQUIRE(same(v, w));
    v = with({{"D2G_EDIT_GRID_MAX", "5"}}); w = def; w.edit_grid_max = 5; REQUIRE(same(v, w));
    v = with({{"D2G_EDIT_DEDUP_CHUNK", "256"}}); w = def; w.edit_dedup_chunk = 256; REQUIRE(same(v, w));
    v = with({{"D2G_EDIT_DEDUP_MAX_CHUNKS", "2"}}); w = def; w.edit_dedup_max_chunks = 2; REQUIRE(same(v, w));
    // the ends of the ranges
    REQUIRE(with({{"D2G_KNN_CHUNK_SLOTS", "18446744073709551615"}}).knn_chunk_slots == ~(size_t)0);
    REQUIRE(with({{"D2G_INTERVAL_LIST_POSITIONS", "1152921504606846975"}}).interval_list_positions == (~0ull) / 16);   // 16 bytes each still fit 64 bits
    REQUIRE(same(def, with({{"D2G_INTERVAL_LIST_POSITIONS", "1152921504606846976"}})));
    REQUIRE(with({{"D2G_SCREEN_RESULT_PAIRS", "1073741824"}}).screen_result_pairs == (1ull << 30));
    REQUIRE(same(def, with({{"D2G_SCREEN_RESULT_PAIRS", "1073741825"}})));                 // never more waves per launch than today
    REQUIRE(with({{"D2G_EDIT_GRID_MAX", "2147483647"}}).edit_grid_max == 0x7fffffffu);
    REQUIRE(same(def, with({{"D2G_EDIT_GRID_MAX", "2147483648"}})));
    REQUIRE(same(def, with({{"D2G_EDIT_GRID_MAX", "4294967297"}})));                       // (not 1 after a narrowing)
    for (const char *bad : {"255", "257", "1000", "128", "1048832", "4294967552"}) REQUIRE(same(def, with({{"D2G_EDIT_DEDUP_CHUNK", bad}})));
    REQUIRE(with({{"D2G_EDIT_DEDUP_CHUNK", "1048576"}}).edit_dedup_chunk == (1u << 20));
    REQUIRE(with({{"D2G_EDIT_DEDUP_MAX_CHUNKS", "1024"}}).edit_dedup_max_chunks == 1024);
    REQUIRE(same(def, with({{"D2G_EDIT_DEDUP_MAX_CHUNKS", "1025"}})));                     // the scratch holds EDD_MAX_CHUNKS counts
    // a valid switch beside an invalid one
    v = with({{"D2G_EDIT_DEDUP_CHUNK", "256"}, {"D2G_EDIT_DEDUP_MAX_CHUNKS", "0"}, {"D2G_EDIT_GRID_MAX", "7"}});
    w = def; w.edit_dedup_chunk = 256; w.edit_grid_max = 7; REQUIRE(same(v, w));
    // the compaction's chunk: today's formula without a switch, at most max_chunks workgroups with one, always whole workgroup rounds
    for (uint32_t N : {1u, 255u, 513u, 1024u, 1025u, 2500u, 1u << 20, (1u << 20) + 1, 3000000u, 0x7fffffffu}) {
        const uint32_t per = (uint32_t)(((uint64_t)N + 1023) / 1024), today = std::max<uint32_t>(1024, (per + 255) / 256 * 256);
        REQUIRE(d2g_edit_dedup_chunk(N, def) == today);
        for (const d2g_limits_tuning &t : {with({{"D2G_EDIT_DEDUP_CHUNK", "256"}}), with({{"D2G_EDIT_DEDUP_CHUNK", "256"}, {"D2G_EDIT_DEDUP_MAX_CHUNKS", "2"}}),
                                           with({{"D2G_EDIT_DEDUP_CHUNK", "256"}, {"D2G_EDIT_DEDUP_MAX_CHUNKS", "1"}}), with({{"D2G_EDIT_DEDUP_MAX_CHUNKS", "3"}})}) {
            const uint32_t c = d2g_edit_dedup_chunk(N, t);
            REQUIRE(c % 256 == 0 && c >= t.edit_dedup_chunk && ((uint64_t)N + c - 1) / c <= t.edit_dedup_max_chunks);
            REQUIRE(c == t.edit_dedup_chunk || (uint64_t)(c - 256) * t.edit_dedup_max_chunks < N);   // no larger than the cover needs
        }
    }
    REQUIRE(d2g_edit_dedup_chunk(513, with({{"D2G_EDIT_DEDUP_CHUNK", "256"}})) == 256);
    REQUIRE(d2g_edit_dedup_chunk(513, with({{"D2G_EDIT_DEDUP_CHUNK", "256"}, {"D2G_EDIT_DEDUP_MAX_CHUNKS", "2"}})) == 512);
    REQUIRE(d2g_edit_dedup_chunk(513, with({{"D2G_EDIT_DEDUP_CHUNK", "256"}, {"D2G_EDIT_DEDUP_MAX_CHUNKS", "1"}})) == 768);
    return 0;
}

int main() {
    if (plan_selftest() || limits_selftest()) return 1;
    std::mt19937_64 rng(7);
    // ---- seqpack: messy FASTA / FASTQ, lower case, N runs, short records, CRLF, no trailing newline, every k
    std::string fa;
    for (int r = 0; r < 40; ++r) {
        fa += (r % 5 == 4) ? "@q" : ">r";
        fa += std::to_string(r) + " desc\n";
        const size_t L = rng() % 700;
        std::string seq;
        for (size_t i = 0; i < L; ++i) seq += "ACGTacgtNn-"[rng() % (r % 3 ? 8 : 11)];
        if (r % 5 == 4) { fa += seq + "\n+\n" + std::string(seq.size(), 'I') + "\n"; continue; }
        for (size_t i = 0; i < seq.size(); i += 61) fa += seq.substr(i, 61) + (r % 7 == 0 ? "\r\n" : "\n");
    }
    fa += ">last\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT";      // no trailing newline
    for (int k = 1; k <= 32; ++k) {
        d2g_seqpack *sp = nullptr;
        REQUIRE(d2g_seqpack_create(k, &sp) == D2G_OK);
        REQUIRE(d2g_seqpack_add_fastx(sp, fa.data(), fa.size()) == D2G_OK);
        REQUIRE(d2g_seqpack_add_sequence(sp, "ACGT", 4) == D2G_OK);
        REQUIRE(d2g_seqpack_add_fastx(sp, "", 0) == D2G_OK);
        REQUIRE(d2g_seqpack_add_fastx_by_record(sp, fa.data(), fa.size()) == D2G_OK);
        const size_t ng = d2g_seqpack_ngenomes(sp), nr = d2g_seqpack_nruns(sp);
        REQUIRE(ng >= 3);
        const uint64_t *rs = d2g_seqpack_run_start(sp);
        const uint32_t *rl = d2g_seqpack_run_len(sp);
        const uint64_t *go = d2g_seqpack_genome_run_off(sp);
        REQUIRE(go[ng] == nr);
        uint64_t bases = 0;
        for (size_t i = 0; i < nr; ++i) { REQUIRE(rl[i] >= (uint32_t)k); REQUIRE(rs[i] == bases); bases += rl[i]; }
        REQUIRE(bases == d2g_seqpack_nbases(sp));
        REQUIRE(d2g_seqpack_packed_bytes(sp) >= (bases + 3) / 4 + 64);
        volatile uint8_t sink = 0;
        const uint8_t *pk = d2g_seqpack_packed(sp);
        for (size_t i = 0; i < d2g_seqpack_packed_bytes(sp); ++i) sink ^= pk[i];       // every byte readable
        uint64_t nk = 0;
        for (size_t g = 0; g < ng; ++g) nk += d2g_seqpack_nkmers(sp, g);
        REQUIRE(nk >= nr);
        d2g_seqpack_clear(sp);
        REQUIRE(d2g_seqpack_ngenomes(sp) == 0);
        REQUIRE(d2g_seqpack_add_path(sp, "/nonexistent/file.fa") == D2G_ERR_IO);
        d2g_seqpack_destroy(sp);
    }
    // ---- finalisation, densify, epilogues
    for (size_t S : {1, 2, 63, 64, 1000, 1024}) {
        const size_t m = d2g_oph_m(S), n = 5;
        std::vector<uint64_t> regs(n * m);
        for (auto &x : regs) x = (rng() % 4 == 0) ? ~0ull : rng() >> (rng() % 40);
        for (size_t i = 0; i < m; ++i) regs[2 * m + i] = ~0ull;                  // an empty sketch
        for (size_t i = 0; i < m; ++i) regs[3 * m + i] = 0;                       // sum == 0
        std::vector<double> sigs(n * S), cards(n);
        REQUIRE(d2g_oph_finalize(regs.data(), n, m, S, sigs.data(), cards.data(), 3) == D2G_OK);
        for (double c : cards) REQUIRE(!(c < 0));
        size_t filled = 0;
        REQUIRE(d2g_densify(sigs.data(), n, S, &filled, 2) == D2G_OK);
        std::vector<float> lut(S + 1);
        for (int meas = 0; meas < 6; ++meas)
            for (int ms = 0; ms < 2; ++ms) {
                const int rc = d2g_epilogue_lut(S, meas, 31, ms, lut.data());
                REQUIRE(rc == D2G_OK || rc == D2G_ERR_UNSUPPORTED);
                for (uint64_t neq : {uint64_t(0), uint64_t(S / 2), uint64_t(S)}) {
                    volatile float a = d2g_epilogue_neq(neq, S, cards[0], cards[1], meas, 31);
                    volatile float b = d2g_epilogue_gtlt(S - neq, 0, S, 1e6, 0.0, meas, 0);
                    (void)a; (void)b;
                }
            }
        const size_t N = 37;
        std::vector<uint32_t> ca(N * (N - 1) / 2), cb(ca.size());
        for (size_t i = 0; i < ca.size(); ++i) { ca[i] = rng() % (S + 1); cb[i] = rng() % (S - ca[i] + 1); }
        std::vector<double> cd(N, 1234.5);
        std::vector<float> out(ca.size());
        for (int meas = 0; meas < 6; ++meas) {
            REQUIRE(d2g_epilogue_ut(ca.data(), cb.data(), cd.data(), N, S, 0, N, meas, 21, 0, 3, out.data()) == D2G_OK);
            REQUIRE(d2g_epilogue_ut(ca.data(), nullptr, cd.data(), N, S, 5, 20, meas, 21, 1, 2, out.data()) == D2G_OK);
        }
    }
    // ---- partition / counts
    for (size_t N : {1, 2, 3, 10, 1000, 50000})
        for (int parts : {1, 2, 3, 8, 13}) {
            std::vector<size_t> b(parts + 1);
            REQUIRE(d2g_ut_partition(N, parts, b.data()) == D2G_OK);
            REQUIRE(b[0] == 0 && b[parts] == N);
            size_t tot = 0;
            for (int p = 0; p < parts; ++p) { REQUIRE(b[p] <= b[p + 1]); tot += d2g_ut_count(N, b[p], b[p + 1]); }
            REQUIRE(tot == N * (N - 1) / 2);
        }
    // ---- neighbour lists: exactly-sized arrays (a read or write past a row's entries or past the outputs is an ASan report)
    {
        const size_t S = 8, n = 4, cap = 3;
        const float lut[S + 1] = {0.f, 0.125f, 0.25f, 0.25f, 0.5f, 0.625f, 0.75f, 0.875f, 1.f};
        const std::vector<uint32_t> rowcnt = {3, 0, 1, 2}, ids = {9, 4, 7, 0, 0, 0, 2, 0, 0, 5, 1}, cts = {2, 8, 3, 0, 0, 0, 1, 0, 0, 4, 4};   // the last row's third slot does not exist
        std::vector<uint64_t> indptr(n + 1);
        std::vector<uint32_t> indices(6);
        std::vector<float> data(6);
        size_t need = 0, over = 0;
        REQUIRE(d2g_knn_finish(rowcnt.data(), ids.data(), cts.data(), n, cap, lut, S, 0, indptr.data(), nullptr, nullptr, 0, &need, &over) == D2G_ERR_NOMEM);
        REQUIRE(need == 6 && over == 0 && indptr[4] == 6);
        REQUIRE(d2g_knn_finish(rowcnt.data(), ids.data(), cts.data(), n, cap, lut, S, 0, indptr.data(), indices.data(), data.data(), 6, &need, &over) == D2G_OK);
        REQUIRE(indices[0] == 4 && indices[1] == 7 && indices[2] == 9 && data[0] == 1.f && data[1] == 0.25f && data[2] == 0.25f && indices[4] == 1 && indices[5] == 5);
        REQUIRE(d2g_knn_finish(rowcnt.data(), ids.data(), cts.data(), n, cap, lut, S, 1, indptr.data(), indices.data(), data.data(), 6, nullptr, nullptr) == D2G_OK);
        REQUIRE(indices[0] == 7 && indices[1] == 9 && indices[2] == 4);
        const std::vector<uint32_t> big = {4, 0, 1, 2};
        REQUIRE(d2g_knn_finish(big.data(), ids.data(), cts.data(), n, cap, lut, S, 0, indptr.data(), indices.data(), data.data(), 6, &need, &over) == D2G_ERR_INVALID && over == 1);
    }
    // ---- greedy clusters: exactly-sized arrays; a malformed assignment is refused before anything is indexed with it
    {
        const std::vector<uint32_t> assign = {0, 0, 2, 3, 3, 0};
        std::vector<uint64_t> indptr(assign.size() + 1);
        std::vector<uint32_t> indices(assign.size());
        size_t nc = 99;
        REQUIRE(d2g_dedup_clusters(assign.data(), assign.size(), indptr.data(), indices.data(), &nc) == D2G_OK && nc == 3);
        REQUIRE(indptr[1] == 3 && indptr[2] == 4 && indptr[3] == 6 && indices[0] == 0 && indices[1] == 1 && indices[2] == 5 && indices[3] == 2 && indices[5] == 4);
        for (const std::vector<uint32_t> &bad : {std::vector<uint32_t>{1, 1}, {0, 2, 2}, {0, 0, 1}, {0, 4000000000u}})
            REQUIRE(d2g_dedup_clusters(bad.data(), bad.size(), indptr.data(), indices.data(), &nc) == D2G_ERR_INVALID);
        REQUIRE(d2g_dedup_clusters(nullptr, 0, indptr.data(), nullptr, &nc) == D2G_OK && nc == 0 && indptr[0] == 0);
    }
    REQUIRE(d2g_wang_hash(133348) != 0 && d2g_seed_mask(0) == 0 && d2g_seed_mask(5) != 0);
    // ---- the k-mers behind registers: exactly-sized arrays, odd S (the last of every m is not read into the output)
    for (uint64_t x : {uint64_t(0), ~uint64_t(0), uint64_t(133348), rng(), rng()})
        REQUIRE(d2g_wang_hash_inverse(d2g_wang_hash(x)) == x && d2g_wang_hash(d2g_wang_hash_inverse(x)) == x);
    for (size_t S : {1, 2, 5, 64}) {
        const size_t m = d2g_oph_m(S), n = 3;
        std::vector<uint64_t> regs(n * m), ids(n * S);
        for (auto &x : regs) x = (rng() % 3 == 0) ? ~0ull : rng();
        REQUIRE(d2g_oph_kmer_ids(regs.data(), n, m, S, ids.data()) == D2G_OK);
        for (size_t i = 0; i < n; ++i)
            for (size_t r = 0; r < S; ++r) REQUIRE(d2g_wang_hash(ids[i * S + r] ^ d2g_oph_xor_const()) == regs[i * m + r]);
        REQUIRE(d2g_oph_kmer_ids(regs.data(), n, m, m + 1, ids.data()) == D2G_ERR_INVALID);
        REQUIRE(d2g_oph_kmer_ids(nullptr, 0, m, S, nullptr) == D2G_OK);
    }
    std::printf("host selftest OK\n");
    return 0;
}
