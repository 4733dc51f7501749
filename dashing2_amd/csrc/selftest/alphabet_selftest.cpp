// alphabet_selftest.cpp -- the host side of the amino-acid walker (K1a) under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make sanitize` in dashing2_amd/csrc).  No GPU, no HIP.  Exit code 0 = no finding.
//   1. the alphabet tables (d2g_alphabet.h): sizes, largest k, every byte's code, names, d2g_key_bits (DNA: 2k bit for bit)
//   2. the byte-per-residue packer (d2g_seqpack.cpp) against a direct restatement: streams, runs, per-genome k-mer totals -- lower case,
//      every invalid letter, records shorter than k, by-record mode, the 64-byte pad, the run split with its k - 1 overlap, clear()
//   3. d2g_plan_check_tail counting a byte per symbol, and what d2g_plan_build refuses under a protein alphabet
#include "../../../include/d2g.h"
#include "../d2g_alphabet.h"
#include "../d2g_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "alphabet selftest failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static const int ALPHABETS[4] = {D2G_ALPHABET_PROTEIN20, D2G_ALPHABET_PROTEIN_14, D2G_ALPHABET_PROTEIN_3BIT, D2G_ALPHABET_PROTEIN_6};
static const char LETTERS[] = "ACDEFGHIKLMNPQRSTVWY";

static int check_tables() {
    const int sizes[4] = {20, 14, 8, 6}, maxk[4] = {14, 16, 21, 24};
    const char *names[4] = {"PROTEIN20", "PROTEIN_14", "PROTEIN_3BIT", "PROTEIN_6"};
    for (int i = 0; i < 4; ++i) {
        const int a = ALPHABETS[i];
        REQUIRE(d2g_alphabet_size(a) == sizes[i] && d2g_alphabet_max_k(a) == maxk[i] && std::strcmp(d2g_alphabet_name(a), names[i]) == 0);
        int valid = 0;
        std::vector<int> seen(sizes[i], 0);
        for (int b = -3; b < 260; ++b) {
            const int c = d2g_alphabet_code(a, b);
            const bool letter = b > 0 && b < 256 && std::strchr(LETTERS, b >= 'a' && b <= 'z' ? b - 32 : b) != nullptr;
            REQUIRE((c >= 0) == letter && c < sizes[i]);
            if (c >= 0) { ++valid; seen[c] = 1; REQUIRE(c == d2g_alphabet_code(a, b ^ 32)); }
        }
        REQUIRE(valid == 40);
        for (int s : seen) REQUIRE(s == 1);
        // the widest key stays below 2^63; one more residue would pass 2^64
        unsigned __int128 top = 1;
        for (int j = 0; j < maxk[i]; ++j) top *= (unsigned)sizes[i];
        REQUIRE(top <= ((unsigned __int128)1 << 63) && top * (unsigned)sizes[i] > ((unsigned __int128)1 << 64));
        REQUIRE(d2g_key_bits(maxk[i], a) <= 63 && d2g_key_bits(maxk[i] + 1, a) == 0 && d2g_key_bits(0, a) == 0);
    }
    REQUIRE(d2g_alphabet_code(D2G_ALPHABET_PROTEIN20, 'Y') == 19 && d2g_alphabet_code(D2G_ALPHABET_PROTEIN_14, 'q') == 3);
    REQUIRE(d2g_alphabet_code(D2G_ALPHABET_PROTEIN_3BIT, 'P') == 7 && d2g_alphabet_code(D2G_ALPHABET_PROTEIN_6, 'V') == 5);
    REQUIRE(d2g_alphabet_size(D2G_ALPHABET_DNA) == 4 && d2g_alphabet_max_k(D2G_ALPHABET_DNA) == 32 && std::strcmp(d2g_alphabet_name(0), "DNA") == 0);
    REQUIRE(d2g_alphabet_size(1) == 0 && d2g_alphabet_max_k(1) == 0 && d2g_alphabet_size(6) == 0 && d2g_alphabet_name(7)[0] == 0);
    for (int k = 1; k <= 32; ++k) REQUIRE(d2g_key_bits(k, D2G_ALPHABET_DNA) == 2 * k);
    REQUIRE(d2g_key_bits(33, D2G_ALPHABET_DNA) == 0);
    const int seam[6][3] = {{2, 7, 31}, {2, 8, 35}, {3, 10, 30}, {3, 11, 33}, {5, 12, 32}, {5, 13, 34}};
    for (auto &s : seam) REQUIRE(d2g_key_bits(s[1], s[0]) == s[2]);
    REQUIRE(d2g_key_bits(1, D2G_ALPHABET_PROTEIN20) == 5 && d2g_key_bits(21, D2G_ALPHABET_PROTEIN_3BIT) == 63);
    return 0;
}

// what the packer must hold for a list of records, restated: runs of letters, those shorter than k dropped
struct Model {
    std::vector<uint8_t> codes;
    std::vector<uint64_t> rs, go{0}, nk;
    std::vector<uint32_t> rl;
    void record(const std::string &seq, int k, int a, uint64_t &tot) {
        size_t i = 0;
        while (i <= seq.size()) {
            size_t j = i;
            while (j < seq.size() && d2g_alphabet_code(a, (unsigned char)seq[j]) >= 0) ++j;
            if (j - i >= (size_t)k) {
                rs.push_back(codes.size()); rl.push_back((uint32_t)(j - i)); tot += j - i - k + 1;
                for (size_t p = i; p < j; ++p) codes.push_back((uint8_t)d2g_alphabet_code(a, (unsigned char)seq[p]));
            }
            i = j + 1;
        }
    }
    void genome(uint64_t tot) { go.push_back(rs.size()); nk.push_back(tot); }
};

static int same(const d2g_seqpack *sp, const Model &m) {
    REQUIRE(d2g_seqpack_ngenomes(sp) == m.nk.size() && d2g_seqpack_nruns(sp) == m.rs.size());
    REQUIRE(d2g_seqpack_nbases(sp) == m.codes.size());
    REQUIRE(d2g_seqpack_packed_bytes(sp) == m.codes.size() + 64);
    const uint8_t *pk = d2g_seqpack_packed(sp);
    REQUIRE(((uintptr_t)pk & 3) == 0);
    REQUIRE(m.codes.empty() || std::memcmp(pk, m.codes.data(), m.codes.size()) == 0);
    for (size_t i = 0; i < 64; ++i) REQUIRE(pk[m.codes.size() + i] == 0);
    for (size_t r = 0; r < m.rs.size(); ++r) REQUIRE(d2g_seqpack_run_start(sp)[r] == m.rs[r] && d2g_seqpack_run_len(sp)[r] == m.rl[r]);
    for (size_t g = 0; g <= m.nk.size(); ++g) REQUIRE(d2g_seqpack_genome_run_off(sp)[g] == m.go[g]);
    for (size_t g = 0; g < m.nk.size(); ++g) REQUIRE(d2g_seqpack_nkmers(sp, g) == m.nk[g]);
    // the plan unit accepts what the packer made, and a stream one byte short of its pad is refused
    PackedRuns in{pk, d2g_seqpack_packed_bytes(sp), d2g_seqpack_run_start(sp), d2g_seqpack_run_len(sp), m.rs.size(), d2g_seqpack_genome_run_off(sp),
                  m.nk.size(), 0, 0, 0, d2g_seqpack_alphabet(sp)};
    std::string err;
    REQUIRE(d2g_plan_check_tail(in, err) == D2G_OK);
    if (!m.rs.empty()) {
        in.packed_bytes -= 1;
        REQUIRE(d2g_plan_check_tail(in, err) == D2G_ERR_INVALID);
        in.alphabet = D2G_ALPHABET_DNA;                                     // the same table read as 2-bit bases needs a quarter: accepted
        REQUIRE(d2g_plan_check_tail(in, err) == D2G_OK);
    }
    return 0;
}

static int check_packer() {
    std::mt19937_64 rng(7);
    const std::string invalid = "XBZJUOxbzjuo*-.1 \t";
    for (int a : ALPHABETS) {
        for (int k : {1, 5, d2g_alphabet_max_k(a)}) {
            d2g_seqpack *sp = nullptr, *by = nullptr;
            REQUIRE(d2g_seqpack_create_alphabet(k, a, &sp) == D2G_OK && d2g_seqpack_alphabet(sp) == a);
            REQUIRE(d2g_seqpack_create_alphabet(k, a, &by) == D2G_OK);
            for (int round = 0; round < 2; ++round) {                       // the second round after clear(): stale bytes must not show
                Model m, mb;
                for (int g = 0; g < 4; ++g) {
                    std::string fasta;
                    uint64_t tot = 0;
                    const int nrec = 1 + (int)(rng() % 5);
                    for (int r = 0; r < nrec; ++r) {
                        std::string seq;
                        const size_t len = r == 1 ? (size_t)(k - 1) : (size_t)(rng() % 400);      // one record shorter than k
                        for (size_t i = 0; i < len; ++i) {
                            const uint64_t v = rng();
                            char c = LETTERS[v % 20];
                            if ((v >> 8) % 3 == 0) c = (char)(c + 32);
                            if ((v >> 16) % 17 == 0 && r != 1) c = invalid[(v >> 24) % invalid.size()];
                            seq.push_back(c);
                        }
                        uint64_t rt = 0;
                        m.record(seq, k, a, tot);
                        mb.record(seq, k, a, rt);
                        mb.genome(rt);
                        fasta += ">rec" + std::to_string(r) + " comment\n";
                        for (size_t i = 0; i < seq.size(); i += 61) fasta += seq.substr(i, 61) + "\n";     // line breaks do not end a run
                        if (seq.empty()) fasta += "\n";
                    }
                    m.genome(tot);
                    REQUIRE(d2g_seqpack_add_fastx(sp, fasta.data(), fasta.size()) == D2G_OK);
                    REQUIRE(d2g_seqpack_add_fastx_by_record(by, fasta.data(), fasta.size()) == D2G_OK);
                }
                if (same(sp, m) || same(by, mb)) return 1;
                REQUIRE(std::strcmp(d2g_seqpack_name(by, 0), "rec0") == 0);
                d2g_seqpack_clear(sp); d2g_seqpack_clear(by);
            }
            // a raw sequence, no header
            Model m;
            uint64_t tot = 0;
            const std::string raw = "acdefXGHIKLMNPQRSTVWYacd*ACD";
            m.record(raw, k, a, tot); m.genome(tot);
            REQUIRE(d2g_seqpack_add_sequence(sp, raw.data(), raw.size()) == D2G_OK);
            if (same(sp, m)) return 1;
            d2g_seqpack_destroy(sp); d2g_seqpack_destroy(by);
        }
        d2g_seqpack *sp = nullptr;
        REQUIRE(d2g_seqpack_create_alphabet(d2g_alphabet_max_k(a) + 1, a, &sp) == D2G_ERR_UNSUPPORTED && sp == nullptr);
        REQUIRE(d2g_seqpack_create_alphabet(0, a, &sp) == D2G_ERR_UNSUPPORTED);
    }
    d2g_seqpack *sp = nullptr;
    REQUIRE(d2g_seqpack_create_alphabet(5, 1, &sp) == D2G_ERR_UNSUPPORTED && d2g_seqpack_create_alphabet(5, 6, &sp) == D2G_ERR_UNSUPPORTED);
    REQUIRE(d2g_seqpack_create_alphabet(32, D2G_ALPHABET_DNA, &sp) == D2G_OK && d2g_seqpack_alphabet(sp) == D2G_ALPHABET_DNA);
    d2g_seqpack_destroy(sp);
    return 0;
}

// the split of a long run: pieces of at most D2G_MAX_RUN residues that overlap by k - 1, so that no k-mer is lost or doubled
static int check_split() {
    setenv("D2G_MAX_RUN", "100", 1);
    const int k = 5;
    d2g_seqpack *sp = nullptr;
    REQUIRE(d2g_seqpack_create_alphabet(k, D2G_ALPHABET_PROTEIN20, &sp) == D2G_OK);
    unsetenv("D2G_MAX_RUN");
    std::string seq;
    for (int i = 0; i < 1000; ++i) seq.push_back(LETTERS[(i * 7 + i / 13) % 20]);
    REQUIRE(d2g_seqpack_add_sequence(sp, seq.data(), seq.size()) == D2G_OK);
    REQUIRE(d2g_seqpack_nkmers(sp, 0) == 1000 - k + 1 && d2g_seqpack_nbases(sp) == 1000);
    const size_t nrun = d2g_seqpack_nruns(sp);
    uint64_t kmers = 0, next = 0;
    for (size_t r = 0; r < nrun; ++r) {
        const uint64_t s = d2g_seqpack_run_start(sp)[r], l = d2g_seqpack_run_len(sp)[r];
        REQUIRE(l <= 100 && l >= (uint64_t)k && s == next);
        kmers += l - k + 1;
        next = s + l - (k - 1);
    }
    REQUIRE(nrun > 1 && kmers == 1000 - k + 1 && next + (k - 1) == 1000);
    d2g_seqpack_destroy(sp);
    return 0;
}

static int check_plan_refusals() {
    const uint64_t rs[2] = {0, 30}, go[2] = {0, 2};
    const uint32_t rl[2] = {30, 200};
    for (int a : ALPHABETS) {
        const int kmax = d2g_alphabet_max_k(a);
        PlanHost p;
        std::string err;
        PackedRuns in{nullptr, 0, rs, rl, 2, go, 1, kmax, 0, 0, a};
        REQUIRE(d2g_plan_build(in, p, err) == D2G_OK && p.nkmers == (uint64_t)(30 - kmax + 1) + (200 - kmax + 1) && p.nbases == 230);
        REQUIRE(p.chunk_off[2] == (uint64_t)((30 - kmax + 1 + 63) / 64 + (200 - kmax + 1 + 63) / 64));      // chunks of 64 emissions, as for DNA
        PlanHost q;
        in.canon = 1;
        REQUIRE(d2g_plan_build(in, q, err) == D2G_ERR_INVALID && err.find("canon") != std::string::npos);
        in.canon = 0; in.k = kmax + 1;
        REQUIRE(d2g_plan_build(in, q, err) == D2G_ERR_UNSUPPORTED && err.find("largest exact k") != std::string::npos);
        in.k = 5; in.w = 9;
        REQUIRE(d2g_plan_build(in, q, err) == D2G_ERR_UNSUPPORTED && err.find("window") != std::string::npos);
        in.w = 5;                                                            // w <= k is no window
        REQUIRE(d2g_plan_build(in, q, err) == D2G_OK);
    }
    PlanHost q;
    std::string err;
    PackedRuns bad{nullptr, 0, rs, rl, 2, go, 1, 5, 0, 0, 1};
    REQUIRE(d2g_plan_build(bad, q, err) == D2G_ERR_INVALID && err == "unknown alphabet");
    return 0;
}

int main() {
    if (check_tables() || check_packer() || check_split() || check_plan_refusals()) return 1;
    std::printf("alphabet selftest OK\n");
    return 0;
}
