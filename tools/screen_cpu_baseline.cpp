// screen_cpu_baseline.cpp -- the algorithm of the reference's `contain` RESTATED on the host, as the CPU figure beside the GPU's in
// tools/screen_time.py.  NOT a dashing2 binary (the reference cannot be built: its encoder and hash live in absent submodules): a hash
// map key -> [reference ids] built from a .kmer64 database, one lookup of maskfn(kmer) per k-mer of every FASTA file, one OpenMP thread
// per file (src/contain_main.cpp:34-59,188-244), with std::unordered_map where the reference has robin_hood's flat map.
//   g++ -O3 -std=c++17 -fopenmp screen_cpu_baseline.cpp -o screen_cpu_baseline
//   screen_cpu_baseline db.kmer64 a.fa b.fa ...      -> one JSON line; the files together are ONE query
#include <omp.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

static inline uint64_t wang64(uint64_t k) {
    k = ~k + (k << 21); k ^= k >> 24; k = k + (k << 3) + (k << 8); k ^= k >> 14;
    k = k + (k << 2) + (k << 4); k ^= k >> 28; k += k << 31;
    return k;
}

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s db.kmer64 query.fa...\n", argv[0]); return 2; }
    std::FILE *fp = std::fopen(argv[1], "rb");
    uint32_t hdr[4]; uint64_t seed;
    if (!fp || std::fread(hdr, 4, 4, fp) != 4 || std::fread(&seed, 8, 1, fp) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const bool canon = hdr[0] & 0x100;
    const uint32_t S = hdr[1];
    const int k = int(hdr[2]);
    if (S == 0 || k < 1 || k > 32) { std::fprintf(stderr, "database out of range\n"); return 2; }
    std::vector<uint64_t> keys;
    for (uint64_t v; std::fread(&v, 8, 1, fp) == 1;) keys.push_back(v);
    std::fclose(fp);
    const size_t nrefs = keys.size() / S;
    const uint64_t xormask = seed ? wang64(seed) : 0;
    double t0 = omp_get_wtime();
    std::unordered_map<uint64_t, std::vector<uint32_t>> kmer2ids;                 // :188-198
    kmer2ids.reserve(keys.size());
    for (size_t i = 0; i < nrefs; ++i) for (uint32_t j = 0; j < S; ++j) kmer2ids[keys[i * S + j]].push_back(uint32_t(i));
    const double t_build = omp_get_wtime() - t0;

    const int nfiles = argc - 2;
    std::vector<std::unordered_map<uint64_t, uint64_t>> res(nfiles);
    std::vector<uint64_t> nk(nfiles, 0);
    const uint64_t kmask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    const int rcshift = 2 * (k - 1);
    t0 = omp_get_wtime();
#pragma omp parallel for schedule(dynamic)
    for (int f = 0; f < nfiles; ++f) {                                            // get_results(): one thread per file, :37-57
        std::FILE *q = std::fopen(argv[2 + f], "rb");
        if (!q) continue;
        std::vector<char> buf(1 << 22);
        auto &myres = res[f];
        uint64_t fwd = 0, rc = 0, n = 0;
        int have = 0;
        bool header = false, bol = true;
        for (size_t got; (got = std::fread(buf.data(), 1, buf.size(), q)) > 0;)
            for (size_t i = 0; i < got; ++i) {
                const char c = buf[i];
                if (c == '\n') { header = false; bol = true; continue; }
                if (bol && c == '>') { header = true; have = 0; }
                bol = false;
                if (header) continue;
                int b;
                switch (c) { case 'A': case 'a': b = 0; break; case 'C': case 'c': b = 1; break; case 'G': case 'g': b = 2; break;
                             case 'T': case 't': b = 3; break; default: b = -1; }
                if (b < 0) { have = 0; continue; }
                fwd = ((fwd << 2) | uint64_t(b)) & kmask;
                rc = (rc >> 2) | (uint64_t(3 - b) << rcshift);
                if (++have < k) continue;
                ++n;
                const uint64_t kmer = wang64((canon ? (fwd < rc ? fwd : rc) : fwd) ^ xormask);      // maskfn, :41
                if (kmer2ids.find(kmer) == kmer2ids.end()) continue;             // :43-44
                ++myres[kmer];                                                    // :45-47
            }
        std::fclose(q);
        nk[f] = n;
    }
    // the files are pieces of one query: their maps add up (operator+=, :25-32), then the loops of :224-231
    std::unordered_map<uint64_t, uint64_t> all;
    for (auto &m : res) for (auto &p : m) all[p.first] += p.second;
    std::vector<uint32_t> matches(nrefs, 0), matchsums(nrefs, 0);
    uint64_t hits = 0;
    for (auto &p : all) { hits += p.second; for (uint32_t r : kmer2ids[p.first]) { ++matches[r]; matchsums[r] += uint32_t(p.second); } }
    const double t_query = omp_get_wtime() - t0;
    uint64_t kmers = 0;
    for (uint64_t v : nk) kmers += v;
    std::printf("{\"threads\": %d, \"files\": %d, \"references\": %zu, \"S\": %u, \"k\": %d, \"map_build_s\": %.6f, \"query_s\": %.6f, \"kmers\": %llu, "
                "\"kmers_per_s\": %.6g, \"hits\": %llu, \"matches_ref0\": %u, \"matchsum_ref0\": %u}\n",
                omp_get_max_threads(), nfiles, nrefs, S, k, t_build, t_query, (unsigned long long)kmers, kmers / t_query, (unsigned long long)hits,
                nrefs ? matches[0] : 0u, nrefs ? matchsums[0] : 0u);
    return 0;
}
