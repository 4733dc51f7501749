// edit_cpu_baseline.cpp -- the CPU yardstick of tools/edit_time.py: THIS REPOSITORY'S OWN restatement of block Myers (Myers 1999 in Hyyro's
// block form, 64-bit words, the match masks of a row record built once and used for all of its pairs), one OpenMP thread per row.  It is
// not edlib and not a dashing2 binary; it does no banding and no early exit, like the GPU kernel it is compared with.
//
//   edit_cpu_baseline <records.bin> <r0> <r1> <step> <threads>
// records.bin: u64 N, u64 off[N + 1], the bytes.  Rows r0, r0 + step, ... < r1 of the strict upper triangle are computed (every j > row).
// Prints one JSON line: seconds, rows, pairs, cells = sum of m n, and the sum of all distances (the caller checks it against the GPU's).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <omp.h>

static uint32_t myers(const std::vector<uint64_t> &peq, size_t B, uint32_t m, const uint8_t *y, uint32_t n, std::vector<uint64_t> &pv, std::vector<uint64_t> &mv) {
    if (m == 0) return n;
    for (size_t b = 0; b < B; ++b) { pv[b] = ~uint64_t(0); mv[b] = 0; }
    uint32_t score = m;
    const unsigned hb = (m - 1) & 63;
    for (uint32_t c = 0; c < n; ++c) {
        const uint64_t *eqc = &peq[size_t(y[c]) * B];
        uint64_t hp = 1, hm = 0;                                   // +1 enters the first block: D[0][j] = j
        for (size_t b = 0; b < B; ++b) {
            uint64_t Eq = eqc[b];
            const uint64_t Pv = pv[b], Mv = mv[b], Xv = Eq | Mv;
            Eq |= hm;
            const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
            uint64_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
            const unsigned bit = b + 1 == B ? hb : 63;
            const uint64_t hpo = (Ph >> bit) & 1, hmo = (Mh >> bit) & 1;
            Ph = (Ph << 1) | hp; Mh = (Mh << 1) | hm;
            pv[b] = Mh | ~(Xv | Ph);
            mv[b] = Ph & Xv;
            hp = hpo; hm = hmo;
        }
        score += uint32_t(hp) - uint32_t(hm);
    }
    return score;
}

int main(int argc, char **argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: edit_cpu_baseline records.bin r0 r1 step threads\n"); return 2; }
    std::FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) { std::perror(argv[1]); return 1; }
    uint64_t N = 0;
    if (std::fread(&N, 8, 1, fp) != 1) return 1;
    std::vector<uint64_t> off(N + 1);
    if (std::fread(off.data(), 8, N + 1, fp) != N + 1) return 1;
    std::vector<uint8_t> bytes(off[N] + 1);
    if (std::fread(bytes.data(), 1, off[N], fp) != off[N]) return 1;
    std::fclose(fp);
    const size_t r0 = std::strtoull(argv[2], nullptr, 10), r1 = std::strtoull(argv[3], nullptr, 10), step = std::strtoull(argv[4], nullptr, 10);
    const int nt = std::atoi(argv[5]);
    if (r1 > N || r0 > r1 || step < 1 || nt < 1) return 2;
    std::vector<size_t> rows;
    for (size_t r = r0; r < r1; r += step) rows.push_back(r);
    uint64_t sum = 0, pairs = 0;
    long double cells = 0;
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel num_threads(nt) reduction(+ : sum, pairs, cells)
    {
        std::vector<uint64_t> peq, pv, mv;
#pragma omp for schedule(dynamic, 1)
        for (size_t k = 0; k < rows.size(); ++k) {
            const size_t i = rows[k];
            const uint32_t m = uint32_t(off[i + 1] - off[i]);
            const size_t B = (m + 63) / 64;
            peq.assign(256 * std::max<size_t>(B, 1), 0);
            pv.resize(B + 1); mv.resize(B + 1);
            for (uint32_t r = 0; r < m; ++r) peq[size_t(bytes[off[i] + r]) * B + (r >> 6)] |= uint64_t(1) << (r & 63);
            for (size_t j = i + 1; j < N; ++j) {
                const uint32_t n = uint32_t(off[j + 1] - off[j]);
                sum += myers(peq, B, m, &bytes[off[j]], n, pv, mv);
                ++pairs; cells += (long double)m * n;
            }
        }
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"seconds\": %.6f, \"rows\": %zu, \"pairs\": %llu, \"cells\": %.0Lf, \"sum\": %llu, \"threads\": %d}\n", s, rows.size(),
                (unsigned long long)pairs, cells, (unsigned long long)sum, nt);
    return 0;
}
