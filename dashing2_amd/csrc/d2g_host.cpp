// d2g_host.cpp -- x86 host half of libd2g, first of three files: version and status strings, the Wang hashes, the O(S) scalar
// arithmetic that must stay on the host to be bit-exact with the reference (x87 long double: OPH finalisation, densify), the
// triangle arithmetic, the host ranking behind a screen, the argument checkers of d2g_kset and d2g_seqset, and the CSR finishers
// of --topk and --greedy.  Counts -> values is d2g_epilogue.cpp, the FASTX ingest d2g_seqpack.cpp.  Compiled with g++ (not hipcc)
// so that `long double` is the 80-bit x87 type the reference's gcc build uses.
//
// Reference lines restated here are cited per function.
#include "../../include/d2g.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <utility>
#include <vector>
#ifdef _OPENMP
#include <parallel/algorithm>
#endif

// K1s (d2g_screen.hip), the host work of d2g_screen_create, here because this file is built with OpenMP: the distinct keys of a database
// in ascending order, their raw k-mers (WangInverse(key) ^ xormask) and, for every database position, the rank of its key among them
void d2g_screen_rank_keys(const uint64_t *keys, size_t n, uint64_t xormask, std::vector<uint64_t> &distinct, std::vector<uint64_t> &raw,
                          std::vector<uint32_t> &rank) {
    distinct.assign(keys, keys + n);
#ifdef _OPENMP
    __gnu_parallel::sort(distinct.begin(), distinct.end());
#else
    std::sort(distinct.begin(), distinct.end());
#endif
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    distinct.shrink_to_fit();
    raw.resize(distinct.size());
    rank.resize(n);
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < distinct.size(); ++i) raw[i] = d2g_wang_hash_inverse(distinct[i]) ^ xormask;
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; ++i) rank[i] = (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), keys[i]) - distinct.begin());
}

extern "C" {

int d2g_version(void) { return D2G_VERSION_MAJOR * 1000 + D2G_VERSION_MINOR; }

const char *d2g_strerror(int st) {
    switch (st) {
        case D2G_OK: return "ok";
        case D2G_ERR_INVALID: return "invalid argument";
        case D2G_ERR_NODEVICE: return "no usable HIP (gfx950) device";
        case D2G_ERR_HIP: return "HIP runtime error";
        case D2G_ERR_NOMEM: return "out of memory";
        case D2G_ERR_UNSUPPORTED: return "unsupported configuration for the MI355X hot path";
        case D2G_ERR_IO: return "I/O error";
        case D2G_ERR_INTERNAL: return "internal invariant failed";
        default: return "unknown d2g status";
    }
}

// sketch::hash::WangHash::hash (absent third-party source; Thomas Wang's published 64-bit mix).
// Reference call sites: enums.h:138 (maskfn), oph.h:49 (BHasher).
uint64_t d2g_wang_hash(uint64_t k) {
    k = ~k + (k << 21);
    k ^= k >> 24;
    k = k + (k << 3) + (k << 8);
    k ^= k >> 14;
    k = k + (k << 2) + (k << 4);
    k ^= k >> 28;
    k += k << 31;
    return k;
}

// sketch::hash::WangHash::inverse (absent third-party source): the steps of the mix above undone from the last to the first.
// y = x + (x << s) and y = ~x + (x << s) are undone s more low bits per substitution, y = x ^ (x >> s) s more high bits; the
// multiplications by 21 = 1 + 4 + 16 and 265 = 1 + 8 + 256 by their inverses modulo 2^64.
uint64_t d2g_wang_hash_inverse(uint64_t k) {
    uint64_t t;
    t = k - (k << 31); t = k - (t << 31); k = k - (t << 31);                              // k += k << 31
    t = k ^ (k >> 28); t = k ^ (t >> 28); k = k ^ (t >> 28);                              // k ^= k >> 28
    k *= 0xcf3cf3cf3cf3cf3dull;                                                          // k *= 21
    t = k; for (int i = 0; i < 4; ++i) t = k ^ (t >> 14); k = t;                          // k ^= k >> 14
    k *= 0xd38ff08b1c03dd39ull;                                                          // k *= 265
    t = k ^ (k >> 24); t = k ^ (t >> 24); k = k ^ (t >> 24);                              // k ^= k >> 24
    t = ~k; for (int i = 0; i < 3; ++i) t = ~(k - (t << 21)); k = t;                      // k = ~k + (k << 21)
    return k;
}

// enums.cpp:133-139
uint64_t d2g_seed_mask(uint64_t seedseed) { return seedseed ? d2g_wang_hash(seedseed) : 0; }

// oph.h:59 seed_ = std::mt19937_64(x)(), oph.h:142 x = 0x321b919a61cb41f7, oph.h:46 CEIXOR constant
uint64_t d2g_oph_xor_const(void) {
    static const uint64_t c = std::mt19937_64(0x321b919a61cb41f7ull)() ^ 0x533f8c2151b20f97ull;
    return c;
}

size_t d2g_oph_m(size_t S) { return S + (S & 1); }   // oph.h:143-146

// ids(), oph.h:264-271 with decode = DHasher::inverse (oph.h:50-52,81-83); the first S of every m (fastxsketch.cpp:619-620)
int d2g_oph_kmer_ids(const uint64_t *regs, size_t n, size_t m, size_t S, uint64_t *ids_out) {
    if (S > m || (n && S && (!regs || !ids_out))) return D2G_ERR_INVALID;
    const uint64_t c = d2g_oph_xor_const();
    for (size_t i = 0; i < n; ++i)
        for (size_t r = 0; r < S; ++r) ids_out[i * S + r] = c ^ d2g_wang_hash_inverse(regs[i * m + r]);
    return D2G_OK;
}

// oph.h:240-247
double d2g_oph_card(const uint64_t *regs, size_t m) {
    long double sum = 0.L;
    for (size_t i = 0; i < m; ++i) sum += regs[i] * 0x1p-64L;
    if (!sum) return std::numeric_limits<double>::infinity();
    return m * (m / sum);
}

// oph.h:248-263
int d2g_oph_signatures(const uint64_t *regs, size_t m, double *sig) {
    if (!regs || !sig) return D2G_ERR_INVALID;
    constexpr uint64_t MAXV = std::numeric_limits<uint64_t>::max();
    const size_t nmax = std::count(regs, regs + m, MAXV);
    const long double mul = -double(1) / (m - nmax);          // double division, then widened
    for (size_t i = 0; i < m; ++i) {
        const uint64_t x = regs[i];
        sig[i] = (x == MAXV || x == 0) ? 0. : double(mul * std::log(0x1p-64L * (MAXV - x + 1)));
    }
    return D2G_OK;
}

int d2g_oph_finalize(const uint64_t *regs, size_t n, size_t m, size_t S, double *sigs, double *cards, int nthreads) {
    if (!regs || !sigs || !cards || S > m) return D2G_ERR_INVALID;
    if (nthreads < 1) nthreads = 1;
#ifdef _OPENMP
    #pragma omp parallel num_threads(nthreads)
#endif
    {
        std::vector<double> tmp(m);
#ifdef _OPENMP
        #pragma omp for schedule(static)
#endif
        for (size_t g = 0; g < n; ++g) {
            const uint64_t *r = regs + g * m;
            cards[g] = d2g_oph_card(r, m);                      // fastxsketch.cpp:567
            d2g_oph_signatures(r, m, tmp.data());               // fastxsketch.cpp:586
            std::memcpy(sigs + g * S, tmp.data(), S * sizeof(double));  // :605,:610 (first S only)
        }
    }
    return D2G_OK;
}

// ssi.h:26-36 (in-tree twin of wy::wyhash64_stateless used at cmp_core.cpp:597)
static inline uint64_t wyhash64_stateless(uint64_t *seed) {
    *seed += 0x60bee2bee120fc15ull;
    __uint128_t l = *seed ^ 0xe7037ed1a0b428dbull;
    l *= *seed;
    return uint64_t(l ^ (l >> 64));
}

// cmp_core.cpp:577-613
static size_t densify_one(double *sig, size_t S, std::vector<double> &tmp) {
    if (size_t(std::count(sig, sig + S, 0.)) == S) return S;
    size_t ne = 0;
    tmp.assign(sig, sig + S);
    for (size_t i = 0; i < S; ++i) {
        if (sig[i] != 0.) continue;
        ++ne;
        uint64_t rng = i + 0x5bf2b8bdf07c06cull, j;
        do j = wyhash64_stateless(&rng) % S; while (sig[j] == 0.);
        tmp[i] = sig[j];
    }
    std::copy(tmp.begin(), tmp.end(), sig);
    return ne;
}

int d2g_densify(double *sigs, size_t n, size_t S, size_t *nfilled, int nthreads) {
    if (!sigs || !S) return D2G_ERR_INVALID;
    if (nthreads < 1) nthreads = 1;
    size_t total = 0;
#ifdef _OPENMP
    #pragma omp parallel num_threads(nthreads) reduction(+:total)
#endif
    {
        std::vector<double> tmp;
#ifdef _OPENMP
        #pragma omp for schedule(dynamic, 32)                   // cmp_core.cpp:707
#endif
        for (size_t i = 0; i < n; ++i) total += densify_one(sigs + i * S, S, tmp);
    }
    if (nfilled) *nfilled = total;
    return D2G_OK;
}

// what d2g_kset_create asks of host arrays before anything reaches a device: the pair kernel's searches and its slice table are
// only right over strictly ascending keys
int d2g_kset_check(const uint64_t *keys, const uint32_t *counts, const uint64_t *set_off, size_t nsets, char *err, size_t errcap) {
    auto fail = [&](const char *fmt, unsigned long long a, unsigned long long b) {
        if (err && errcap) std::snprintf(err, errcap, fmt, a, b);
        return (int)D2G_ERR_INVALID;
    };
    auto fail0 = [&](const char *msg) {
        if (err && errcap) std::snprintf(err, errcap, "%s", msg);
        return (int)D2G_ERR_INVALID;
    };
    if (!set_off) return fail0("d2g_kset: null set_off");
    for (size_t i = 0; i < nsets; ++i)
        if (set_off[i + 1] < set_off[i]) return fail("d2g_kset: set_off decreases at set %llu (to %llu)", i, set_off[i + 1]);
    if (nsets && set_off[nsets] > set_off[0] && !keys) return fail0("d2g_kset: null keys");
    for (size_t i = 0; i < nsets; ++i)
        for (uint64_t e = set_off[i]; e < set_off[i + 1]; ++e) {
            if (e > set_off[i] && keys[e] <= keys[e - 1])
                return fail(keys[e] == keys[e - 1] ? "d2g_kset: set %llu holds a key twice (entry %llu): keys must be strictly ascending"
                                                   : "d2g_kset: set %llu is not sorted (entry %llu): keys must be strictly ascending",
                            i, e - set_off[i]);
            if (counts && counts[e] == 0) return fail("d2g_kset: set %llu has a count of 0 (entry %llu)", i, e - set_off[i]);
        }
    return D2G_OK;
}

// K1s: slots of a screen's table = the power of two >= 2 D, >= 16.  The probe numbers slots in a uint32 where ~0 means "not in the
// table" and `slots` itself names the all-ones k-mer behind them (d2g_filter_find, d2g_kmers.h): both need slots <= 2^31, D <= 2^30.
int d2g_screen_table_slots(uint64_t ndistinct, uint64_t *slots) {
    if (!slots) return D2G_ERR_INVALID;
    *slots = 0;
    if (ndistinct > D2G_SCREEN_MAX_KEYS) return D2G_ERR_UNSUPPORTED;
    uint64_t s = 16;
    while (s < 2 * ndistinct) s <<= 1;
    *slots = s;
    return D2G_OK;
}

size_t d2g_ut_count(size_t N, size_t r0, size_t r1) {
    if (r1 > N) r1 = N;
    if (r0 >= r1) return 0;
    // sum_{r=r0}^{r1-1} (N-1-r)
    const size_t n = r1 - r0;
    const size_t tri1 = r1 * (r1 - 1) / 2, tri0 = r0 ? r0 * (r0 - 1) / 2 : 0;
    return n * (N - 1) - (tri1 - tri0);
}

int d2g_ut_partition(size_t N, int nparts, size_t *bounds) {
    if (nparts < 1 || !bounds) return D2G_ERR_INVALID;
    const long double total = N ? (long double)N * (N - 1) / 2 : 0;
    bounds[0] = 0;
    size_t r = 0;
    for (int p = 1; p < nparts; ++p) {
        const long double target = total * p / nparts;
        // pairs in rows [0,r) = r*(N-1) - r(r-1)/2 ; advance to the first r reaching the target
        while (r < N && (long double)r * (N - 1) - (long double)r * (r - 1) / 2 < target) ++r;
        bounds[p] = r;
    }
    bounds[nparts] = N;
    return D2G_OK;
}

// candidate lists of the selection kernel -> CSR in the order of the reference's neighbour lists: std::sort of (mult * value, id)
// pairs (src/index_build.h:16 pqueue::sort, mult = -1 for similarities: index_build.cpp:184), then the sign flip of
// src/cmp_core.cpp:787-793 -- the values written are the plain table entries.
int d2g_knn_finish(const uint32_t *rowcnt, const uint32_t *ids, const uint32_t *counts, size_t nrows, size_t cap, const float *lut,
                   size_t S, int isdist, uint64_t *indptr, uint32_t *indices, float *data, size_t out_cap, size_t *nnz_needed,
                   size_t *overflow_rows) {
    if (!indptr || !lut || (nrows && !rowcnt)) return D2G_ERR_INVALID;
    size_t over = 0, nnz = 0;
    for (size_t i = 0; i < nrows; ++i) { over += rowcnt[i] > cap; nnz += rowcnt[i]; }
    if (overflow_rows) *overflow_rows = over;
    if (over) return D2G_ERR_INVALID;
    if (nnz && (!ids || !counts)) return D2G_ERR_INVALID;
    for (size_t i = 0; i < nrows; ++i)
        for (size_t e = 0; e < rowcnt[i]; ++e) if (counts[i * cap + e] > S) return D2G_ERR_INVALID;
    indptr[0] = 0;
    for (size_t i = 0; i < nrows; ++i) indptr[i + 1] = indptr[i] + rowcnt[i];
    if (nnz_needed) *nnz_needed = nnz;
    if (nnz > out_cap) return D2G_ERR_NOMEM;
    if (nnz && (!indices || !data)) return D2G_ERR_INVALID;
    const float mult = isdist ? 1.f : -1.f;
    std::vector<std::pair<float, uint32_t>> row;
    for (size_t i = 0; i < nrows; ++i) {
        const size_t n = rowcnt[i];
        row.resize(n);
        for (size_t e = 0; e < n; ++e) row[e] = {mult * lut[counts[i * cap + e]], ids[i * cap + e]};
        std::sort(row.begin(), row.end());
        uint32_t *oi = indices + indptr[i];
        float *od = data + indptr[i];
        for (size_t e = 0; e < n; ++e) { oi[e] = row[e].second; od[e] = mult * row[e].first; }
    }
    return D2G_OK;
}

// assign[] of the greedy clustering -> dedup_core's (ids, constituents) as one CSR: clusters in creation order, which is the
// ascending order of their representatives (a representative is the first sketch of its cluster in input order)
int d2g_dedup_clusters(const uint32_t *assign, size_t N, uint64_t *indptr, uint32_t *indices, size_t *nclusters) {
    if (!indptr || !nclusters || (N && (!assign || !indices))) return D2G_ERR_INVALID;
    for (size_t i = 0; i < N; ++i)
        if (assign[i] > i || assign[assign[i]] != assign[i]) return D2G_ERR_INVALID;
    std::vector<uint32_t> cid(N);                             // cluster of a representative; then the next free slot of a cluster
    size_t C = 0;
    for (size_t i = 0; i < N; ++i) if (assign[i] == i) cid[i] = (uint32_t)C++;
    std::vector<uint64_t> fill(C + 1, 0);
    for (size_t i = 0; i < N; ++i) ++fill[cid[assign[i]] + 1];
    indptr[0] = 0;
    for (size_t c = 0; c < C; ++c) { indptr[c + 1] = indptr[c] + fill[c + 1]; fill[c] = indptr[c]; }
    for (size_t i = 0; i < N; ++i) indices[fill[cid[assign[i]]]++] = (uint32_t)i;     // in input order: the representative comes first
    *nclusters = C;
    return D2G_OK;
}

// K2h: what d2g_seqset_create asks of host arrays before anything reaches a device: the pair kernel indexes by these offsets without checks
int d2g_seqset_check(const uint8_t *bytes, const uint64_t *off, size_t nrec, uint64_t nbytes, char *err, size_t errcap) {
    auto fail = [&](int rc, const char *fmt, unsigned long long a, unsigned long long b) {
        if (err && errcap) std::snprintf(err, errcap, fmt, a, b);
        return rc;
    };
    if (!off) return fail(D2G_ERR_INVALID, "d2g_seqset: null off", 0, 0);
    if (nbytes && !bytes) return fail(D2G_ERR_INVALID, "d2g_seqset: null bytes", 0, 0);
    if (off[0] != 0) return fail(D2G_ERR_INVALID, "d2g_seqset: off must begin at 0 (it begins at %llu)", off[0], 0);
    for (size_t i = 0; i < nrec; ++i)
        if (off[i + 1] < off[i]) return fail(D2G_ERR_INVALID, "d2g_seqset: off decreases at record %llu (to %llu)", i, off[i + 1]);
    if (off[nrec] != nbytes) return fail(D2G_ERR_INVALID, "d2g_seqset: off ends at %llu, the records have %llu bytes", off[nrec], nbytes);
    for (size_t i = 0; i < nrec; ++i)
        if (off[i + 1] - off[i] > D2G_EDIT_MAX_LEN)
            return fail(D2G_ERR_UNSUPPORTED, "d2g_seqset: record %llu has %llu symbols, more than D2G_EDIT_MAX_LEN = 65535", i, off[i + 1] - off[i]);
    return D2G_OK;
}
int d2g_seqset_recode_map(const uint8_t *bytes, uint64_t nbytes, uint8_t map[256]) {
    bool seen[256] = {};
    for (uint64_t e = 0; e < nbytes; ++e) seen[bytes[e]] = true;
    int sigma = 0;
    for (int b = 0; b < 256; ++b) map[b] = seen[b] ? uint8_t(sigma++) : uint8_t(0);
    return std::max(sigma, 1);
}

}  // extern "C"
