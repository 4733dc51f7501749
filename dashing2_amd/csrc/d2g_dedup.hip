// d2g_dedup.hip -- K2f: greedy clustering on the device (gfx950), cmp --greedy T.
//
// Replaces the exhaustive branch of dedup_core (reference src/dedup_core.cpp:262-283) for values that are a NON-DECREASING function of
// the equality count: sketch i, in input order, joins the representative with the largest value (among equal values the smallest
// index) if that value reaches the threshold, and founds a cluster of its own otherwise.  A sketch is compared with REPRESENTATIVES
// only.  The state is assign[N] in device memory, assign[j] == j <=> j is a representative; only those 4 N bytes leave the device.
//
// Rows are taken in bands [a0, a1) of at most DEDUP_MAX_BAND rows, in ascending order on ONE stream (stream order makes the decisions
// of earlier bands visible).  Per band:
//   1. the rectangular walk (d2g_cmp_eqcount_rect_dev: bit-sliced, direct or code-plane sets) writes the counts of rows [a0, a1) x
//      columns [0, a1) -- nothing to the right of the band's own rows is ever read -- into the context's scratch band, row stride a1;
//   2. dedup_best_kernel, one workgroup per row: over the columns j < a0 that are representatives and whose value class reaches
//      min_count, the maximum of key = class << 32 | (0xFFFFFFFF - j): largest class first, then smallest j.  Per wave by cross-lane
//      exchange, then four totals through LDS; one u64 per row, 0 = none.  DEDUP_UNROLL loads in flight per lane, as in K2e;
//   3. dedup_resolve_kernel, ONE workgroup: rows a0 .. a1 - 1 in order.  Thread t owns the band's column a0 + t and keeps its
//      representative flag; for row r the threads t < r reduce the same key over the in-band representatives, the result is combined
//      with the row's key of step 2, EVERY thread takes the same decision from it (thread r sets its flag, thread 0 writes assign),
//      and one barrier per row follows (the wave totals alternate between two LDS rows, so the next row's totals never overwrite
//      what a slower wave still reads).  The counts of later rows do not depend on earlier decisions: they are loaded DEDUP_AHEAD rows
//      ahead.  The loop is bounded by the band; no spinning, no communication between workgroups.
// Bounds: band index < (a1 - a0) * a1 <= the scratch's B * N; keys[r], r < a1 - a0 <= DEDUP_MAX_BAND; assign is read at j < a0 and
// written at [a0, a1) only; a class lookup is clamped to S.
#include "d2g_internal.h"
#include "d2g_k2.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

namespace {

constexpr int DEDUP_THREADS = 256, DEDUP_WAVES = DEDUP_THREADS / 64;
constexpr int DEDUP_UNROLL = 4;                               // loads of a row in flight per lane (dedup_best_kernel)
constexpr int DEDUP_AHEAD = 4;                                // rows whose in-band counts are in flight (dedup_resolve_kernel)
constexpr size_t DEDUP_MAX_BAND = DEDUP_THREADS;              // the in-order step is sequential in the band: one column per thread
constexpr size_t DEDUP_BAND_BYTES = (size_t)64 << 20;         // the band of K2e

struct DedupArgs {
    const uint32_t *band;       // [a1 - a0][a1] equality counts
    uint32_t a0, a1, S, min_count;
    const uint32_t *cls;        // [S + 1] or null = identity
    uint32_t *assign;           // [N]
    unsigned long long *keys;   // [a1 - a0]: best key over the columns j < a0; null in the resolve step = no such columns
};

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int o = 32; o; o >>= 1) { const unsigned long long x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    return v;
}

// key of column j with count c, 0 if it does not qualify (the caller has checked that j is a representative)
__device__ __forceinline__ unsigned long long dedup_key(const DedupArgs &a, uint32_t c, uint32_t j) {
    if (c < a.min_count) return 0ull;                         // cls[c] <= c: below min_count the class is too
    const uint32_t cl = a.cls ? a.cls[c < a.S ? c : a.S] : c;
    return cl >= a.min_count ? ((unsigned long long)cl << 32 | (0xFFFFFFFFu - j)) : 0ull;
}

__global__ __launch_bounds__(DEDUP_THREADS) void dedup_best_kernel(DedupArgs a) {
    __shared__ unsigned long long wtot[DEDUP_WAVES];
    const uint32_t tid = threadIdx.x;
    const uint32_t *__restrict__ row = a.band + (size_t)blockIdx.x * a.a1;
    const uint32_t *__restrict__ assign = a.assign;
    unsigned long long best = 0;
    for (uint32_t jb = tid; jb < a.a0; jb += DEDUP_UNROLL * DEDUP_THREADS) {
        uint32_t c[DEDUP_UNROLL], rep[DEDUP_UNROLL];
#pragma unroll
        for (int u = 0; u < DEDUP_UNROLL; ++u) {
            const uint32_t j = jb + u * DEDUP_THREADS;
            c[u] = j < a.a0 ? row[j] : 0u;
            rep[u] = j < a.a0 ? assign[j] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < DEDUP_UNROLL; ++u) {
            const uint32_t j = jb + u * DEDUP_THREADS;
            if (j < a.a0 && rep[u] == j) { const unsigned long long k = dedup_key(a, c[u], j); best = k > best ? k : best; }
        }
    }
    best = wave_max(best);
    if ((tid & 63u) == 0) wtot[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DEDUP_WAVES; ++w) best = wtot[w] > best ? wtot[w] : best;
        a.keys[blockIdx.x] = best;
    }
}

__global__ __launch_bounds__(DEDUP_THREADS) void dedup_resolve_kernel(DedupArgs a) {
    __shared__ unsigned long long wtot[2][DEDUP_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t nrows = a.a1 - a.a0;                      // <= DEDUP_MAX_BAND (checked by the launcher)
    const uint32_t *__restrict__ col = a.band + a.a0 + tid;  // this thread's column, row r at col[r * a1]; read only where tid < r < nrows
    bool isrep = false;                                       // of row a0 + tid, once it is decided
    uint32_t c[DEDUP_AHEAD];
    unsigned long long old[DEDUP_AHEAD];
#pragma unroll
    for (int p = 0; p < DEDUP_AHEAD; ++p) {
        const uint32_t r = (uint32_t)p;
        c[p] = (r < nrows && tid < r) ? col[(size_t)r * a.a1] : 0u;
        old[p] = (r < nrows && a.keys) ? a.keys[r] : 0ull;
    }
    for (uint32_t rb = 0; rb < nrows; rb += DEDUP_AHEAD) {
#pragma unroll
        for (int p = 0; p < DEDUP_AHEAD; ++p) {
            const uint32_t r = rb + p;
            if (r >= nrows) break;                            // uniform
            const uint32_t cur = c[p];
            const unsigned long long oldbest = old[p];
            const uint32_t rn = r + DEDUP_AHEAD;              // the loads of a later row: independent of this row's decision
            c[p] = (rn < nrows && tid < rn) ? col[(size_t)rn * a.a1] : 0u;
            old[p] = (rn < nrows && a.keys) ? a.keys[rn] : 0ull;
            if (wave * 64u < r) {                             // (wave-uniform) this wave owns columns in front of row r
                unsigned long long k = (tid < r && isrep) ? dedup_key(a, cur, a.a0 + tid) : 0ull;
                k = wave_max(k);
                if ((tid & 63u) == 0) wtot[r & 1u][wave] = k;
            } else if ((tid & 63u) == 0) wtot[r & 1u][wave] = 0ull;
            __syncthreads();
            unsigned long long m = oldbest;
#pragma unroll
            for (int w = 0; w < DEDUP_WAVES; ++w) { const unsigned long long x = wtot[r & 1u][w]; m = x > m ? x : m; }
            if (tid == r) isrep = m == 0ull;
            if (tid == 0) a.assign[a.a0 + r] = m ? 0xFFFFFFFFu - (uint32_t)m : a.a0 + r;
        }
    }
}

}  // namespace

extern "C" {

int d2g_cmp_dedup_dev(d2g_ctx *ctx, const d2g_cmp_set *set, uint32_t min_count, const uint32_t *cls_dev, uint32_t *assign_dev,
                      size_t band_rows, void *stream) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set && set->ctx == ctx, "dedup: set belongs to another context");
    D2G_CHECK(ctx, set->N < (1ull << 31) && set->S < (1ull << 31), "dedup: shape too large");
    const size_t N = set->N;
    if (!N) return D2G_OK;
    D2G_CHECK(ctx, assign_dev != nullptr, "dedup: null assignment");
    size_t B = band_rows;
    if (!B) B = std::max<size_t>(32, DEDUP_BAND_BYTES / (4 * N) / 32 * 32);
    B = std::min(std::min(B, DEDUP_MAX_BAND), N);
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->knn_band.grow(ctx, B * N, 0, "dedup band alloc")) return rc;
    if (int rc = ctx->dedup_keys.grow(ctx, DEDUP_MAX_BAND, 0, "dedup keys alloc")) return rc;
    const hipStream_t s = as_stream(stream);
    for (size_t a0 = 0; a0 < N; a0 += B) {
        const size_t a1 = std::min(a0 + B, N);
        if (int rc = d2g_cmp_eqcount_rect_dev(ctx, set, a0, a1, 0, a1, ctx->knn_band, stream)) return rc;
        DedupArgs a;
        a.band = ctx->knn_band; a.a0 = (uint32_t)a0; a.a1 = (uint32_t)a1; a.S = (uint32_t)set->S; a.min_count = min_count;
        a.cls = cls_dev; a.assign = assign_dev; a.keys = a0 ? ctx->dedup_keys.get() : nullptr;
        if (a0) {
            d2g_timer tm(ctx, &ctx->ev_dedup, s);
            hipLaunchKernelGGL(dedup_best_kernel, dim3((unsigned)(a1 - a0)), dim3(DEDUP_THREADS), 0, s, a);
            tm.stop();
            D2G_HIP(ctx, hipGetLastError());
        }
        d2g_timer tm(ctx, &ctx->ev_dedup_resolve, s);
        hipLaunchKernelGGL(dedup_resolve_kernel, dim3(1), dim3(DEDUP_THREADS), 0, s, a);
        tm.stop();
        D2G_HIP(ctx, hipGetLastError());
    }
    return D2G_OK;
}

int d2g_cmp_set_dedup(d2g_ctx *ctx, const d2g_cmp_set *set, const float *lut, double threshold, size_t band_rows, uint32_t *assign_out) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set && set->ctx == ctx, "dedup: set belongs to another context");
    D2G_CHECK(ctx, lut != nullptr, "dedup: null table");
    const size_t N = set->N, S = set->S;
    for (size_t e = 0; e < S; ++e) D2G_CHECK(ctx, lut[e + 1] >= lut[e], "dedup: the value table is not non-decreasing in the equality count");
    if (!N) return D2G_OK;
    D2G_CHECK(ctx, assign_out != nullptr, "dedup: null assignment");
    const float simt = (float)(threshold > 0. ? threshold : 0.9);            // dedup_core.cpp:264
    std::vector<uint32_t> cls(S + 1, 0);
    for (size_t e = 1; e <= S; ++e) cls[e] = lut[e] == lut[e - 1] ? cls[e - 1] : (uint32_t)e;
    uint32_t min_count = 0;
    while (min_count <= S && !(lut[min_count] >= simt)) ++min_count;          // joins unless v < simt (:276), a float comparison
    d2g_dev<uint32_t> d_cls, d_assign;
    int rc;
    if ((rc = d_cls.alloc(ctx, S + 1, "dedup class table alloc")) || (rc = d_assign.alloc(ctx, N, "dedup assignment alloc"))) return rc;
    D2G_HIP(ctx, hipMemcpy(d_cls, cls.data(), (S + 1) * 4, hipMemcpyHostToDevice));
    if ((rc = d2g_cmp_dedup_dev(ctx, set, min_count, d_cls, d_assign, band_rows, nullptr))) return rc;
    D2G_HIP(ctx, hipMemcpy(assign_out, d_assign, N * 4, hipMemcpyDeviceToHost));
    return D2G_OK;
}

int d2g_cmp_dedup(d2g_ctx *ctx, const uint64_t *sig_bits, size_t N, size_t S, int measure, int k, int multiset_space, int algo,
                  double threshold, size_t band_rows, uint32_t *assign_out) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, measure >= D2G_SIMILARITY && measure <= D2G_UNION_SIZE, "dedup: unknown measure");
    D2G_CHECK(ctx, S >= 1, "dedup: empty sketches");
    if (measure == D2G_POISSON_LLR) {
        ctx->last_error = "dedup: with a distance the reference founds a new cluster when the nearest representative is CLOSER than the threshold (SURVEY F13); distances are not clustered";
        return D2G_ERR_UNSUPPORTED;
    }
    std::vector<float> lut(S + 1);
    if (d2g_epilogue_lut(S, measure, k, multiset_space, lut.data()) != D2G_OK) {
        ctx->last_error = "dedup: the value is not a function of the equality count alone (cardinality-dependent measure, or a sketch size that is not a power of two in set space)";
        return D2G_ERR_UNSUPPORTED;
    }
    if (!N) return D2G_OK;
    d2g_cmp_set *set = nullptr;
    if (int rc = d2g_cmp_set_create(ctx, sig_bits, N, S, algo, &set)) return rc;
    const std::unique_ptr<d2g_cmp_set, void (*)(d2g_cmp_set *)> set_owner(set, d2g_cmp_set_destroy);
    return d2g_cmp_set_dedup(ctx, set, lut.data(), threshold, band_rows, assign_out);
}

}  // extern "C"

void d2g_warm_dedup() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&dedup_best_kernel)); }
