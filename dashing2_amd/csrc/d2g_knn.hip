// d2g_knn.hip -- K2e: nearest neighbours selected on the device (gfx950).
//
// Replaces build_exact_graph (reference src/index_build.cpp:166-228) for values that are a monotone function of the equality count:
// top-K and threshold both become "list every j != i with neq(i, j) >= t_i" (include/d2g.h).  Only the listed neighbours cross PCIe.
//
// Per band of B rows: the existing rectangular walk (d2g_cmp_eqcount_rect_dev: bit-sliced, direct or code-plane sets) writes the
// B x N counts into a scratch band of the context, then knn_select_kernel runs ONE workgroup per row:
//   (a) top-K only: t_i = the K-th largest eligible count.  S <= KNN_HIST_S: a histogram of the row in LDS (LDS atomics; the count 0,
//       which most columns of a real matrix hold, is summed in a register and added once), scanned from the top by 256 threads.
//       Larger S: bisection on the count, one counting pass over the row per step (at most log2(S) + 1 passes).
//       t_i is then lowered to the minimum of its value class (cls), so that a tie class spanning several counts stays whole.
//   (b) an order-preserving compaction.  Each of the four waves owns one contiguous quarter of the row: a counting pass (wave ballot
//       + popcount), ONE workgroup barrier for the four totals, then a writing pass in which a lane's slot is the wave's running base
//       + the set bits below it in the ballot.  A row's entries come out in ascending j whatever the schedule: bit-reproducible.
// A row is read two (threshold) or three (top-K, histogram form) times; the band is sized to at most 64 MB so that those reads are
// served by the caches (a row is N * 4 bytes: L2 for the re-reads, the 256 MB memory-side cache for the first) -- an ASSUMPTION of
// the design, not something the counters have been asked about.
// One workgroup per row and a few hundred rows per band leave the latency of a load to the lane: KNN_UNROLL = 4 loads in flight per lane
// took the selection at N = 50 000, S = 1024, K = 10 from 32.7 to 14.0 ms (profiles/knn_time.json has the shipped form).
// Bounds: band index < B * N; a slot is written only at p < cap inside the row's own cap slots; histogram bins are clamped to S.
#include "d2g_internal.h"
#include "d2g_k2.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

namespace {

constexpr int KNN_THREADS = 256, KNN_WAVES = KNN_THREADS / 64;
constexpr int KNN_UNROLL = 4;                               // loads of a row in flight per lane: one workgroup per row and a few hundred rows per band leave the latency to the lane
constexpr uint32_t KNN_HIST_S = 4096;                       // sketch sizes up to this take the LDS histogram (16 KB), larger ones the bisection
constexpr size_t KNN_BAND_BYTES = (size_t)64 << 20;         // default band: well inside the 256 MB memory-side cache

struct KnnArgs {
    const uint32_t *band;       // [rows of this launch][N] equality counts
    uint32_t N, S, K, min_count;
    size_t row0;                // sketch index of the band's first row (the self pair is excluded by index)
    size_t out0;                // ... and its row in the outputs
    const uint32_t *cls;        // [S + 1] or null
    size_t cap;
    uint32_t *rowcnt, *ids, *counts;
};

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// sum over the workgroup, returned to every thread (two barriers; `red` has KNN_WAVES words and is free again on return)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *red) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
    for (int w = 0; w < KNN_WAVES; ++w) s += red[w];
    __syncthreads();
    return s;
}

// columns of the row other than `self` whose count is at least x
__device__ __forceinline__ uint32_t count_at_least(const uint32_t *__restrict__ row, uint32_t N, uint32_t self, uint32_t x, uint32_t *red) {
    uint32_t n = 0;
    for (uint32_t jb = threadIdx.x; jb < N; jb += KNN_UNROLL * KNN_THREADS) {
        uint32_t c[KNN_UNROLL];
#pragma unroll
        for (int u = 0; u < KNN_UNROLL; ++u) { const uint32_t j = jb + u * KNN_THREADS; c[u] = j < N ? row[j] : 0u; }
#pragma unroll
        for (int u = 0; u < KNN_UNROLL; ++u) { const uint32_t j = jb + u * KNN_THREADS; n += (j < N && j != self && c[u] >= x) ? 1u : 0u; }
    }
    return block_sum(n, red);
}

__global__ __launch_bounds__(KNN_THREADS) void knn_select_kernel(KnnArgs a) {
    __shared__ uint32_t hist[KNN_HIST_S + 1];
    __shared__ uint32_t red[KNN_WAVES];
    __shared__ uint32_t wtot[KNN_WAVES];
    __shared__ uint32_t sh_t;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = a.N, S = a.S;
    const uint32_t *__restrict__ row = a.band + (size_t)blockIdx.x * N;
    const size_t self64 = a.row0 + blockIdx.x;
    const uint32_t self = (uint32_t)self64;                  // N < 2^31 (checked by the launcher)
    uint32_t t = a.min_count;
    if (a.K) {
        const uint32_t K = a.K;
        if (S <= KNN_HIST_S) {
            for (uint32_t b = tid; b <= S; b += KNN_THREADS) hist[b] = 0;
            if (tid == 0) sh_t = a.min_count;                // fewer than K eligible columns: all of them
            __syncthreads();
            uint32_t zeros = 0;
            for (uint32_t jb = tid; jb < N; jb += KNN_UNROLL * KNN_THREADS) {
                uint32_t c[KNN_UNROLL];
#pragma unroll
                for (int u = 0; u < KNN_UNROLL; ++u) { const uint32_t j = jb + u * KNN_THREADS; c[u] = j < N ? row[j] : 0u; }
#pragma unroll
                for (int u = 0; u < KNN_UNROLL; ++u) {
                    const uint32_t j = jb + u * KNN_THREADS;
                    if (j >= N || j == self || c[u] < a.min_count) continue;
                    if (c[u] == 0) ++zeros; else atomicAdd(&hist[c[u] < S ? c[u] : S], 1u);
                }
            }
            if (zeros) atomicAdd(&hist[0], zeros);
            __syncthreads();
            // thread k owns the bins [lo, hi) counted from the top: hi = S + 1 - k * per
            const uint32_t nb = S + 1, per = (nb + KNN_THREADS - 1) / KNN_THREADS;
            const int hi = (int)nb - (int)(tid * per), lo = hi - (int)per > 0 ? hi - (int)per : 0;
            uint32_t own = 0;
            for (int b = hi - 1; b >= lo; --b) own += hist[b];
            // exclusive prefix of `own` over the threads: wave scan, then the totals of the waves before
            uint32_t inc = own;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t up = __shfl_up(inc, o, 64); if ((int)lane >= o) inc += up; }
            if (lane == 63) red[wave] = inc;
            __syncthreads();
            uint32_t before = inc - own;
            for (uint32_t w = 0; w < wave; ++w) before += red[w];
            if (before < K && before + own >= K) {           // exactly one thread: the K-th largest lies in its bins
                uint32_t acc = before;
                for (int b = hi - 1; b >= lo; --b) { acc += hist[b]; if (acc >= K) { sh_t = (uint32_t)b; break; } }
            }
            __syncthreads();
            t = sh_t;
        } else if (count_at_least(row, N, self, a.min_count, red) >= K) {
            // largest t in [min_count, S] with at least K columns at or above it
            uint32_t lo = a.min_count, hi = S;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                if (count_at_least(row, N, self, mid, red) >= K) lo = mid; else hi = mid - 1;
            }
            t = lo;
        }
        if (a.cls) { const uint32_t c = a.cls[t < S ? t : S]; t = c > a.min_count ? c : a.min_count; }
    }
    // (b) compaction: wave w owns columns [j0, j1)
    const uint32_t seg = (N + 64u * KNN_WAVES - 1) / (64u * KNN_WAVES) * 64u;
    const uint32_t j0 = wave * seg, j1 = j0 + seg < N ? j0 + seg : N;
    uint32_t mine = 0;
    for (uint32_t base = j0; base < j1; base += 64 * KNN_UNROLL) {
        uint32_t c[KNN_UNROLL];
#pragma unroll
        for (int u = 0; u < KNN_UNROLL; ++u) { const uint32_t j = base + 64 * u + lane; c[u] = j < j1 ? row[j] : 0u; }
#pragma unroll
        for (int u = 0; u < KNN_UNROLL; ++u) {
            const uint32_t j = base + 64 * u + lane;
            mine += (uint32_t)__popcll(__ballot(j < j1 && j != self && c[u] >= t));
        }
    }
    if (lane == 0) wtot[wave] = mine;
    __syncthreads();
    uint32_t pos = 0, total = 0;
    for (uint32_t w = 0; w < KNN_WAVES; ++w) { const uint32_t x = wtot[w]; total += x; if (w < wave) pos += x; }
    const size_t orow = a.out0 + blockIdx.x;
    if (tid == 0) a.rowcnt[orow] = total;
    if (a.cap == 0 || pos >= a.cap) return;                  // (wave-uniform) nothing of this wave's share fits
    uint32_t *__restrict__ oid = a.ids + orow * a.cap, *__restrict__ ocn = a.counts + orow * a.cap;
    for (uint32_t base = j0; base < j1 && pos < a.cap; base += 64 * KNN_UNROLL) {
        uint32_t c[KNN_UNROLL];
#pragma unroll
        for (int u = 0; u < KNN_UNROLL; ++u) { const uint32_t j = base + 64 * u + lane; c[u] = j < j1 ? row[j] : 0u; }
#pragma unroll
        for (int u = 0; u < KNN_UNROLL; ++u) {                 // in column order: a lane's slot = the wave's running base + the listed lanes below it
            const uint32_t j = base + 64 * u + lane;
            const bool q = j < j1 && j != self && c[u] >= t;
            const unsigned long long m = __ballot(q);
            if (q) {
                const size_t p = (size_t)pos + lanes_below(m);
                if (p < a.cap) { oid[p] = j; ocn[p] = c[u]; }
            }
            pos += (uint32_t)__popcll(m);
        }
    }
}

}  // namespace

// knn_select_kernel over a band that somebody else filled (d2g_edit_near.hip: closeness by edit distance): rows [row0, row0 + nrows)
// of `band`, [nrows][N] values in [0, S]; outputs from row out0 on.  The contract of d2g_cmp_knn_dev's selection, logged as "knn".
int d2g_knn_select_band(d2g_ctx *ctx, const uint32_t *band, size_t N, size_t S, size_t K, uint32_t min_count, size_t row0, size_t nrows, size_t out0,
                        size_t cap, uint32_t *rowcnt_dev, uint32_t *ids_dev, uint32_t *counts_dev, hipStream_t s) {
    D2G_CHECK(ctx, N < (1ull << 31) && S < (1ull << 31), "knn: shape too large");
    if (!nrows) return D2G_OK;
    KnnArgs a;
    a.band = band; a.N = (uint32_t)N; a.S = (uint32_t)S;
    a.K = (uint32_t)std::min<size_t>(K, 0xFFFFFFFFu); a.min_count = min_count;
    a.row0 = row0; a.out0 = out0; a.cls = nullptr; a.cap = cap;
    a.rowcnt = rowcnt_dev; a.ids = ids_dev; a.counts = counts_dev;
    d2g_timer tm(ctx, &ctx->ev_knn, s);
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)nrows), dim3(KNN_THREADS), 0, s, a);
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

extern "C" {

int d2g_cmp_knn_dev(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1, size_t K, uint32_t min_count, const uint32_t *cls_dev,
                    size_t cap, uint32_t *rowcnt_dev, uint32_t *ids_dev, uint32_t *counts_dev, size_t band_rows, void *stream) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set && set->ctx == ctx, "knn: set belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= set->N, "knn: row range out of bounds");
    D2G_CHECK(ctx, set->N < (1ull << 31) && set->S < (1ull << 31), "knn: shape too large");
    if (r0 == r1) return D2G_OK;
    D2G_CHECK(ctx, rowcnt_dev != nullptr, "knn: null row counts");
    D2G_CHECK(ctx, cap == 0 || (ids_dev != nullptr && counts_dev != nullptr), "knn: null candidate buffers");
    const size_t N = set->N, rows = r1 - r0;
    size_t B = band_rows;
    if (!B) B = std::max<size_t>(32, KNN_BAND_BYTES / (4 * N) / 32 * 32);
    B = std::min(B, rows);
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->knn_band.grow(ctx, B * N, 0, "knn band alloc")) return rc;
    const hipStream_t s = as_stream(stream);
    for (size_t a0 = r0; a0 < r1; a0 += B) {
        const size_t a1 = std::min(a0 + B, r1);
        if (int rc = d2g_cmp_eqcount_rect_dev(ctx, set, a0, a1, 0, N, ctx->knn_band, stream)) return rc;
        KnnArgs a;
        a.band = ctx->knn_band; a.N = (uint32_t)N; a.S = (uint32_t)set->S;
        a.K = (uint32_t)std::min<size_t>(K, 0xFFFFFFFFu); a.min_count = min_count;
        a.row0 = a0; a.out0 = a0 - r0; a.cls = cls_dev; a.cap = cap;
        a.rowcnt = rowcnt_dev; a.ids = ids_dev; a.counts = counts_dev;
        d2g_timer tm(ctx, &ctx->ev_knn, s);
        hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)(a1 - a0)), dim3(KNN_THREADS), 0, s, a);
        tm.stop();
        D2G_HIP(ctx, hipGetLastError());
    }
    return D2G_OK;
}

int d2g_cmp_set_knn(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1, const float *lut, int isdist, size_t K, double threshold,
                    size_t cap, size_t band_rows, uint64_t *indptr_out, uint32_t *indices_out, float *data_out, size_t out_cap,
                    size_t *nnz_needed) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set && set->ctx == ctx, "knn: set belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= set->N, "knn: row range out of bounds");
    D2G_CHECK(ctx, lut != nullptr && indptr_out != nullptr, "knn: null table / indptr");
    D2G_CHECK(ctx, (K >= 1) != (threshold > 0.), "knn: give either K >= 1 (top-K) or a threshold > 0");
    const size_t N = set->N, S = set->S, rows = r1 - r0;
    for (size_t e = 0; e < S; ++e)
        D2G_CHECK(ctx, isdist ? lut[e + 1] <= lut[e] : lut[e + 1] >= lut[e], "knn: the value table is not monotone in the equality count");
    // value classes, and the smallest count that takes part (top-K) or passes (threshold)
    std::vector<uint32_t> cls(S + 1, 0);
    for (size_t e = 1; e <= S; ++e) cls[e] = lut[e] == lut[e - 1] ? cls[e - 1] : (uint32_t)e;
    uint32_t min_count = 0;
    if (K) { if (!isdist) while (min_count <= S && lut[min_count] == 0.f) ++min_count; }                       // index_build.cpp:194
    else while (min_count <= S && !(isdist ? (double)lut[min_count] <= threshold : (double)lut[min_count] >= threshold)) ++min_count;   // :184-185,211
    indptr_out[0] = 0;
    if (nnz_needed) *nnz_needed = 0;
    if (!rows) return D2G_OK;
    const size_t widest = std::max<size_t>(N - 1, 1);
    if (!cap) cap = K ? std::max(2 * K, K + 32) : 64;
    cap = std::min(cap, widest);
    const size_t slots = ctx->limits.knn_chunk_slots;          // KNN_CHUNK_SLOTS (d2g_limits.h) unless D2G_KNN_CHUNK_SLOTS shrinks it
    const size_t chunk = std::min(rows, std::max<size_t>(1, slots / cap));
    d2g_dev<uint32_t> d_cls, d_cnt, d_ids, d_cts, d_ids2, d_cts2;
    int rc;
    if ((rc = d_cls.alloc(ctx, S + 1, "knn class table alloc")) || (rc = d_cnt.alloc(ctx, chunk, "knn row counts alloc")) ||
        (rc = d_ids.alloc(ctx, chunk * cap, "knn candidates alloc")) || (rc = d_cts.alloc(ctx, chunk * cap, "knn candidates alloc"))) return rc;
    D2G_HIP(ctx, hipMemcpy(d_cls, cls.data(), (S + 1) * 4, hipMemcpyHostToDevice));
    std::vector<uint32_t> h_cnt(chunk), h_ids(chunk * cap), h_cts(chunk * cap), h_cnt2, h_ids2, h_cts2, indices;
    std::vector<float> data;
    std::vector<uint64_t> ip;
    size_t done = 0;                                         // rows finished (indptr_out[0 .. done] written)
    // rows [first, first + n) of candidate lists with `cp` slots each -> appended to the CSR
    auto append = [&](const uint32_t *cnt, const uint32_t *ids, const uint32_t *cts, size_t n, size_t cp) -> int {
        size_t need = 0;
        for (size_t i = 0; i < n; ++i) need += cnt[i];
        const size_t old = indices.size();
        indices.resize(old + need); data.resize(old + need); ip.resize(n + 1);
        const int r = d2g_knn_finish(cnt, ids, cts, n, cp, lut, S, isdist, ip.data(), indices.data() + old, data.data() + old, need, nullptr, nullptr);
        if (r) { ctx->last_error = "knn: finishing the candidate lists failed"; return r; }
        for (size_t i = 0; i < n; ++i) indptr_out[done + i + 1] = old + ip[i + 1];
        done += n;
        return D2G_OK;
    };
    for (size_t c0 = r0; c0 < r1; c0 += chunk) {
        const size_t c1 = std::min(c0 + chunk, r1), n = c1 - c0;
        if ((rc = d2g_cmp_knn_dev(ctx, set, c0, c1, K, min_count, K ? d_cls.get() : nullptr, cap, d_cnt, d_ids, d_cts, band_rows, nullptr))) return rc;
        D2G_HIP(ctx, hipMemcpy(h_cnt.data(), d_cnt, n * 4, hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(h_ids.data(), d_ids, n * cap * 4, hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(h_cts.data(), d_cts, n * cap * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n;) {
            size_t e = i;
            if (h_cnt[i] <= cap) {                           // a run of rows that fit
                while (e < n && h_cnt[e] <= cap) ++e;
                if ((rc = append(h_cnt.data() + i, h_ids.data() + i * cap, h_cts.data() + i * cap, e - i, cap))) return rc;
            } else {                                         // a run of rows that did not: once more, with a cap that fits them
                size_t cap2 = 0;
                while (e < n && h_cnt[e] > cap && (e - i + 1) * std::max<size_t>(cap2, h_cnt[e]) <= std::max<size_t>(slots, h_cnt[i])) { cap2 = std::max<size_t>(cap2, h_cnt[e]); ++e; }
                const size_t m = e - i;
                if ((rc = d_ids2.grow(ctx, m * cap2, 0, "knn candidates alloc")) || (rc = d_cts2.grow(ctx, m * cap2, 0, "knn candidates alloc"))) return rc;
                if ((rc = d2g_cmp_knn_dev(ctx, set, c0 + i, c0 + e, K, min_count, K ? d_cls.get() : nullptr, cap2, d_cnt, d_ids2, d_cts2, band_rows, nullptr))) return rc;
                h_cnt2.resize(m); h_ids2.resize(m * cap2); h_cts2.resize(m * cap2);
                D2G_HIP(ctx, hipMemcpy(h_cnt2.data(), d_cnt, m * 4, hipMemcpyDeviceToHost));
                D2G_HIP(ctx, hipMemcpy(h_ids2.data(), d_ids2, m * cap2 * 4, hipMemcpyDeviceToHost));
                D2G_HIP(ctx, hipMemcpy(h_cts2.data(), d_cts2, m * cap2 * 4, hipMemcpyDeviceToHost));
                if ((rc = append(h_cnt2.data(), h_ids2.data(), h_cts2.data(), m, cap2))) return rc;
            }
            i = e;
        }
    }
    if (nnz_needed) *nnz_needed = indices.size();
    if (indices.size() > out_cap) { ctx->last_error = "knn: the output arrays are too small (see nnz_needed)"; return D2G_ERR_NOMEM; }
    if (!indices.empty()) {
        D2G_CHECK(ctx, indices_out != nullptr && data_out != nullptr, "knn: null output");
        std::memcpy(indices_out, indices.data(), indices.size() * 4);
        std::memcpy(data_out, data.data(), data.size() * 4);
    }
    return D2G_OK;
}

int d2g_cmp_knn(d2g_ctx *ctx, const uint64_t *sig_bits, size_t N, size_t S, size_t r0, size_t r1, int measure, int k, int multiset_space,
                int algo, size_t K, double threshold, size_t cap, size_t band_rows, uint64_t *indptr_out, uint32_t *indices_out,
                float *data_out, size_t out_cap, size_t *nnz_needed) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, measure >= D2G_SIMILARITY && measure <= D2G_UNION_SIZE, "knn: unknown measure");
    D2G_CHECK(ctx, S >= 1 && r0 <= r1 && r1 <= N, "knn: row range out of bounds");
    std::vector<float> lut(S + 1);
    if (d2g_epilogue_lut(S, measure, k, multiset_space, lut.data()) != D2G_OK) {
        ctx->last_error = "knn: the value is not a function of the equality count alone (cardinality-dependent measure, or a sketch size that is not a power of two in set space)";
        return D2G_ERR_UNSUPPORTED;
    }
    d2g_cmp_set *set = nullptr;
    if (int rc = d2g_cmp_set_create(ctx, sig_bits, N, S, algo, &set)) return rc;
    const std::unique_ptr<d2g_cmp_set, void (*)(d2g_cmp_set *)> set_owner(set, d2g_cmp_set_destroy);
    return d2g_cmp_set_knn(ctx, set, r0, r1, lut.data(), measure == D2G_POISSON_LLR, K, threshold, cap, band_rows, indptr_out, indices_out,
                           data_out, out_cap, nnz_needed);
}

}  // extern "C"

void d2g_warm_knn() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&knn_select_kernel)); }
