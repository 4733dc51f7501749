// d2g_edit_near.hip -- K2i: neighbours within a bound T on the edit distance, over a d2g_seqset (gfx950).
//
// Replaces build_exact_graph over compare() with M_EDIT_DISTANCE (reference src/index_build.cpp:166-228): "which records are within T
// edits of this one", "which K are nearest".  The device writes the CLOSENESS c = T + 1 - min(d, T + 1) (include/d2g.h), which K2e's
// selection kernel (d2g_knn.hip, unchanged) reads as it reads equality counts; only the listed neighbours cross PCIe.
//
// edit_near_kernel, the band route (T <= D2G_EDIT_BAND_MAX): the transpose of K2h's decomposition.
//   * ONE WAVE serves one row record as the query and a tile of positions of the set's order by length; the query's match bits
//     Peq[code][word] are built once per tile in LDS, by LDS atomic OR, as K2h's edit_build_peq does; a tile none of whose columns
//     passes the length filter |len_i - len_j| <= T (or whose query is empty) builds no table and only fills;
//   * every LANE takes one column record and runs Hyyro's diagonal-band form of Myers' recurrence over its symbols (Hyyro 2003; Myers,
//     J. ACM 46(3), 1999; the band is Ukkonen's, 1985): the 2T + 1 diagonals around the main one live in the top bits of one 64-bit
//     word pair (VP, VN) that slides down the query by one row per column.  Nothing crosses lanes;
//   * a step reads the 64-bit window of the symbol's table row that begins at bit `start` = column + T - 63: three 32-bit words at
//     start >> 5 and two funnel shifts.  A table row is [2 zero words][W = ceil(m / 32) words][>= 2 zero words], so a window that
//     begins before the query or ends behind it reads zeros, never another row: the word index is start / 32 + 2 in [0, W + 1]
//     (start >= -63; start <= m + 2T - 64 <= m - 2 because a column that passed the filter has at most m + T symbols).  The min() on the
//     index can therefore never act; it is DEFENSIVE ONLY, one VALU a step: it bounds the ADDRESS should the derivation ever be broken by a
//     change, not the value (the shift would then belong to another word).  Likewise `col < n` in the step's condition is implied by
//     `active`, which goes false at col + 1 == n;
//   * all lanes of a step read the SAME word index for DIFFERENT symbols: address = code * stride + word.  The stride is ODD, so up to 32
//     codes fall on 32 different banks (ds_read_b32 banks are dwords mod 32 per half-wave); equal codes are one address, a broadcast;
//   * the score follows the main diagonal while it exists (it cannot decrease there) and the last row afterwards (where it can, by one
//     per column): a lane whose score exceeds brk = 2T + n - m can no longer come back to T and is done with c = 0; the wave leaves a
//     round when all its lanes are done.  The tiles follow the order by length, so the lanes of a round have nearly the same n;
//   * the column's symbols come 16 per load, one load ahead, as in K2h.
// The full route (T above the band, a row whose table does not fit in LDS, or a query of one block whose bound is wide: EDIT_NEAR_FULL_MAX_LEN): K2h's edit_pair_kernel,
// unchanged, over the window of columns that can pass for ANY row of the run, straight into the output, then edit_clamp_kernel in place
// (a column outside the window is decided by the lengths alone and never read).
// Bounds: out index < (r1 - r0) * N; table index < sigma * stride (code < sigma by the recoding, word <= W + 3 < stride); a record's
// codes are read in whole 16-byte chunks below its padded end.
#include "d2g_edit.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

namespace {

// The crossover of the two routes at T <= D2G_EDIT_BAND_MAX, from profiles/edit_within_time.json ("crossover", 10 000 reads a side): a query
// of one 32-row block costs K2h's kernel one lane per pair as well, on 32-bit words (35 VALU a step against the band's 47 on 64-bit
// words), so the band kernel is ahead there only while its early exit bites.  32 symbols, band / full ms: T = 5 2.42 / 2.89, T = 6 2.72 / 2.90,
// T = 7 3.12 / 2.90; 16 symbols: T = 3 1.69 / 1.70, T = 4 1.93 / 1.70.  Rows of at most EDIT_NEAR_FULL_MAX_LEN symbols take the band route
// only while EDIT_NEAR_SHORT_T_FACTOR T is below their length -- or when they have at most EDIT_NEAR_TINY_LEN symbols, where both routes are
// bound by the output and the full route writes it twice (8 symbols: 1.13 .. 1.19 against 1.19 .. 1.20 ms at every T).  Every longer row (33
// and 64 symbols measured, T = 3 .. 31) was ahead on the band at every bound.  That file was written by the library built from THESE
// constants: at each of its 29 points "dispatcher_route" is the faster of the two forced routes.  Change a constant, run the tool again.
constexpr uint32_t EDIT_NEAR_FULL_MAX_LEN = 32;
constexpr uint32_t EDIT_NEAR_SHORT_T_FACTOR = 5;
constexpr uint32_t EDIT_NEAR_TINY_LEN = 8;
constexpr uint32_t EDIT_NEAR_TILE = 512;                    // positions of the order per workgroup (D2G_EDIT_TILE overrides)
constexpr size_t NEAR_BAND_BYTES = (size_t)64 << 20;        // d2g_edit_within_dev's default band, as K2e's

struct NearArgs {
    const uint8_t *codes;
    const uint64_t *doff;
    const uint32_t *len, *order;
    uint32_t N, sigma, T;
    uint32_t row0;                     // first row of this launch
    uint32_t a0;                       // ... and of the output
    uint32_t ntiles, tile, stride;     // stride: odd, >= (the most words of a row of this launch) + 4
    uint32_t *out;
};

__device__ __forceinline__ uint32_t near_wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__device__ __forceinline__ uint32_t near_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

__global__ __launch_bounds__(64) void edit_near_kernel(NearArgs a) {
    extern __shared__ uint32_t near_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = a.row0 + blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t m = a.len[i], T = a.T, W = (m + 31) >> 5, stride = a.stride;
    const uint32_t p0 = tile * a.tile, p1 = min(a.N, p0 + a.tile);
    uint32_t *__restrict__ orow = a.out + (size_t)(i - a.a0) * a.N;
    {   // a tile without a pair for the band builds no table: zeros outside the filter, T + 1 - the other's length beside an empty record
        bool any = false;
        for (uint32_t p = p0 + lane; p < p1; p += 64) { const uint32_t n = a.len[a.order[p]]; any |= m && n && near_absdiff(m, n) <= T; }
        if (!__any(any)) {
            for (uint32_t p = p0 + lane; p < p1; p += 64) {
                const uint32_t j = a.order[p], dl = near_absdiff(m, a.len[j]);
                orow[j] = dl > T ? 0u : T + 1 - dl;
            }
            return;
        }
    }
    const uint8_t *q = a.codes + a.doff[i];
    for (uint32_t e = lane; e < a.sigma * stride; e += 64) near_lds[e] = 0;
    __syncthreads();
    for (uint32_t r = lane; r < m; r += 64) atomicOr(&near_lds[(uint32_t)q[r] * stride + 2 + (r >> 5)], 1u << (r & 31));
    __syncthreads();
    const uint32_t dend = m > T ? m - T : 0;                     // columns [0, dend): the score follows the diagonal; from there on the last row
    for (uint32_t base = p0; base < p1; base += 64) {
        const uint32_t p = base + lane;
        const bool has = p < p1;
        const uint32_t j = has ? a.order[p] : 0u, n = has ? a.len[j] : 0u, dl = near_absdiff(m, n);
        bool active = has && n && dl <= T;
        uint32_t c = has && dl <= T ? T + 1 - dl : 0u;           // final for a lane that does not run (n == 0: d = m)
        uint64_t VP = ~0ull << (63 - T), VN = 0, hor = 1ull << (62 - (T > m ? T - m : 0));
        int start = (int)T - 63, cur = (int)min(T, m);
        const int brk = (int)(2 * T + n) - (int)m;
        const uint32_t nmax = near_wave_max(active ? n : 0u), nchunks = (nmax + 15) / 16, tchunks = (n + 15) / 16;
        const uint4 *t4 = reinterpret_cast<const uint4 *>(a.codes + a.doff[j]);
        uint4 nxt = make_uint4(0, 0, 0, 0);
        if (active) nxt = t4[0];
        for (uint32_t ch = 0; ch < nchunks; ++ch) {
            if (!__any(active)) break;
            const uint4 cw = nxt;
            if (active && ch + 1 < tchunks) nxt = t4[ch + 1];
#pragma unroll
            for (uint32_t u = 0; u < 16; ++u) {
                const uint32_t col = ch * 16 + u;
                const uint32_t w = (u >> 2) == 0 ? cw.x : (u >> 2) == 1 ? cw.y : (u >> 2) == 2 ? cw.z : cw.w;
                if (active && col < n) {
                    const uint32_t sym = (w >> (8 * (u & 3))) & 255u;
                    const uint32_t wi = min((uint32_t)((start >> 5) + 2), W + 1), sh = (uint32_t)start & 31u;
                    const uint32_t *row = near_lds + sym * stride + wi;
                    const uint32_t w0 = row[0], w1 = row[1], w2 = row[2];
                    const uint64_t X = ((uint64_t)__builtin_amdgcn_alignbit(w2, w1, sh) << 32) | __builtin_amdgcn_alignbit(w1, w0, sh);
                    const uint64_t D0 = (((X & VP) + VP) ^ VP) | X | VN;
                    const uint64_t HP = VN | ~(D0 | VP), HN = D0 & VP;
                    if (col < dend) cur += (D0 >> 63) ? 0 : 1;
                    else { cur += ((HP & hor) ? 1 : 0) - ((HN & hor) ? 1 : 0); hor >>= 1; }
                    VP = HN | ~((D0 >> 1) | HP);
                    VN = (D0 >> 1) & HP;
                    ++start;
                    if (cur > brk) { active = false; c = 0; }
                    else if (col + 1 == n) { active = false; c = (uint32_t)cur <= T ? T + 1 - (uint32_t)cur : 0u; }
                }
            }
        }
        if (has) orow[j] = c;
    }
}

// the full route's second half, in place: v = d(i, j) where the lengths let the pair pass (edit_pair_kernel wrote it), anything elsewhere
__global__ __launch_bounds__(256) void edit_clamp_kernel(uint32_t *v, const uint32_t *len, uint32_t row0, uint32_t nrows, uint32_t N, uint32_t T) {
    const size_t total = (size_t)nrows * N;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const uint32_t r = (uint32_t)(e / N), j = (uint32_t)(e - (size_t)r * N);
        const uint32_t dl = near_absdiff(len[row0 + r], len[j]);
        uint32_t c = 0;
        if (dl <= T) { const uint32_t d = v[e]; c = d <= T ? T + 1 - d : 0u; }
        v[e] = c;
    }
}

uint32_t near_stride(uint32_t len) { return (((len + 31) / 32) + 4) | 1u; }

// the route of row i: true = the band kernel
bool near_band_row(const d2g_ctx *ctx, const d2g_seqset *ss, uint32_t i, uint32_t T) {
    if (T > (uint32_t)D2G_EDIT_BAND_MAX || ctx->edit.near_route == 2) return false;
    if ((uint64_t)ss->sigma * near_stride(ss->len[i]) > EDIT_LDS_WORDS) return false;
    return ctx->edit.near_route == 1 || ss->len[i] > EDIT_NEAR_FULL_MAX_LEN || ss->len[i] <= EDIT_NEAR_TINY_LEN || EDIT_NEAR_SHORT_T_FACTOR * T < ss->len[i];
}

}  // namespace

void d2g_warm_edit_near() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&edit_near_kernel));
}

extern "C" {

int d2g_edit_band_max(void) { return D2G_EDIT_BAND_MAX; }

int d2g_edit_near_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, uint32_t T, uint32_t *close_dev, void *stream) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= ss->N, "d2g_edit_near_dev: rows out of range");
    D2G_CHECK(ctx, T < (1u << 31), "d2g_edit_near_dev: the bound must be below 2^31");
    if (r0 == r1) return D2G_OK;
    D2G_CHECK(ctx, close_dev != nullptr, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t s = as_stream(stream);
    const uint32_t N = (uint32_t)ss->N;
    // Maximal runs of CONSECUTIVE rows of one route: a run is one launch (band) or two (pair kernel, clamp) under a timer bracket of its
    // own, with its own window search.  Rows are not regrouped by route (both kernels take a contiguous row range and write contiguous
    // output rows), so a call whose rows alternate between records of 9 .. 32 symbols and longer ones at 5T >= the short length is cut
    // into as many runs as it has rows, each a launch of a few waves: a cliff that is NOT measured.  A set of one kind of record, or one
    // sorted by length, has at most three runs.
    for (uint32_t a0 = (uint32_t)r0; a0 < (uint32_t)r1;) {
        const bool band = near_band_row(ctx, ss, a0, T);
        uint32_t a1 = a0 + 1, lmin = ss->len[a0], lmax = lmin;
        while (a1 < (uint32_t)r1 && near_band_row(ctx, ss, a1, T) == band) { lmin = std::min(lmin, ss->len[a1]); lmax = std::max(lmax, ss->len[a1]); ++a1; }
        uint32_t *out = close_dev + (size_t)(a0 - (uint32_t)r0) * N;
        if (band) {
            NearArgs a{ss->codes, ss->doff, ss->dlen, ss->order, N, ss->sigma, T, a0, a0, 0, 0, near_stride(lmax), out};
            a.tile = ctx->edit.tile > 0 ? (uint32_t)ctx->edit.tile : EDIT_NEAR_TILE;
            a.ntiles = div_up<uint32_t>(N, a.tile);
            const size_t lds = sizeof(uint32_t) * (size_t)ss->sigma * a.stride;
            if (lds > sizeof(uint32_t) * EDIT_LDS_WORDS) { ctx->last_error = "d2g_edit_near: the match table does not fit in LDS"; return D2G_ERR_INTERNAL; }
            const uint32_t rows_per = std::max<uint32_t>(1, ctx->limits.edit_grid_max / a.ntiles);
            d2g_timer tm(ctx, &ctx->ev_editnear, s);
            for (uint32_t r = a0; r < a1; r += rows_per) {
                a.row0 = r;
                hipLaunchKernelGGL(edit_near_kernel, dim3(std::min(rows_per, a1 - r) * a.ntiles), dim3(64), lds, s, a);
            }
            tm.stop();
        } else {
            // the columns that can pass for any row of the run: lengths in [lmin - T, lmax + T], one window of the order
            const uint32_t lo = lmin > T ? lmin - T : 0, hi = (uint32_t)std::min<uint64_t>((uint64_t)lmax + T, 0xFFFFFFFFu);
            const uint32_t p0 = (uint32_t)(std::lower_bound(ss->sorted_len.begin(), ss->sorted_len.end(), lo) - ss->sorted_len.begin());
            const uint32_t p1 = (uint32_t)(std::upper_bound(ss->sorted_len.begin(), ss->sorted_len.end(), hi) - ss->sorted_len.begin());
            if (int rc = d2g_edit_rect_window(ctx, ss, a0, a1, p0, p1, out, s)) return rc;
            const size_t total = (size_t)(a1 - a0) * N;
            d2g_timer tm(ctx, &ctx->ev_editnear, s);
            hipLaunchKernelGGL(edit_clamp_kernel, dim3((unsigned)std::min<size_t>(div_up<size_t>(total, 256), (size_t)ctx->num_cus * 32)), dim3(256), 0, s, out,
                               ss->dlen.get(), a0, a1 - a0, N, T);
            tm.stop();
        }
        D2G_HIP(ctx, hipGetLastError());
        a0 = a1;
    }
    return D2G_OK;
}

int d2g_edit_within_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, size_t K, uint32_t T, size_t cap, uint32_t *rowcnt_dev,
                        uint32_t *ids_dev, uint32_t *close_dev, size_t band_rows, void *stream) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= ss->N, "d2g_edit_within_dev: rows out of range");
    D2G_CHECK(ctx, T < (1u << 31) - 1, "d2g_edit_within_dev: the bound must be below 2^31 - 1");
    if (r0 == r1) return D2G_OK;
    D2G_CHECK(ctx, rowcnt_dev != nullptr, "d2g_edit_within_dev: null row counts");
    D2G_CHECK(ctx, cap == 0 || (ids_dev != nullptr && close_dev != nullptr), "d2g_edit_within_dev: null candidate buffers");
    const size_t N = ss->N, rows = r1 - r0;
    size_t B = band_rows;
    if (!B) B = std::max<size_t>(32, NEAR_BAND_BYTES / (4 * N) / 32 * 32);
    B = std::min(B, rows);
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->knn_band.grow(ctx, B * N, 0, "knn band alloc")) return rc;
    for (size_t a0 = r0; a0 < r1; a0 += B) {
        const size_t a1 = std::min(a0 + B, r1);
        if (int rc = d2g_edit_near_dev(ctx, ss, a0, a1, T, ctx->knn_band, stream)) return rc;
        if (int rc = d2g_knn_select_band(ctx, ctx->knn_band, N, (size_t)T + 1, K, 1, a0, a1 - a0, a0 - r0, cap, rowcnt_dev, ids_dev, close_dev, as_stream(stream))) return rc;
    }
    return D2G_OK;
}

}  // extern "C"

namespace {

// d2g_edit_knn's state: the device buffers every level of the escalation shares (a level has copied its lists to the host before the
// next one runs), the outputs in row order.  Host cost, not measured: every level of the escalation (at most 17: the bound at least
// doubles up to D2G_EDIT_MAX_LEN) holds six host vectors of its chunk, and the whole CSR is assembled here before d2g_edit_knn looks at
// out_cap, as d2g_cmp_set_knn does
struct EditKnn {
    d2g_ctx *ctx = nullptr;
    const d2g_seqset *ss = nullptr;
    size_t K = 0, cap = 0, band_rows = 0;
    d2g_dev<uint32_t> d_cnt, d_ids, d_cls;
    std::vector<uint32_t> indices;
    std::vector<float> data;
    uint64_t *indptr_out = nullptr;
    size_t done = 0;                                         // rows finished (indptr_out[0 .. done] written)

    // n rows of candidate lists with cp slots each, closeness under `bound` -> appended to the CSR as distances
    int append(const uint32_t *cnt, const uint32_t *ids, const uint32_t *cls, size_t n, size_t cp, uint32_t bound) {
        std::vector<float> lut((size_t)bound + 2);
        for (size_t c = 0; c <= (size_t)bound + 1; ++c) lut[c] = (float)((size_t)bound + 1 - c);
        size_t need = 0;
        for (size_t i = 0; i < n; ++i) need += cnt[i];
        const size_t old = indices.size();
        indices.resize(old + need); data.resize(old + need);
        std::vector<uint64_t> ip(n + 1);
        const int r = d2g_knn_finish(cnt, ids, cls, n, cp, lut.data(), (size_t)bound + 1, 1, ip.data(), indices.data() + old, data.data() + old, need, nullptr, nullptr);
        if (r) { ctx->last_error = "d2g_edit_knn: finishing the candidate lists failed"; return r; }
        for (size_t i = 0; i < n; ++i) indptr_out[done + i + 1] = old + ip[i + 1];
        done += n;
        return D2G_OK;
    }

    // the candidate lists of rows [c0, c1) under `bound` with cp slots each -> cnt [n], ids / cls [n][cp] on the host
    int fetch(size_t c0, size_t c1, uint32_t bound, size_t cp, std::vector<uint32_t> &cnt, std::vector<uint32_t> &ids, std::vector<uint32_t> &cls) {
        const size_t n = c1 - c0;
        int rc;
        if ((rc = d_cnt.grow(ctx, n, 0, "edit knn row counts alloc")) || (rc = d_ids.grow(ctx, n * cp, 0, "edit knn candidates alloc")) ||
            (rc = d_cls.grow(ctx, n * cp, 0, "edit knn candidates alloc"))) return rc;
        if ((rc = d2g_edit_within_dev(ctx, ss, c0, c1, K, bound, cp, d_cnt, d_ids, d_cls, band_rows, nullptr))) return rc;
        cnt.resize(n); ids.resize(n * cp); cls.resize(n * cp);
        D2G_HIP(ctx, hipMemcpy(cnt.data(), d_cnt, n * 4, hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(ids.data(), d_ids, n * cp * 4, hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(cls.data(), d_cls, n * cp * 4, hipMemcpyDeviceToHost));
        return D2G_OK;
    }

    // rows [c0, c1) under `bound`, in chunks; top-K: the rows that are short of min(K, N - 1) entries go on with 2 bound + 1
    int run(size_t c0, size_t c1, uint32_t bound) {
        const size_t want = std::min(K, ss->N - 1);
        const size_t slots = ctx->limits.edit_knn_chunk_slots;   // NEAR_CHUNK_SLOTS (d2g_limits.h) unless D2G_EDIT_KNN_CHUNK_SLOTS shrinks it
        const size_t chunk = std::max<size_t>(1, slots / cap);
        std::vector<uint32_t> cnt, ids, cls, cnt2, ids2, cls2;
        for (size_t b0 = c0; b0 < c1; b0 += chunk) {
            const size_t b1 = std::min(b0 + chunk, c1), n = b1 - b0;
            int rc;
            if ((rc = fetch(b0, b1, bound, cap, cnt, ids, cls))) return rc;
            auto kind = [&](size_t i) { return K && cnt[i] < want && bound < ss->maxlen ? 2 : cnt[i] > cap ? 1 : 0; };   // 2: short, 1: overflowed, 0: complete
            for (size_t i = 0; i < n;) {
                const int k = kind(i);
                size_t e = i + 1;
                if (k == 1) {                                    // only the rows that overflowed run again: a run of them whose widest list fits the slot budget
                    size_t cap2 = cnt[i];
                    while (e < n && kind(e) == 1 && (e - i + 1) * std::max<size_t>(cap2, cnt[e]) <= std::max<size_t>(slots, cnt[i])) { cap2 = std::max<size_t>(cap2, cnt[e]); ++e; }
                    if ((rc = fetch(b0 + i, b0 + e, bound, cap2, cnt2, ids2, cls2))) return rc;
                    if ((rc = append(cnt2.data(), ids2.data(), cls2.data(), e - i, cap2, bound))) return rc;
                } else {
                    while (e < n && kind(e) == k) ++e;
                    if (k == 0) { if ((rc = append(cnt.data() + i, ids.data() + i * cap, cls.data() + i * cap, e - i, cap, bound))) return rc; }
                    else if ((rc = run(b0 + i, b0 + e, (uint32_t)std::min<uint64_t>(2ull * bound + 1, ss->maxlen)))) return rc;
                }
                i = e;
            }
        }
        return D2G_OK;
    }
};

}  // namespace

extern "C" int d2g_edit_knn(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, size_t K, uint32_t T, size_t cap, size_t band_rows,
                            uint64_t *indptr_out, uint32_t *indices_out, float *data_out, size_t out_cap, size_t *nnz_needed) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= ss->N, "d2g_edit_knn: row range out of bounds");
    D2G_CHECK(ctx, indptr_out != nullptr, "d2g_edit_knn: null indptr");
    indptr_out[0] = 0;
    if (nnz_needed) *nnz_needed = 0;
    if (r0 == r1) return D2G_OK;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    EditKnn st;
    st.ctx = ctx; st.ss = ss; st.K = K; st.band_rows = band_rows; st.indptr_out = indptr_out;
    st.cap = std::min(cap ? cap : K ? std::max(2 * K, K + 32) : 64, std::max<size_t>(ss->N - 1, 1));
    // no distance exceeds the longest record: a larger bound lists the same records
    if (int rc = st.run(r0, r1, std::min(T, ss->maxlen))) return rc;
    D2G_HIP(ctx, hipStreamSynchronize(nullptr));
    if (nnz_needed) *nnz_needed = st.indices.size();
    if (st.indices.size() > out_cap) { ctx->last_error = "d2g_edit_knn: the output arrays are too small (see nnz_needed)"; return D2G_ERR_NOMEM; }
    if (!st.indices.empty()) {
        D2G_CHECK(ctx, indices_out != nullptr && data_out != nullptr, "d2g_edit_knn: null output");
        std::memcpy(indices_out, st.indices.data(), st.indices.size() * 4);
        std::memcpy(data_out, st.data.data(), st.data.size() * 4);
    }
    return D2G_OK;
}
