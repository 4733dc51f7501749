// d2g_edit_dedup.hip -- K2j: greedy clustering by edit distance over a d2g_seqset (gfx950), d2g_edit_dedup_dev.
//
// The rule (the repository's own; the reference's exhaustive dedup_core is inverted for a distance, F13): record i, in input
// order, joins the representative r < i with the smallest d(i, r), among equal distances the smallest r, if that distance is <= T, and
// founds a cluster otherwise.  In K2i's closeness c = T + 1 - min(d, T + 1) that is K2f's rule with the identity class table and
// min_count = 1: the largest key c << 32 | (0xFFFFFFFF - r) over the representatives wins, 0 = found a cluster.  The state is assign[N]
// in device memory, assign[j] == j <=> j is a representative.
//
// Rows go in bands [a0, a1) of at most EDD_MAX_BAND rows, ascending, on ONE stream.  Per band:
//   1. edit_dedup_count_kernel, edit_dedup_compact_kernel: the set's order by length, compacted under the flag j < a0 && assign[j] == j,
//      into the representative list (its length stays in a device word; the host never reads it).  The order is kept, so a tile of the
//      list holds records of nearly one length and whole tiles fall to the length filter.  Two launches: a count per chunk of the order,
//      then every chunk sums the counts in front of it and writes its part; the second also zeroes the band's keys;
//   2. edit_dedup_list_kernel, the hot path: edit_near_kernel's decomposition (d2g_edit_near.hip: one wave per (band row, tile of a
//      list), the row's Peq in LDS by LDS atomic OR, odd stride, three-word window, one pair per lane in one 64-bit band word, the length
//      filter, the early exit at brk = 2T + n - m, the same values beside empty records) with two changes.  The work items are
//      (row, tile) pairs over a list whose length is a device value: the grid is sized from the CU count and strides over them, and the kernel
//      itself picks the tile, 64 .. 512 positions, from the list's length (edd_tile).  And a
//      tile of the representative list REDUCES: every lane keeps the largest key of its pairs, the wave takes the maximum once per work
//      item, and lane 0 issues one 64-bit atomicMax on keys[row] (a vector atomic); no rows x representatives band reaches memory.  The
//      same launch serves the band's own block in a STORING mode: behind a row's list tiles come the tiles of the list {a0 .. i - 1},
//      whose closeness goes to block[row][column - a0] (only columns in front of the row: the in-order step reads no others);
//   3. rows without a band kernel (T > D2G_EDIT_BAND_MAX, or sigma x stride > 16 384 words; D2G_EDIT_DEDUP_ROUTE=2: every row):
//      d2g_edit_near_dev, unchanged, over each run of such rows x all N columns into the context's scratch band, then
//      edit_dedup_best_kernel, K2f's dedup_best_kernel with a row stride of N: the best key over the representatives j < a0;
//   4. edit_dedup_resolve_kernel, ONE workgroup: K2f's dedup_resolve_kernel, reading a row's in-band closeness from the block (stride
//      EDD_MAX_BAND) or from the scratch band (stride N, column a0 + t) by the row's route.  K2f's kernel has one number for the row
//      stride and the band's end, which neither layout fits; hence a sibling and not a launcher.
// The reduction is exact: max is associative and commutative, every (row, representative) pair is in exactly one tile, and a key holds
// the column's index, so the result does not depend on the list's order (D2G_EDIT_DEDUP_REVERSE=1 writes the list backwards; tests).
// Bounds: list index < *nlist <= a0 <= N (the list has N words); block index < EDD_MAX_BAND^2; keys[r], r < a1 - a0 <= EDD_MAX_BAND;
// table index < sigma * stride as in edit_near_kernel (a row whose own stride would exceed the launch's is an all-columns row and is
// skipped); assign is read at j < a0 and written at [a0, a1); the scratch band at < (a1 - a0) * N.
#include "d2g_edit.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int EDD_THREADS = 256, EDD_WAVES = EDD_THREADS / 64;
constexpr size_t EDD_MAX_BAND = EDD_THREADS;              // the in-order step: one band column per thread
constexpr uint32_t EDD_TILE_MIN = 64, EDD_TILE_MAX = 512; // positions of a list per work item: between these by the list's length (edd_tile; D2G_EDIT_TILE overrides)
constexpr uint32_t EDD_WAVES_PER_CU = 20;                 // the list kernel's grid: one-wave workgroups, five resident per SIMD (86 VGPRs)
static_assert(EDD_THREADS == (int)EDD_THREADS_HOST, "d2g_limits.h rounds a compaction chunk to the workgroup size");   // EDD_CHUNK, EDD_MAX_CHUNKS: d2g_limits.h
constexpr int EDD_UNROLL = 4, EDD_AHEAD = 4;              // as DEDUP_UNROLL, DEDUP_AHEAD of d2g_dedup.hip

__device__ __forceinline__ uint32_t edd_wave_max32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ unsigned long long edd_wave_max(unsigned long long v) {
    for (int o = 32; o; o >>= 1) { const unsigned long long x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    return v;
}
__device__ __forceinline__ uint32_t edd_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
__device__ __forceinline__ unsigned long long edd_key(uint32_t c, uint32_t j) { return c ? ((unsigned long long)c << 32 | (0xFFFFFFFFu - j)) : 0ull; }
// the route of a row of `len` symbols: true = the list kernel (the host's edd_list_row says the same)
__device__ __forceinline__ bool edd_row_fits(uint32_t sigma, uint32_t len) { return sigma * ((((len + 31) >> 5) + 4) | 1u) <= EDIT_LDS_WORDS; }

// ---------------------------------------------------------------- the representative list
struct CompactArgs {
    const uint32_t *order, *assign;
    uint32_t N, a0, chunk, nchunks, reverse;
    uint32_t *cnt;                     // [nchunks]
    uint32_t *list, *nlist;            // [N], [1]
    unsigned long long *keys;          // [EDD_MAX_BAND], zeroed here
};

__device__ __forceinline__ bool edd_is_rep(const CompactArgs &a, uint32_t p) {
    if (p >= a.N) return false;
    const uint32_t j = a.order[p];
    return j < a.a0 && a.assign[j] == j;
}

// sum of v over the workgroup, to every thread
__device__ __forceinline__ uint32_t edd_block_sum(uint32_t v, uint32_t *lds /* [EDD_WAVES] */) {
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < EDD_WAVES; ++w) s += lds[w];
    return s;
}

__global__ __launch_bounds__(EDD_THREADS) void edit_dedup_count_kernel(CompactArgs a) {
    __shared__ uint32_t wsum[EDD_WAVES];
    const uint32_t p0 = blockIdx.x * a.chunk, p1 = min(a.N, p0 + a.chunk);
    uint32_t n = 0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += EDD_THREADS) n += edd_is_rep(a, p) ? 1u : 0u;
    n = edd_block_sum(n, wsum);
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(EDD_THREADS) void edit_dedup_compact_kernel(CompactArgs a) {
    __shared__ uint32_t wsum[EDD_WAVES], wcnt[EDD_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t before = 0, all = 0;
    for (uint32_t k = tid; k < a.nchunks; k += EDD_THREADS) { const uint32_t c = a.cnt[k]; all += c; before += k < blockIdx.x ? c : 0u; }
    before = edd_block_sum(before, wsum);
    all = edd_block_sum(all, wsum);
    if (blockIdx.x == 0) {
        if (tid == 0) *a.nlist = all;
        a.keys[tid] = 0ull;                                      // EDD_THREADS == EDD_MAX_BAND
    }
    const uint32_t p0 = blockIdx.x * a.chunk, p1 = min(a.N, p0 + a.chunk);
    for (uint32_t base = p0; base < p1; base += EDD_THREADS) {   // uniform
        const uint32_t p = base + tid;
        const bool f = p < p1 && edd_is_rep(a, p);
        const unsigned long long b = __ballot(f);
        __syncthreads();
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pos = before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)), step = 0;
#pragma unroll
        for (int w = 0; w < EDD_WAVES; ++w) { pos += (uint32_t)w < wave ? wcnt[w] : 0u; step += wcnt[w]; }
        if (f) a.list[a.reverse ? all - 1u - pos : pos] = a.order[p];
        before += step;
    }
}

// ---------------------------------------------------------------- the list kernel
// Positions of a list per work item where D2G_EDIT_TILE does not say: a work item builds the row's table once, so a longer tile spreads
// that over more rounds (edit_near_kernel's 512 at most), but the grid must stay full: the largest multiple of 64 that still leaves a
// work item per workgroup, EDD_TILE_MIN at least.  The list's length is a device value, so the kernel computes it.
__device__ __forceinline__ uint32_t edd_tile(uint32_t nrows, uint32_t L, uint32_t grid) {
    const uint64_t t = ((uint64_t)nrows * L / grid) & ~63ull;
    return (uint32_t)(t < EDD_TILE_MIN ? EDD_TILE_MIN : t > EDD_TILE_MAX ? EDD_TILE_MAX : t);
}
struct ListArgs {
    const uint8_t *codes;
    const uint64_t *doff;
    const uint32_t *len;
    const uint32_t *list, *nlist;      // the representatives in front of the band, their number
    uint32_t sigma, T, a0, nrows;
    uint32_t tile, stride;             // tile: positions of a list per work item, 0 = by the list's length (edd_tile); stride: odd, >= (the most words of a list row of the band) + 4
    unsigned long long *keys;          // [nrows]
    uint32_t *block;                   // [nrows][EDD_MAX_BAND]
};

__global__ __launch_bounds__(64) void edit_dedup_list_kernel(ListArgs a) {
    extern __shared__ uint32_t edd_lds[];
    const uint32_t lane = threadIdx.x, T = a.T, stride = a.stride;
    const uint32_t L = min(*a.nlist, a.a0);
    const uint32_t tile = a.tile ? a.tile : edd_tile(a.nrows, L, gridDim.x), own_tiles = (a.nrows + tile - 1) / tile;
    const uint32_t per_row = (L + tile - 1) / tile + own_tiles;
    const uint64_t items = (uint64_t)a.nrows * per_row;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {          // everything about an item is wave-uniform
        const uint32_t r = (uint32_t)(item / per_row), t = (uint32_t)(item % per_row);
        const uint32_t i = a.a0 + r, m = a.len[i], W = (m + 31) >> 5;
        if (!edd_row_fits(a.sigma, m)) continue;                                 // an all-columns row
        const bool own = t >= per_row - own_tiles;                               // the band's own block: columns a0 + p, p < r
        const uint32_t p0 = (own ? t - (per_row - own_tiles) : t) * tile, p1 = min(own ? r : L, p0 + tile);
        if (p0 >= p1) continue;
        bool any = false;
        for (uint32_t p = p0 + lane; p < p1; p += 64) { const uint32_t n = a.len[own ? a.a0 + p : a.list[p]]; any |= m && n && edd_absdiff(m, n) <= T; }
        const bool run = __any(any);                                             // a tile without a pair for the band builds no table
        if (run) {
            const uint8_t *q = a.codes + a.doff[i];
            __syncthreads();                                                     // the table of the item before this one is read no more
            for (uint32_t e = lane; e < a.sigma * stride; e += 64) edd_lds[e] = 0;
            __syncthreads();
            for (uint32_t x = lane; x < m; x += 64) atomicOr(&edd_lds[(uint32_t)q[x] * stride + 2 + (x >> 5)], 1u << (x & 31));
            __syncthreads();
        }
        const uint32_t dend = m > T ? m - T : 0;
        unsigned long long best = 0;
        for (uint32_t base = p0; base < p1; base += 64) {
            const uint32_t p = base + lane;
            const bool has = p < p1;
            const uint32_t j = has ? (own ? a.a0 + p : a.list[p]) : 0u, n = has ? a.len[j] : 0u, dl = edd_absdiff(m, n);
            bool active = run && has && n && dl <= T;
            uint32_t c = has && dl <= T ? T + 1 - dl : 0u;       // final for a lane that does not run (an empty record: d = the other's length)
            // from here to the end of the chunk loop: edit_near_kernel's pair, statement for statement
            uint64_t VP = ~0ull << (63 - T), VN = 0, hor = 1ull << (62 - (T > m ? T - m : 0));
            int start = (int)T - 63, cur = (int)min(T, m);
            const int brk = (int)(2 * T + n) - (int)m;
            const uint32_t nmax = edd_wave_max32(active ? n : 0u), nchunks = (nmax + 15) / 16, tchunks = (n + 15) / 16;
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
                        const uint32_t *row = edd_lds + sym * stride + wi;
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
            if (has) {
                if (own) a.block[(size_t)r * EDD_MAX_BAND + p] = c;
                else { const unsigned long long k = edd_key(c, j); best = k > best ? k : best; }
            }
        }
        if (!own) {
            best = edd_wave_max(best);
            if (lane == 0 && best) atomicMax(&a.keys[r], best);
        }
    }
}

// ---------------------------------------------------------------- all-columns rows: the best representative of earlier bands
struct BestArgs {
    const uint32_t *rows;              // closeness of band row r at rows + r * N
    const uint32_t *assign;
    uint32_t a0, N, r0;                // the launch's first band row
    unsigned long long *keys;
};

__global__ __launch_bounds__(EDD_THREADS) void edit_dedup_best_kernel(BestArgs a) {
    __shared__ unsigned long long wtot[EDD_WAVES];
    const uint32_t tid = threadIdx.x, r = a.r0 + blockIdx.x;
    const uint32_t *__restrict__ row = a.rows + (size_t)r * a.N;
    const uint32_t *__restrict__ assign = a.assign;
    unsigned long long best = 0;
    for (uint32_t jb = tid; jb < a.a0; jb += EDD_UNROLL * EDD_THREADS) {
        uint32_t c[EDD_UNROLL], rep[EDD_UNROLL];
#pragma unroll
        for (int u = 0; u < EDD_UNROLL; ++u) {
            const uint32_t j = jb + u * EDD_THREADS;
            c[u] = j < a.a0 ? row[j] : 0u;
            rep[u] = j < a.a0 ? assign[j] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < EDD_UNROLL; ++u) {
            const uint32_t j = jb + u * EDD_THREADS;
            if (j < a.a0 && rep[u] == j) { const unsigned long long k = edd_key(c[u], j); best = k > best ? k : best; }
        }
    }
    best = edd_wave_max(best);
    if ((tid & 63u) == 0) wtot[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < EDD_WAVES; ++w) best = wtot[w] > best ? wtot[w] : best;
        a.keys[r] = best;
    }
}

// ---------------------------------------------------------------- the in-order step
struct ResolveArgs {
    const uint32_t *block;             // [nrows][EDD_MAX_BAND]: the list rows' closeness to the band's columns in front of them
    const uint32_t *rows;              // [nrows][N]: the all-columns rows'
    const uint32_t *len;
    uint32_t a0, nrows, N, sigma, list_ok;   // list_ok: 0 = every row is an all-columns row
    const unsigned long long *keys;    // [nrows]: best key over the columns j < a0
    uint32_t *assign;
};

// row r's closeness to the band column `tid`, tid < r
__device__ __forceinline__ uint32_t edd_in_band(const ResolveArgs &a, uint32_t r, uint32_t tid) {
    return a.list_ok && edd_row_fits(a.sigma, a.len[a.a0 + r]) ? a.block[(size_t)r * EDD_MAX_BAND + tid] : a.rows[(size_t)r * a.N + a.a0 + tid];
}

__global__ __launch_bounds__(EDD_THREADS) void edit_dedup_resolve_kernel(ResolveArgs a) {
    __shared__ unsigned long long wtot[2][EDD_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t nrows = a.nrows;                           // <= EDD_MAX_BAND (the launcher's bands)
    bool isrep = false;                                       // of row a0 + tid, once it is decided
    uint32_t c[EDD_AHEAD];
    unsigned long long old[EDD_AHEAD];
#pragma unroll
    for (int p = 0; p < EDD_AHEAD; ++p) {
        const uint32_t r = (uint32_t)p;
        c[p] = (r < nrows && tid < r) ? edd_in_band(a, r, tid) : 0u;
        old[p] = r < nrows ? a.keys[r] : 0ull;
    }
    for (uint32_t rb = 0; rb < nrows; rb += EDD_AHEAD) {
#pragma unroll
        for (int p = 0; p < EDD_AHEAD; ++p) {
            const uint32_t r = rb + p;
            if (r >= nrows) break;                            // uniform
            const uint32_t cur = c[p];
            const unsigned long long oldbest = old[p];
            const uint32_t rn = r + EDD_AHEAD;                // the loads of a later row: independent of this row's decision
            c[p] = (rn < nrows && tid < rn) ? edd_in_band(a, rn, tid) : 0u;
            old[p] = rn < nrows ? a.keys[rn] : 0ull;
            if (wave * 64u < r) {                             // (wave-uniform) this wave owns columns in front of row r
                unsigned long long k = (tid < r && isrep) ? edd_key(cur, a.a0 + tid) : 0ull;
                k = edd_wave_max(k);
                if ((tid & 63u) == 0) wtot[r & 1u][wave] = k;
            } else if ((tid & 63u) == 0) wtot[r & 1u][wave] = 0ull;
            __syncthreads();
            unsigned long long m = oldbest;
#pragma unroll
            for (int w = 0; w < EDD_WAVES; ++w) { const unsigned long long x = wtot[r & 1u][w]; m = x > m ? x : m; }
            if (tid == r) isrep = m == 0ull;
            if (tid == 0) a.assign[a.a0 + r] = m ? 0xFFFFFFFFu - (uint32_t)m : a.a0 + r;
        }
    }
}

uint32_t edd_stride(uint32_t len) { return (((len + 31) / 32) + 4) | 1u; }

// The route of row i: true = the list kernel.  The dispatcher (D2G_EDIT_DEDUP_ROUTE unset or 0) takes it wherever it exists: on every
// shape of profiles/edit_dedup_time.json it is the faster of the two forced routes (tools/edit_dedup_time.py writes that file), by 1.21 x
// where every record founds a cluster (20 000 unrelated reads: N^2 / 2 pairs here, N^2 there) and by 1.8 .. 6.0 x elsewhere.
bool edd_list_row(const d2g_ctx *ctx, const d2g_seqset *ss, uint32_t i, uint32_t T) {
    if (T > (uint32_t)D2G_EDIT_BAND_MAX || ctx->edit.dedup_route == 2) return false;
    return (uint64_t)ss->sigma * edd_stride(ss->len[i]) <= EDIT_LDS_WORDS;
}

}  // namespace

void d2g_warm_edit_dedup() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&edit_dedup_list_kernel));
}

extern "C" {

int d2g_edit_dedup_dev(d2g_ctx *ctx, const d2g_seqset *ss, uint32_t T, uint32_t *assign_dev, size_t band_rows, void *stream) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, T < (1u << 31) - 1, "d2g_edit_dedup_dev: the bound must be below 2^31 - 1");
    D2G_CHECK(ctx, ss->N < (1ull << 31), "d2g_edit_dedup_dev: too many records");
    const uint32_t N = (uint32_t)ss->N;
    if (!N) return D2G_OK;
    D2G_CHECK(ctx, assign_dev != nullptr, "d2g_edit_dedup_dev: null assignment");
    const uint32_t B = (uint32_t)std::min<size_t>(std::min<size_t>(band_rows ? band_rows : EDD_MAX_BAND, EDD_MAX_BAND), N);
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> list_row(N);
    bool any_all = false;
    for (uint32_t i = 0; i < N; ++i) { list_row[i] = edd_list_row(ctx, ss, i, T); any_all |= !list_row[i]; }
    // scratch of the context (grow-only, K2e's one-stream rule): the list [N], its length [1], the chunk counts, the band's own block
    const uint32_t chunk = d2g_edit_dedup_chunk(N, ctx->limits);   // EDD_CHUNK, or what EDD_MAX_CHUNKS workgroups need to cover N
    const uint32_t nchunks = div_up<uint32_t>(N, chunk);
    if (int rc = ctx->edit_dedup_ws.grow(ctx, (size_t)N + 1 + EDD_MAX_CHUNKS + EDD_MAX_BAND * EDD_MAX_BAND, 0, "edit dedup scratch alloc")) return rc;
    if (int rc = ctx->dedup_keys.grow(ctx, EDD_MAX_BAND, 0, "dedup keys alloc")) return rc;
    if (any_all) if (int rc = ctx->knn_band.grow(ctx, (size_t)B * N, 0, "edit dedup band alloc")) return rc;
    uint32_t *const d_list = ctx->edit_dedup_ws, *const d_nlist = d_list + N, *const d_cnt = d_nlist + 1, *const d_block = d_cnt + EDD_MAX_CHUNKS;
    const hipStream_t s = as_stream(stream);
    const uint32_t tile = ctx->edit.tile > 0 ? (uint32_t)ctx->edit.tile : 0u, tile_lo = tile ? tile : EDD_TILE_MIN;   // tile_lo: the most work items a band can have
    for (uint32_t a0 = 0; a0 < N; a0 += B) {
        const uint32_t a1 = std::min(a0 + B, N), nrows = a1 - a0;
        uint32_t lmax = 0, nlistrows = 0;
        for (uint32_t i = a0; i < a1; ++i) if (list_row[i]) { lmax = std::max(lmax, ss->len[i]); ++nlistrows; }
        d2g_timer tm(ctx, &ctx->ev_editdedup, s);
        {
            CompactArgs c{ss->order, assign_dev, N, a0, chunk, nchunks, (uint32_t)ctx->edit.dedup_reverse, d_cnt, d_list, d_nlist, ctx->dedup_keys};
            d2g_timer tl(ctx, &ctx->ev_editdedup_list, s);
            hipLaunchKernelGGL(edit_dedup_count_kernel, dim3(nchunks), dim3(EDD_THREADS), 0, s, c);
            hipLaunchKernelGGL(edit_dedup_compact_kernel, dim3(nchunks), dim3(EDD_THREADS), 0, s, c);
            tl.stop();
        }
        if (nlistrows) {
            ListArgs l{ss->codes, ss->doff, ss->dlen, d_list, d_nlist, ss->sigma, T, a0, nrows, tile, edd_stride(lmax), ctx->dedup_keys, d_block};
            const uint64_t items = (uint64_t)nrows * (div_up<uint32_t>(a0, tile_lo) + div_up<uint32_t>(nrows, tile_lo));
            const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)std::max(ctx->num_cus, 1) * EDD_WAVES_PER_CU));
            hipLaunchKernelGGL(edit_dedup_list_kernel, dim3(grid), dim3(64), sizeof(uint32_t) * (size_t)ss->sigma * l.stride, s, l);
        }
        for (uint32_t r = a0; r < a1;) {                     // runs of consecutive all-columns rows
            if (list_row[r]) { ++r; continue; }
            uint32_t e = r + 1;
            while (e < a1 && !list_row[e]) ++e;
            if (int rc = d2g_edit_near_dev(ctx, ss, r, e, T, ctx->knn_band + (size_t)(r - a0) * N, stream)) { tm.stop(); return rc; }
            BestArgs b{ctx->knn_band, assign_dev, a0, N, r - a0, ctx->dedup_keys};
            hipLaunchKernelGGL(edit_dedup_best_kernel, dim3(e - r), dim3(EDD_THREADS), 0, s, b);
            r = e;
        }
        {
            ResolveArgs v{d_block, ctx->knn_band, ss->dlen, a0, nrows, N, ss->sigma, T <= (uint32_t)D2G_EDIT_BAND_MAX && ctx->edit.dedup_route != 2 ? 1u : 0u, ctx->dedup_keys, assign_dev};
            d2g_timer tr(ctx, &ctx->ev_editdedup_resolve, s);
            hipLaunchKernelGGL(edit_dedup_resolve_kernel, dim3(1), dim3(EDD_THREADS), 0, s, v);
            tr.stop();
        }
        tm.stop();
        D2G_HIP(ctx, hipGetLastError());
    }
    return D2G_OK;
}

int d2g_edit_dedup(d2g_ctx *ctx, const d2g_seqset *ss, uint32_t T, size_t band_rows, uint32_t *assign_out) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    if (!ss->N) return D2G_OK;
    D2G_CHECK(ctx, assign_out != nullptr, "d2g_edit_dedup: null assignment");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    d2g_dev<uint32_t> d_assign;
    if (int rc = d_assign.alloc(ctx, ss->N, "edit dedup assignment alloc")) return rc;
    if (int rc = d2g_edit_dedup_dev(ctx, ss, T, d_assign, band_rows, nullptr)) return rc;
    D2G_HIP(ctx, hipMemcpy(assign_out, d_assign, ss->N * 4, hipMemcpyDeviceToHost));
    return D2G_OK;
}

}  // extern "C"
