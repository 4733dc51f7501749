// d2g_k3_countsketch.hip -- K3k, the count-sketch chain of the --multiset path.
#include "d2g_k3.h"
#include <algorithm>
#include <cstring>

// =============================================================================================
// K3k: --multiset -c/--countsketch-size/--countmin-size <cells> -- approximate counting in a single-row count-sketch
//   reference src/counter.h:16-19 (the row of `cells` floats), 68-77 (Counter::add(uint64_t)), 131-137 (finalize into the sketch)
// Per k-mer x the walker emits: hv = Wang(maskfn(x)) = Wang(Wang(x ^ XORMASK)), table[hv % cells] += (hv >> 63) ? +1 : -1 -- in int32,
// so the result is the exact integer whatever the order (the reference's float cell stops counting at 2^24: SURVEY F28).  Then every
// cell with |c| >= threshold (and > 0) is one element (id = the cell number, weight = |c|) of BagMinHash.
//   k3k_add      one walk of the k-mers, one atomic add each: into an LDS copy of the genome's row that the workgroup flushes (cells
//                <= L), or straight into the row in global memory
//   k3k_count / k3k_scan / k3k_write   the kept cells of every row, in ascending order, as the (ids, w) lists the list stage reads
//   k3_lists_prepare / k3_lists_walk        BagMinHash over those lists where they lie (the list stage, d2g_k3_lists.hip)
// A batch whose rows do not fit the table budget goes in groups of consecutive genomes (d2g_cs_groups), each through all three stages.
// =============================================================================================
namespace {

// L: the most cells a workgroup accumulates in LDS.  Measured (profiles/countsketch_time.json, 1000 x 5 Mbp): the LDS form never stops
// winning while the row fits -- its flush is coalesced (consecutive lanes, consecutive cells: full 256-byte atomic wave instructions)
// where the global form issues 64 separate 4-byte requests per wave instruction and runs at about 2.8e10 adds/s for the whole chip.
// 9 ms up to 8192 cells (five workgroups per CU), 11.5 at 16384, 25 at 40960 (one workgroup per CU: the walker loses its occupancy)
// against 136-182 ms in the global form: no crossover below the 160 KiB of LDS, so L is that bound.
constexpr uint32_t K3K_LDS_CELLS = D2G_CS_LDS_MAX;
static_assert(K3K_LDS_CELLS <= D2G_CS_LDS_MAX, "the LDS form holds a whole row");
constexpr int K3K_PER = 16;                              // consecutive cells per lane of the compaction
constexpr int K3K_TILE = K3_THREADS * K3K_PER;           // cells per workgroup of the compaction
constexpr int K3K_SCAN_THREADS = 1024;

struct CsArgs {
    KmerArgs km;
    uint64_t xormask;
    int32_t *table;              // [rows][cells]
    const uint32_t *g_row;       // [n] row of genome g in this group's table
    uint64_t cells;              // 1 .. 2^31
    uint64_t recip;              // floor(2^64 / cells) (not read when cells is a power of two)
};

template <bool FILT, bool WIN, bool AA, bool LDS>
__global__ __launch_bounds__(K1_THREADS) void k3k_add_kernel(CsArgs a) {
    extern __shared__ __attribute__((aligned(16))) int32_t k3k_lds[];
    const uint32_t g = a.km.blk_genome[blockIdx.x + a.km.blk0];
    int32_t *row = a.table + (size_t)a.g_row[g] * a.cells;
    const uint64_t xormask = a.xormask, cells = a.cells, recip = a.recip;
    if constexpr (LDS) {
        const uint32_t C = (uint32_t)cells;
        for (uint32_t i = threadIdx.x; i < C; i += K1_THREADS) k3k_lds[i] = 0;
        __syncthreads();
        d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
            const uint64_t hv = wang64(wang64(x ^ xormask));             // maskfn (src/enums.h:136-140), then counter.h:74
            atomicAdd(&k3k_lds[(uint32_t)d2g_cs_mod(hv, cells, recip)], (hv >> 63) ? 1 : -1);   // BM64 clear: -1 (counter.h:75)
        });
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < C; i += K1_THREADS) {
            const int32_t v = k3k_lds[i];
            if (v) atomicAdd(&row[i], v);                                // the other workgroups of this genome add into the same cells
        }
    } else {
        d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
            const uint64_t hv = wang64(wang64(x ^ xormask));
            atomicAdd(&row[d2g_cs_mod(hv, cells, recip)], (hv >> 63) ? 1 : -1);
        });
    }
}

struct CsListArgs {
    const int32_t *table;        // [rows][cells]
    uint64_t cells;
    uint32_t ntile, rows;        // tiles of K3K_TILE cells per row; workgroup b of count / write owns tile b % ntile of row b / ntile
    double thr;
    uint32_t *tile_cnt;          // [rows * ntile] kept cells
    uint64_t *tile_off;          // [rows * ntile + 1] exclusive prefix: where the tile writes
    uint64_t *row_off;           // [rows + 1] where a row's list begins
    unsigned long long *total;   // [rows] sum of the kept |c|, zeroed by the host
    uint64_t *ids; double *w;    // the lists
};
// the weight a cell passes on: |c| when |c| >= threshold (counter.h:135: >=, not the exact mode's >) and not 0 (BagMinHash2::update
// ignores a weight of 0), else 0.  |c| < 2^31: an input holds fewer k-mers
__device__ __forceinline__ uint32_t k3k_weight(int32_t c, double thr) {
    const uint32_t v = c < 0 ? 0u - (uint32_t)c : (uint32_t)c;
    return (v && (double)v >= thr) ? v : 0u;
}
__global__ __launch_bounds__(K3_THREADS) void k3k_count_kernel(CsListArgs a) {
    __shared__ uint32_t cnt;
    __shared__ unsigned long long ws;
    const uint32_t row = blockIdx.x / a.ntile, t = blockIdx.x % a.ntile;
    if (threadIdx.x == 0) { cnt = 0; ws = 0; }
    __syncthreads();
    const int32_t *tab = a.table + (size_t)row * a.cells;
    const uint64_t c0 = (uint64_t)t * K3K_TILE + (uint64_t)threadIdx.x * K3K_PER;
    uint32_t mine = 0;
    unsigned long long sum = 0;
#pragma unroll
    for (int j = 0; j < K3K_PER; ++j)
        if (c0 + j < a.cells) { const uint32_t v = k3k_weight(tab[c0 + j], a.thr); mine += v != 0; sum += v; }
    if (mine) { atomicAdd(&cnt, mine); atomicAdd(&ws, sum); }
    __syncthreads();
    if (threadIdx.x == 0) { a.tile_cnt[blockIdx.x] = cnt; if (ws) atomicAdd(&a.total[row], ws); }
}
// one workgroup: exclusive prefix over all tiles of the group (row-major: a row's tiles are consecutive, so its list is contiguous and ascending)
__global__ __launch_bounds__(K3K_SCAN_THREADS) void k3k_scan_kernel(CsListArgs a) {
    __shared__ uint64_t part[K3K_SCAN_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint64_t N = (uint64_t)a.rows * a.ntile, per = (N + K3K_SCAN_THREADS - 1) / K3K_SCAN_THREADS;
    const uint64_t lo = tid * per < N ? tid * per : N, hi = lo + per < N ? lo + per : N;
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += a.tile_cnt[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t o = 1; o < K3K_SCAN_THREADS; o <<= 1) {
        const uint64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint64_t run = part[tid] - s;
    for (uint64_t i = lo; i < hi; ++i) {
        a.tile_off[i] = run;
        if (i % a.ntile == 0) a.row_off[i / a.ntile] = run;
        run += a.tile_cnt[i];
    }
    if (tid == K3K_SCAN_THREADS - 1) { a.tile_off[N] = part[tid]; a.row_off[a.rows] = part[tid]; }
}
__global__ __launch_bounds__(K3_THREADS) void k3k_write_kernel(CsListArgs a) {
    __shared__ uint32_t wsum[K3_THREADS / 64];
    if (a.tile_cnt[blockIdx.x] == 0) return;                            // uniform over the workgroup
    const uint32_t tid = threadIdx.x, row = blockIdx.x / a.ntile, t = blockIdx.x % a.ntile;
    const int32_t *tab = a.table + (size_t)row * a.cells;
    const uint64_t c0 = (uint64_t)t * K3K_TILE + (uint64_t)tid * K3K_PER;
    uint32_t v[K3K_PER], mine = 0;
#pragma unroll
    for (int j = 0; j < K3K_PER; ++j) { v[j] = c0 + j < a.cells ? k3k_weight(tab[c0 + j], a.thr) : 0u; mine += v[j] != 0; }
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if ((tid & 63) >= (uint32_t)o) incl += u; }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint64_t pos = a.tile_off[blockIdx.x] + (incl - mine);
    for (uint32_t w = 0; w < (tid >> 6); ++w) pos += wsum[w];
#pragma unroll
    for (int j = 0; j < K3K_PER; ++j)
        if (v[j]) { a.ids[pos] = c0 + j; a.w[pos] = (double)v[j]; ++pos; }
}

// what a count-sketch call refuses before it stages or launches anything: the cells, and an input that could overflow an int32 cell
int cs_check(d2g_ctx *ctx, const PackedRuns &in, uint64_t cells) {
    D2G_CHECK(ctx, cells >= 1 && cells <= D2G_CS_MAX_CELLS, "count-sketch: cells must be in [1, 2^31]");
    if (!in.genome_run_off || (in.nrun && !in.run_len) || in.k < 1) return D2G_OK;       // left to the plan's own checks
    for (size_t g = 0; g < in.n; ++g) {
        uint64_t nk = 0;
        for (uint64_t r = in.genome_run_off[g]; r < in.genome_run_off[g + 1] && r < in.nrun; ++r) nk += d2g_run_emissions_of(in.run_len[r], in.k, in.w);
        D2G_CHECK(ctx, nk < D2G_CS_MAX_KMERS, "count-sketch: 2^31 k-mers or more in one input (a cell is an int32)");
    }
    return D2G_OK;
}

// one count-sketch call over a staged batch: what it is to leave behind
struct CsRun {
    uint64_t xormask = 0, cells = 1;
    double thr = 0.;
    int32_t *table_out = nullptr;                                       // host [n][cells]: the signed tables
    bool lists = false;                                                 // host lists: ids_out / w_out [cap], set_off_out [n + 1], total_out [n]
    uint64_t *ids_out = nullptr; double *w_out = nullptr; size_t cap = 0; uint64_t *set_off_out = nullptr, *total_out = nullptr;
    size_t m = 0;                                                       // > 0: BagMinHash registers [n][m] and total weights [n] ...
    double *sig_out = nullptr, *tw_out = nullptr; hipMemcpyKind out = hipMemcpyDeviceToHost;   // ... copied out as `out` says
};

int cs_run(const KmerBatch &b, const CsRun &c) {
    d2g_ctx *ctx = b.ctx;
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    const size_t n = r.n, m = c.m;
    if (n == 0) return D2G_OK;
    d2g_k3_state *st = r.st;
    hipStream_t s = r.s;
    const K3Host &kh = r.kh;
    const uint64_t cells = c.cells;
    D2G_CHECK(ctx, kh.gblk[n] == r.nblk, "internal: K3k block layout disagrees with the launch plan");
    // the table budget: what is free now and what the state already holds; a sixth of it, since a kept cell costs 16 bytes of list
    // beside its 4 of table
    size_t free_b = 0, total_b = 0;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    D2G_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t avail = (uint64_t)free_b + st->cs.d_cs_table.cap() * sizeof(int32_t), row_bytes = cells * sizeof(int32_t);
    if (row_bytes > avail) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "count-sketch: one table of %llu cells needs %llu bytes of device memory, %llu are free",
                      (unsigned long long)cells, (unsigned long long)row_bytes, (unsigned long long)avail);
        ctx->last_error = msg;
        return D2G_ERR_NOMEM;
    }
    const uint64_t budget = ctx->k3_tune.cs_table_bytes ? ctx->k3_tune.cs_table_bytes : avail / 6;
    std::vector<uint32_t> row;
    const std::vector<size_t> cut = d2g_cs_groups(kh.gblk.data(), n, cells, budget, row);
    const uint64_t ntile = div_up<uint64_t>(cells, K3K_TILE);
    if (int rc = st->cs.d_cs_row.grow(ctx, n, 4096)) return rc;
    if (!st->count.d_status) if (int rc = st->count.d_status.alloc(ctx, 2, "k3 status alloc")) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->cs.d_cs_row, row.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemsetAsync(st->count.d_status, 0, 2 * sizeof(int), s));
    if (m) {
        if (int rc = st->sketch.d_h.grow(ctx, std::max<size_t>(n * m, 1), 4096)) return rc;
        if (int rc = st->sketch.d_tw.grow(ctx, n, 4096)) return rc;
        if (int rc = st->sketch.d_guess.grow(ctx, n, 4096)) return rc;
        if (int rc = st->sketch.d_redo.grow(ctx, n, 4096)) return rc;
        k3_init_registers(s, st->sketch.d_h, n * m, st->sketch.d_tw, st->sketch.d_redo, n);
    }
    const int lds_cells = ctx->k3_tune.cs_lds_cells >= 0 ? ctx->k3_tune.cs_lds_cells : (int)K3K_LDS_CELLS;
    const bool lds = cells <= (uint64_t)lds_cells;
    const auto add = lds ? d2g_walker_variant(r.km, [](auto f, auto w, auto aa) { return k3k_add_kernel<f(), w(), aa(), true>; })
                         : d2g_walker_variant(r.km, [](auto f, auto w, auto aa) { return k3k_add_kernel<f(), w(), aa(), false>; });
    if (lds) D2G_HIP(ctx, hipFuncSetAttribute((const void *)add, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(cells * sizeof(int32_t))));
    std::vector<uint64_t> rowinfo, set_off, total;
    std::vector<double> tw;
    uint64_t at = 0;                                                    // host lists: elements written so far
    ctx->cs_batches += 1; ctx->cs_groups += cut.size() - 1;
    for (size_t j = 0; j + 1 < cut.size(); ++j) {
        const size_t g0 = cut[j], g1 = cut[j + 1], ng = g1 - g0;
        size_t rows = 0;
        for (size_t g = g0; g < g1; ++g) rows += row[g] != ~0u;
        set_off.assign(ng + 1, 0); total.assign(ng, 0);
        if (rows) {
            // ---- the table: zeroed for exactly rows * cells cells, one walk
            D2G_CHECK(ctx, rows * ntile < (1ull << 31), "count-sketch: too many table tiles in one group; sketch in smaller batches");
            const size_t tcells = rows * cells;
            if (st->cs.d_cs_table.cap() < tcells) if (int rc = st->cs.d_cs_table.alloc(ctx, tcells, "count-sketch table")) return rc;
            ctx->cs_table_bytes = std::max<uint64_t>(ctx->cs_table_bytes, tcells * sizeof(int32_t));
            {
                d2g_timer tm(ctx, &ctx->ev_k3k, s);
                D2G_HIP(ctx, hipMemsetAsync(st->cs.d_cs_table, 0, tcells * sizeof(int32_t), s));
                CsArgs a;
                a.km = r.km; a.km.blk0 = kh.gblk[g0]; a.xormask = c.xormask; a.table = st->cs.d_cs_table; a.g_row = st->cs.d_cs_row;
                a.cells = cells; a.recip = d2g_cs_recip(cells);
                const unsigned nb = kh.gblk[g1] - kh.gblk[g0];
                hipLaunchKernelGGL(add, dim3(nb), dim3(K1_THREADS), lds ? cells * sizeof(int32_t) : 0, s, a);
                tm.stop();
            }
            // ---- the lists: count per tile, prefix, write; only row_off and the totals come back in between
            const size_t N = rows * ntile;
            if (int rc = st->cs.d_cs_tile_cnt.grow(ctx, N, 4096)) return rc;
            if (int rc = st->cs.d_cs_tile_off.grow(ctx, N + 1 + 2 * rows + 1, 4096)) return rc;
            CsListArgs la;
            la.table = st->cs.d_cs_table; la.cells = cells; la.ntile = (uint32_t)ntile; la.rows = (uint32_t)rows; la.thr = c.thr;
            la.tile_cnt = st->cs.d_cs_tile_cnt; la.tile_off = st->cs.d_cs_tile_off; la.row_off = st->cs.d_cs_tile_off + N + 1;
            la.total = reinterpret_cast<unsigned long long *>(la.row_off + rows + 1); la.ids = nullptr; la.w = nullptr;
            rowinfo.assign(2 * rows + 1, 0);
            d2g_timer tm(ctx, &ctx->ev_k3kcompact, s);
            D2G_HIP(ctx, hipMemsetAsync(la.total, 0, rows * sizeof(uint64_t), s));
            hipLaunchKernelGGL(k3k_count_kernel, dim3((unsigned)N), dim3(K3_THREADS), 0, s, la);
            hipLaunchKernelGGL(k3k_scan_kernel, dim3(1), dim3(K3K_SCAN_THREADS), 0, s, la);
            D2G_HIP(ctx, hipMemcpyAsync(rowinfo.data(), la.row_off, rowinfo.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            D2G_HIP(ctx, hipStreamSynchronize(s));
            const uint64_t nel = rowinfo[rows];
            if (int rc = st->cs.d_cs_ids.grow(ctx, std::max<uint64_t>(nel, 1), 4096)) return rc;
            if (int rc = st->cs.d_cs_w.grow(ctx, std::max<uint64_t>(nel, 1), 4096)) return rc;
            la.ids = st->cs.d_cs_ids; la.w = st->cs.d_cs_w;
            if (nel) hipLaunchKernelGGL(k3k_write_kernel, dim3((unsigned)N), dim3(K3_THREADS), 0, s, la);
            tm.stop();
            d2g_cs_expand_set_off(row.data(), g0, g1, rowinfo.data(), rowinfo.data() + rows + 1, set_off.data(), total.data());
        }
        const uint64_t nel = set_off[ng];
        if (c.table_out) {
            for (size_t g = g0; g < g1; ++g) {
                if (row[g] == ~0u) std::memset(c.table_out + g * cells, 0, cells * sizeof(int32_t));
                else D2G_HIP(ctx, hipMemcpyAsync(c.table_out + g * cells, st->cs.d_cs_table + (size_t)row[g] * cells, cells * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            }
            D2G_HIP(ctx, hipStreamSynchronize(s));
        }
        if (c.lists) {
            D2G_CHECK(ctx, at + nel <= c.cap, "d2g_countsketch_cells: output capacity too small");
            if (nel) {
                D2G_HIP(ctx, hipMemcpyAsync(c.ids_out + at, st->cs.d_cs_ids, nel * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                D2G_HIP(ctx, hipMemcpyAsync(c.w_out + at, st->cs.d_cs_w, nel * sizeof(double), hipMemcpyDeviceToHost, s));
                D2G_HIP(ctx, hipStreamSynchronize(s));
            }
            for (size_t i = 0; i < ng; ++i) { c.set_off_out[g0 + i] = at + set_off[i]; c.total_out[g0 + i] = total[i]; }
            at += nel;
            c.set_off_out[n] = at;
        }
        if (m && nel) {
            // ---- BagMinHash over the lists where they lie, into this group's slices of the registers (a group without a kept cell
            // keeps its +inf registers and total 0)
            tw.resize(ng);
            for (size_t i = 0; i < ng; ++i) tw[i] = (double)total[i];
            const K3ListRegs regs{st->sketch.d_h + g0 * m, st->sketch.d_guess + g0, st->sketch.d_redo + g0, st->sketch.d_tw + g0, st->count.d_status};
            K3ListWalk walk;
            d2g_timer tm(ctx, &ctx->ev_k3kbmh, s);
            int rc = k3_lists_prepare(ctx, s, st->cs.d_cs_ids, st->cs.d_cs_w, set_off.data(), tw.data(), ng, m, st->cs.lists, regs, &walk);
            if (!rc) rc = k3_lists_walk(ctx, s, walk);
            tm.stop();
            if (rc) { (void)hipStreamSynchronize(s); return rc; }              // `tw` is read by a copy that may still be in flight
        }
    }
    D2G_HIP(ctx, hipGetLastError());
    if (m) {
        D2G_HIP(ctx, hipMemcpyAsync(c.sig_out, st->sketch.d_h, n * m * sizeof(double), c.out, s));
        D2G_HIP(ctx, hipMemcpyAsync(c.tw_out, st->sketch.d_tw, n * sizeof(double), c.out, s));
    }
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return D2G_OK;
}

int cs_sketch_check(d2g_ctx *ctx, const PackedRuns &in, size_t sketchsize, uint64_t cells, double threshold, const double *sig_out, const double *tw_out) {
    if (int rc = bmh_check(ctx, in.n, sketchsize, threshold, sig_out, tw_out)) return rc;
    return cs_check(ctx, in, cells);
}
int sketcher_run_bmh_cs(d2g_sketcher *sk, const PackedRuns &in, uint64_t xormask, size_t sketchsize, uint64_t cells, double threshold,
                        double *sig_out, double *tw_out) {
    if (!sk) return D2G_ERR_INVALID;
    if (int rc = cs_sketch_check(sk->ctx, d2g_sketcher_view(sk, in), sketchsize, cells, threshold, sig_out, tw_out)) return rc;
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    CsRun c;
    c.xormask = xormask; c.cells = cells; c.thr = threshold; c.m = sketchsize; c.sig_out = sig_out; c.tw_out = tw_out;
    return cs_run(b, c);
}

}  // namespace

extern "C" {

int d2g_countsketch_lds_cells(void) { return (int)K3K_LDS_CELLS; }

int d2g_countsketch_stats(d2g_ctx *ctx, uint64_t *table_bytes, uint64_t *groups, uint64_t *batches) {
    if (!ctx) return D2G_ERR_INVALID;
    if (table_bytes) *table_bytes = ctx->cs_table_bytes;
    if (groups) *groups = ctx->cs_groups;
    if (batches) *batches = ctx->cs_batches;
    return D2G_OK;
}

int d2g_sketcher_run_bmh_cs(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                            size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, size_t sketchsize,
                            uint64_t cells, double count_threshold, double *sig_out, double *total_weight_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_run_bmh_cs(sk, in, xormask, sketchsize, cells, count_threshold, sig_out, total_weight_out);
}

int d2g_bmh_sketch_cs(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                      size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, size_t sketchsize,
                      uint64_t cells, double count_threshold, double *sig_out, double *total_weight_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        return sketcher_run_bmh_cs(sk, in, xormask, sketchsize, cells, count_threshold, sig_out, total_weight_out);
    });
}

int d2g_bmh_sketch_cs_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, uint64_t xormask, size_t sketchsize,
                          uint64_t cells, double count_threshold, double *sig_out_dev, double *total_weight_out_dev, void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = cs_sketch_check(ctx, plan->runs(canon), sketchsize, cells, count_threshold, sig_out_dev, total_weight_out_dev)) return rc;
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    CsRun c;
    c.xormask = xormask; c.cells = cells; c.thr = count_threshold; c.m = sketchsize; c.sig_out = sig_out_dev; c.tw_out = total_weight_out_dev;
    c.out = hipMemcpyDeviceToDevice;
    return cs_run(b, c);
}

int d2g_countsketch_table(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                          size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, uint64_t cells,
                          int32_t *table_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, table_out != nullptr || n == 0, "null output");
    if (int rc = cs_check(ctx, in, cells)) return rc;
    D2G_CHECK(ctx, (uint64_t)n * cells <= (1ull << 28), "d2g_countsketch_table: more than 2^28 cells in all (the dense read-back is for small tables; d2g_countsketch_cells has no such limit)");
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        KmerBatch b;
        if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
        CsRun c;
        c.xormask = xormask; c.cells = cells; c.thr = 0.; c.table_out = table_out;
        return cs_run(b, c);
    });
}

int d2g_countsketch_cells(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                          size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, uint64_t cells,
                          double count_threshold, uint64_t *ids_out, double *w_out, size_t cap, uint64_t *set_off_out, uint64_t *total_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set_off_out != nullptr && (total_out != nullptr || n == 0), "null output");
    D2G_CHECK(ctx, cap == 0 || (ids_out && w_out), "null output");
    D2G_CHECK(ctx, count_threshold == count_threshold, "count_threshold is NaN");
    if (int rc = cs_check(ctx, in, cells)) return rc;
    for (size_t g = 0; g <= n; ++g) set_off_out[g] = 0;
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        KmerBatch b;
        if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
        CsRun c;
        c.xormask = xormask; c.cells = cells; c.thr = count_threshold; c.lists = true;
        c.ids_out = ids_out; c.w_out = w_out; c.cap = cap; c.set_off_out = set_off_out; c.total_out = total_out;
        return cs_run(b, c);
    });
}

}  // extern "C"


void d2g_warm_k3_countsketch() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k3k_count_kernel));
}
