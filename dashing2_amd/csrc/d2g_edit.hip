// d2g_edit.hip -- K2h: exact edit distances between resident records (--parse-by-seq --edit-distance --compute-edit-distance) on gfx950.
//
// Replaces, for every pair, one edlibAlign call in global distance mode on the two records' raw bytes (reference src/cmp_core.cpp:331-347,
// 450-457): the unit-cost Levenshtein distance over bytes.  An integer; the device returns it as u32, exactly.  No floating point here.
//
// The algorithm is Myers' bit-vector recurrence (J. ACM 46(3), 1999) in Hyyro's block form: the query's m rows are cut into blocks of 32,
// a block keeps the vertical deltas of its rows in two words (Pv, Mv), takes the horizontal delta hin in {-1, 0, +1} that enters its top
// row and hands the one that leaves its bottom row to the block below.  Global distance: hin of the first block is +1 in every column,
// Pv starts as all ones, the score starts as m and follows the horizontal deltas of row m.
//
// edit_pair_kernel: ONE WAVE (a workgroup of 64 threads) serves one row record as the query and a tile of column records.
//   * the query's match masks Peq[code][block] are built once in LDS by LDS atomic OR, one per query symbol (sigma x P words: a row of
//     the table is as wide as a pair has lanes, so that lanes on different symbols read different banks);
//   * a lane is one block of the query.  A pair takes P = the power of two >= B lanes, so 64 / P column records run side by side;
//   * the blocks of a pair advance as an anti-diagonal wavefront: lane b works on column t - b at step t, and takes the horizontal delta
//     AND the column's symbol from lane b - 1 with one cross-lane move per step; lane 0 of a pair reads the target, 16 symbols per load,
//     one load ahead;
//   * Pv, Mv and the score stay in registers; the lane that holds the query's last row adds the delta at bit (m - 1) mod 32;
//   * a query of more blocks than a strip holds (64, fewer where sigma is large: the table of one strip and the planes below share
//     64 KiB of LDS) runs strip by strip, one pair per wave: the horizontal deltas that leave a strip's last row are kept as two bit
//     planes over the target's columns in LDS, written 32 columns at a time by the strip's last lane and read by lane 0 of the next
//     strip, in place (the writer trails the reader by the strip's height);
//   * the columns of a tile are taken in order of length (an order of ALL records, made once per d2g_seqset), so the lane groups of a
//     wave run to nearly the same column count; outputs are written by index, so the order is invisible.
// Rows are launched in three classes by their block count (up to 8 blocks; one strip; several strips) so that a short query never
// carries the LDS of a long one; a workgroup whose row is of another class leaves at once.
// Not built: the alignment path, a register-resident Peq for small alphabets.  Banding and the early exit at a threshold are not this
// kernel's either (a block outside a band would be an idle lane here, not a saved step): they are d2g_edit_near.hip's (K2i).
#include "d2g_edit.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

namespace {

constexpr int EDIT_SMALL_BLOCKS = 8;       // rows of up to this many blocks form the first launch class (EDIT_PAD, EDIT_LDS_WORDS: d2g_edit.h)

struct EditArgs {
    const uint8_t *codes;              // recoded symbols, record i at codes + doff[i]
    const uint64_t *doff;              // [N + 1], multiples of EDIT_PAD
    const uint32_t *len;               // [N]
    const uint32_t *order;             // [N] record indices by ascending length
    uint32_t N, sigma;
    uint32_t a0, a1, b0, b1;           // row records [a0, a1); column records [b0, b1) (ut: every j > i)
    uint32_t row0;                     // first row of this launch
    uint32_t ntiles, tile;             // tiles of `tile` positions of `order`
    uint32_t cls;                      // 0: rows of <= EDIT_SMALL_BLOCKS blocks, 1: other rows of one strip, 2: rows of several strips
    uint32_t strip;                    // blocks per strip
    uint32_t plane_words;              // words per plane (class 2)
    int ut;
    uint32_t *out;
};

__device__ __forceinline__ bool edit_valid(const EditArgs &a, uint32_t i, uint32_t j) { return a.ut ? j > i : (j >= a.b0 && j < a.b1); }

__device__ __forceinline__ size_t edit_out_index(const EditArgs &a, uint32_t i, uint32_t j) {
    if (a.ut) {
        const uint64_t n = i - a.a0, tri1 = (uint64_t)i * (i ? i - 1 : 0) / 2, tri0 = (uint64_t)a.a0 * (a.a0 ? a.a0 - 1 : 0) / 2;
        return (size_t)(n * ((uint64_t)a.N - 1) - (tri1 - tri0) + (j - i - 1));
    }
    return (size_t)(i - a.a0) * (a.b1 - a.b0) + (j - a.b0);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// the table of blocks [blk0, blk0 + nblk) of the query: peq[code * stride + block].  stride is the lanes of a pair (a power of two) or
// the strip's blocks: with 32 | stride the lanes of a pair, each on a symbol of its own, read 32 different banks
__device__ __forceinline__ void edit_build_peq(uint32_t *peq, const uint8_t *q, uint32_t m, uint32_t blk0, uint32_t nblk, uint32_t stride, uint32_t sigma,
                                               uint32_t lane) {
    __syncthreads();                                             // the previous strip's reads are done
    for (uint32_t e = lane; e < sigma * stride; e += 64) peq[e] = 0;
    __syncthreads();
    const uint32_t r0 = blk0 * 32, r1 = min(m, (blk0 + nblk) * 32);
    for (uint32_t r = r0 + lane; r < r1; r += 64) atomicOr(&peq[(uint32_t)q[r] * stride + ((r - r0) >> 5)], 1u << (r & 31));
    __syncthreads();
}

// One strip of the query against the column record of every lane group.  b: this lane's block in the strip (lanes with b >= nblk idle),
// hb: the bit of this block's last row, n: the column's length (0 for a group without one), tgt: its codes.  planes_in / planes_out: the
// strip takes its top deltas from / leaves its bottom deltas in pp / pm (one group per wave then), else +1 enters and the score follows.
__device__ __forceinline__ void edit_run_strip(const uint32_t *peq, uint32_t nblk, uint32_t stride, uint32_t b, uint32_t hb, uint32_t n, uint32_t nmax, const uint8_t *tgt,
                                               bool planes_in, bool planes_out, uint32_t *pp, uint32_t *pm, uint32_t &score) {
    uint32_t Pv = 0xffffffffu, Mv = 0, outw = 0, hpw = 0xffffffffu, hmw = 0, accp = 0, accm = 0;
    if (nmax == 0) return;
    const bool first = b == 0, last = b + 1 == nblk;
    const uint32_t nsteps = nmax + nblk - 1, nchunks = (nsteps + 15) / 16, tchunks = (n + 15) / 16;
    const uint4 *t4 = reinterpret_cast<const uint4 *>(tgt);
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (first && tchunks) nxt = t4[0];
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint4 cur = nxt;
        if (first && c + 1 < tchunks) nxt = t4[c + 1];
#pragma unroll
        for (uint32_t u = 0; u < 16; ++u) {
            const uint32_t t = c * 16 + u;
            const uint32_t recv = (uint32_t)__shfl_up((int)outw, 1);
            const uint32_t w = (u >> 2) == 0 ? cur.x : (u >> 2) == 1 ? cur.y : (u >> 2) == 2 ? cur.z : cur.w;
            uint32_t sym, hp, hm;
            if (first) {
                if (planes_in && (t & 31) == 0 && t < n) { hpw = pp[t >> 5]; hmw = pm[t >> 5]; }
                sym = (w >> (8 * (u & 3))) & 255u; hp = hpw & 1u; hm = hmw & 1u;
            } else { sym = recv >> 2; hp = recv & 1u; hm = (recv >> 1) & 1u; }
            const uint32_t col = t - b;
            if (b < nblk && t >= b && col < n) {
                if (first && planes_in) { hpw >>= 1; hmw >>= 1; }
                uint32_t Eq = peq[sym * stride + b];
                const uint32_t Xv = Eq | Mv;
                Eq |= hm;
                const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
                uint32_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
                const uint32_t hpo = (Ph >> hb) & 1u, hmo = (Mh >> hb) & 1u;
                Ph = (Ph << 1) | hp; Mh = (Mh << 1) | hm;
                Pv = Mh | ~(Xv | Ph);
                Mv = Ph & Xv;
                outw = hpo | (hmo << 1) | (sym << 2);
                if (last) {
                    if (planes_out) {
                        accp |= hpo << (col & 31); accm |= hmo << (col & 31);
                        if ((col & 31) == 31 || col + 1 == n) { pp[col >> 5] = accp; pm[col >> 5] = accm; accp = accm = 0; }
                    } else score += hpo - hmo;
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void edit_pair_kernel(EditArgs a) {
    extern __shared__ uint32_t edit_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = a.row0 + blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t m = a.len[i], B = (m + 31) >> 5;
    const uint32_t cls = B <= (uint32_t)EDIT_SMALL_BLOCKS && B <= a.strip ? 0u : B <= a.strip ? 1u : 2u;
    if (cls != a.cls) return;
    const uint32_t p0 = tile * a.tile, p1 = min(a.N, p0 + a.tile);
    {   // a tile without a pair of this launch builds no table
        bool any = false;
        for (uint32_t p = p0 + lane; p < p1; p += 64) any |= edit_valid(a, i, a.order[p]);
        if (!__any(any)) return;
    }
    if (m == 0) {                                                // an empty query: the other record's length, as edlib returns it
        for (uint32_t p = p0 + lane; p < p1; p += 64) { const uint32_t j = a.order[p]; if (edit_valid(a, i, j)) a.out[edit_out_index(a, i, j)] = a.len[j]; }
        return;
    }
    const uint8_t *q = a.codes + a.doff[i];
    if (cls != 2) {
        uint32_t P = 1;
        while (P < B) P <<= 1;
        const uint32_t G = 64 / P, g = lane / P, b = lane & (P - 1);
        const uint32_t hb = b + 1 == B ? (m - 1) & 31 : 31;
        edit_build_peq(edit_lds, q, m, 0, B, P, a.sigma, lane);
        uint32_t pos = p0 + g;
        for (;;) {
            while (pos < p1 && !edit_valid(a, i, a.order[pos])) pos += G;
            const bool has = pos < p1;
            if (!__any(has)) break;
            const uint32_t j = has ? a.order[pos] : 0u, n = has ? a.len[j] : 0u;
            pos += G;
            uint32_t score = m;
            edit_run_strip(edit_lds, B, P, b, hb, n, wave_max(n), a.codes + a.doff[j], false, false, nullptr, nullptr, score);
            if (has && b + 1 == B) a.out[edit_out_index(a, i, j)] = score;
        }
        return;
    }
    // several strips: one pair at a time, the deltas between strips in two planes behind the table
    const uint32_t nstrips = (B + a.strip - 1) / a.strip;
    uint32_t *pp = edit_lds + a.sigma * a.strip, *pm = pp + a.plane_words;
    for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t j = a.order[p];
        if (!edit_valid(a, i, j)) continue;
        const uint32_t n = a.len[j];
        uint32_t score = m;
        for (uint32_t s = 0; s < nstrips && n; ++s) {
            const uint32_t blk0 = s * a.strip, nblk = min(a.strip, B - blk0);
            const uint32_t hb = blk0 + lane + 1 == B ? (m - 1) & 31 : 31;
            edit_build_peq(edit_lds, q, m, blk0, nblk, a.strip, a.sigma, lane);
            edit_run_strip(edit_lds, nblk, a.strip, lane, hb, n, n, a.codes + a.doff[j], s > 0, s + 1 < nstrips, pp, pm, score);
        }
        const uint32_t lastb = B - (nstrips - 1) * a.strip - 1;
        if (lane == lastb) a.out[edit_out_index(a, i, j)] = score;
    }
}

// bytes -> dense codes in order of byte value; one workgroup per record, the pad behind a record stays 0
__global__ __launch_bounds__(256) void edit_recode_kernel(const uint8_t *raw, const uint64_t *off, const uint64_t *doff, const uint8_t *map, uint8_t *codes, uint32_t N) {
    __shared__ uint8_t lut[256];
    lut[threadIdx.x] = map[threadIdx.x];
    __syncthreads();
    for (uint32_t i = blockIdx.x; i < N; i += gridDim.x) {
        const uint64_t s = off[i], n = off[i + 1] - s, d = doff[i];
        for (uint64_t e = threadIdx.x; e < n; e += 256) codes[d + e] = lut[raw[s + e]];
    }
}

}  // namespace

void d2g_warm_edit() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&edit_pair_kernel));
}

namespace {

// blocks per strip: what 64 KiB of LDS hold of the table once the planes of the longest column are set aside (a query of one strip has none)
uint32_t edit_strip_blocks(const d2g_ctx *ctx, const d2g_seqset *ss, uint32_t *plane_words) {
    const uint32_t Bmax = (ss->maxlen + 31) / 32, pw = std::max<uint32_t>(1, (ss->maxlen + 31) / 32);
    uint32_t strip = std::min<uint32_t>(64, EDIT_LDS_WORDS / ss->sigma);
    if (ctx->edit.strip > 0) strip = std::min<uint32_t>(strip, (uint32_t)ctx->edit.strip);
    if (Bmax > strip) strip = std::min<uint32_t>(strip, (EDIT_LDS_WORDS - 2 * pw) / ss->sigma);
    *plane_words = pw;
    return std::max<uint32_t>(strip, 1);
}

// columns: those of [b0, b1) (ut: every j > i) among the records at positions [p0, p1) of the order by length
int edit_launch(d2g_ctx *ctx, const d2g_seqset *ss, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, int ut, uint32_t *out, hipStream_t s, uint32_t p0, uint32_t p1) {
    uint32_t pw = 0;
    const uint32_t strip = edit_strip_blocks(ctx, ss, &pw);
    uint32_t cmax[3] = {0, 0, 0};                                // the most blocks of a row of each class; 0: no such row
    bool have[3] = {false, false, false};
    for (uint32_t i = a0; i < a1; ++i) {
        const uint32_t B = (ss->len[i] + 31) / 32, c = B <= (uint32_t)EDIT_SMALL_BLOCKS && B <= strip ? 0 : B <= strip ? 1 : 2;
        have[c] = true; cmax[c] = std::max(cmax[c], B);
    }
    static const uint32_t kTile[3] = {512, 64, 8};
    d2g_timer tm(ctx, &ctx->ev_edit, s);
    for (uint32_t c = 0; c < 3; ++c) {
        if (!have[c]) continue;
        EditArgs a{ss->codes, ss->doff, ss->dlen, ss->order, (uint32_t)ss->N, ss->sigma, a0, a1, b0, b1, a0, 0, 0, c, strip, pw, ut, out};
        if (p0 != 0 || p1 != ss->N) { a.order = ss->order.get() + p0; a.N = p1 - p0; }   // (rect only: the triangle's index needs the true N)
        a.tile = ctx->edit.tile > 0 ? (uint32_t)ctx->edit.tile : kTile[c];
        a.ntiles = div_up<uint32_t>(a.N, a.tile);
        uint32_t P = 1;                                              // the lanes of the class's widest pair: its table's stride
        while (P < cmax[c]) P <<= 1;
        const size_t lds = sizeof(uint32_t) * (c == 2 ? (size_t)ss->sigma * strip + 2 * (size_t)pw : (size_t)ss->sigma * P);
        if (lds > sizeof(uint32_t) * EDIT_LDS_WORDS) { ctx->last_error = "d2g_edit: the match table does not fit in LDS"; return D2G_ERR_INTERNAL; }
        const uint32_t rows_per = std::max<uint32_t>(1, ctx->limits.edit_grid_max / a.ntiles);
        for (uint32_t r = a0; r < a1; r += rows_per) {
            a.row0 = r;
            const uint32_t nr = std::min(rows_per, a1 - r);
            hipLaunchKernelGGL(edit_pair_kernel, dim3(nr * a.ntiles), dim3(64), lds, s, a);
        }
    }
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

}  // namespace

int d2g_edit_rect_window(d2g_ctx *ctx, const d2g_seqset *ss, uint32_t a0, uint32_t a1, uint32_t p0, uint32_t p1, uint32_t *out, hipStream_t s) {
    if (a0 >= a1 || p0 >= p1) return D2G_OK;
    return edit_launch(ctx, ss, a0, a1, 0, (uint32_t)ss->N, 0, out, s, p0, p1);
}

extern "C" {

int d2g_seqset_create(d2g_ctx *ctx, const uint8_t *bytes, const uint64_t *off, size_t nrec, uint64_t nbytes, d2g_seqset **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    char err[200] = "";
    if (int rc = d2g_seqset_check(bytes, off, nrec, nbytes, err, sizeof err)) { ctx->last_error = err; return rc; }
    D2G_CHECK(ctx, nrec < (1ull << 31), "d2g_seqset: too many records");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<d2g_seqset> ss(new (std::nothrow) d2g_seqset());
    if (!ss) return D2G_ERR_NOMEM;
    ss->ctx = ctx; ss->N = nrec; ss->nsym = nbytes;
    uint8_t map[256];
    ss->sigma = (uint32_t)d2g_seqset_recode_map(bytes, nbytes, map);
    std::vector<uint64_t> doff(nrec + 1, 0);
    ss->len.resize(nrec);
    for (size_t i = 0; i < nrec; ++i) {
        ss->len[i] = (uint32_t)(off[i + 1] - off[i]);
        ss->maxlen = std::max(ss->maxlen, ss->len[i]);
        doff[i + 1] = doff[i] + div_up<uint64_t>(ss->len[i], EDIT_PAD) * EDIT_PAD;
    }
    ss->padded = doff[nrec] + EDIT_PAD;
    std::vector<uint32_t> order(nrec);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ss->len[x] < ss->len[y]; });
    ss->sorted_len.resize(nrec);
    for (size_t p = 0; p < nrec; ++p) ss->sorted_len[p] = ss->len[order[p]];
    ss->bytes = ss->padded + (nrec + 1) * sizeof(uint64_t) + 2 * std::max<size_t>(nrec, 1) * sizeof(uint32_t);
    const size_t staging = std::max<uint64_t>(nbytes, 1) + (nrec + 1) * sizeof(uint64_t) + 256;
    size_t free_b = 0, total_b = 0;
    D2G_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    if (ss->bytes + staging > free_b) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "d2g_seqset: the records need %zu bytes of device memory, %zu are free (no out-of-core path)", ss->bytes + staging, free_b);
        ctx->last_error = msg;
        return D2G_ERR_NOMEM;
    }
    d2g_dev<uint8_t> raw, dmap;
    d2g_dev<uint64_t> roff;
    if (int rc = ss->codes.alloc(ctx, ss->padded, "d2g_seqset codes")) return rc;
    if (int rc = ss->doff.alloc(ctx, nrec + 1, "d2g_seqset offsets")) return rc;
    if (int rc = ss->dlen.alloc(ctx, std::max<size_t>(nrec, 1), "d2g_seqset lengths")) return rc;
    if (int rc = ss->order.alloc(ctx, std::max<size_t>(nrec, 1), "d2g_seqset order")) return rc;
    if (int rc = raw.alloc(ctx, std::max<uint64_t>(nbytes, 1), "d2g_seqset staging")) return rc;
    if (int rc = roff.alloc(ctx, nrec + 1, "d2g_seqset staging offsets")) return rc;
    if (int rc = dmap.alloc(ctx, 256, "d2g_seqset code table")) return rc;
    const uint64_t zero = 0;
    {
        d2g_timer tm(ctx, &ctx->ev_editprep, nullptr);
        if (nbytes) D2G_HIP(ctx, hipMemcpyAsync(raw, bytes, nbytes, hipMemcpyHostToDevice, nullptr));
        D2G_HIP(ctx, hipMemcpyAsync(roff, nrec ? off : &zero, (nrec + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, nullptr));
        D2G_HIP(ctx, hipMemcpyAsync(ss->doff, doff.data(), (nrec + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, nullptr));
        D2G_HIP(ctx, hipMemcpyAsync(dmap, map, 256, hipMemcpyHostToDevice, nullptr));
        if (nrec) D2G_HIP(ctx, hipMemcpyAsync(ss->dlen, ss->len.data(), nrec * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
        if (nrec) D2G_HIP(ctx, hipMemcpyAsync(ss->order, order.data(), nrec * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
        D2G_HIP(ctx, hipMemsetAsync(ss->codes, 0, ss->padded, nullptr));
        if (nrec) hipLaunchKernelGGL(edit_recode_kernel, dim3((unsigned)std::min<size_t>(nrec, (size_t)ctx->num_cus * 8)), dim3(256), 0, nullptr, raw.get(), roff.get(),
                                     ss->doff.get(), dmap.get(), ss->codes.get(), (uint32_t)nrec);
        tm.stop();
    }
    D2G_HIP(ctx, hipGetLastError());
    D2G_HIP(ctx, hipStreamSynchronize(nullptr));
    *out = ss.release();
    return D2G_OK;
}

void   d2g_seqset_destroy(d2g_seqset *ss) { delete ss; }
size_t d2g_seqset_nrecords(const d2g_seqset *ss) { return ss ? ss->N : 0; }
size_t d2g_seqset_device_bytes(const d2g_seqset *ss) { return ss ? ss->bytes : 0; }
int    d2g_seqset_alphabet_size(const d2g_seqset *ss) { return ss ? (int)ss->sigma : D2G_ERR_INVALID; }
int    d2g_seqset_strip_blocks(const d2g_ctx *ctx, const d2g_seqset *ss) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    uint32_t pw;
    return (int)edit_strip_blocks(ctx, ss, &pw);
}

int d2g_edit_ut_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, uint32_t *out_dev, void *stream) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= ss->N, "d2g_edit_ut_dev: rows out of range");
    const size_t nout = d2g_ut_count(ss->N, r0, r1);
    if (nout == 0) return D2G_OK;
    D2G_CHECK(ctx, out_dev != nullptr, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rl = std::min(r1, ss->N - 1);                 // the last row has no pair
    return edit_launch(ctx, ss, (uint32_t)r0, (uint32_t)rl, (uint32_t)r0 + 1, (uint32_t)ss->N, 1, out_dev, as_stream(stream), 0, (uint32_t)ss->N);
}

int d2g_edit_rect_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t a0, size_t a1, size_t b0, size_t b1, uint32_t *out_dev, void *stream) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, a0 <= a1 && a1 <= ss->N && b0 <= b1 && b1 <= ss->N, "d2g_edit_rect_dev: block out of range");
    if (a0 == a1 || b0 == b1) return D2G_OK;
    D2G_CHECK(ctx, out_dev != nullptr, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    return edit_launch(ctx, ss, (uint32_t)a0, (uint32_t)a1, (uint32_t)b0, (uint32_t)b1, 0, out_dev, as_stream(stream), 0, (uint32_t)ss->N);
}

// host-pointer forms: the distances of the range to `out`; synchronise
int d2g_edit_ut(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, uint32_t *out) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= ss->N, "d2g_edit_ut: rows out of range");
    const size_t nout = d2g_ut_count(ss->N, r0, r1);
    if (nout == 0) return D2G_OK;
    D2G_CHECK(ctx, out != nullptr, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    d2g_dev<uint32_t> d;
    if (int rc = d.alloc(ctx, nout, "d2g_edit_ut output")) return rc;
    if (int rc = d2g_edit_ut_dev(ctx, ss, r0, r1, d, nullptr)) return rc;
    D2G_HIP(ctx, hipMemcpy(out, d, nout * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return D2G_OK;
}

int d2g_edit_rect(d2g_ctx *ctx, const d2g_seqset *ss, size_t a0, size_t a1, size_t b0, size_t b1, uint32_t *out) {
    if (!ctx || !ss) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ss->ctx == ctx, "d2g_seqset belongs to another context");
    D2G_CHECK(ctx, a0 <= a1 && a1 <= ss->N && b0 <= b1 && b1 <= ss->N, "d2g_edit_rect: block out of range");
    if (a0 == a1 || b0 == b1) return D2G_OK;
    D2G_CHECK(ctx, out != nullptr, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nout = (a1 - a0) * (b1 - b0);
    d2g_dev<uint32_t> d;
    if (int rc = d.alloc(ctx, nout, "d2g_edit_rect output")) return rc;
    if (int rc = d2g_edit_rect_dev(ctx, ss, a0, a1, b0, b1, d, nullptr)) return rc;
    D2G_HIP(ctx, hipMemcpy(out, d, nout * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return D2G_OK;
}

}  // extern "C"
