// d2g_kset_cmp.hip -- K2g: exact intersections of resident, sorted k-mer sets (--set, --countdict) on gfx950.
//
// Replaces, for every pair, weighted_compare on two files (reference src/wcompare.cpp:145-187; opened, merged with one 8-byte fread per
// element and closed per pair by compare(), src/cmp_core.cpp:527-569): isz(i, j) = sum over the keys both sets hold of min(w_i, w_j),
// w = 1 under --set and the k-mer's count under --countdict.  An integer; the device returns it as u64, exactly.  No floating point here:
// the measure is the host's d2g_epilogue_exact*.
//
// Keys are Wang hashes, uniform over 2^64, so the key space is cut by the top p bits into P = 2^p ranges ("slices") that every set is cut
// at alike (kset_slice_kernel: slice_off[N][P + 1], one binary search per boundary, once per d2g_kset).  p aims at a mean slice of
// 256 .. 512 keys for the LARGEST set, so that a slice of any set nearly always fits one LDS chunk of KSET_CHUNK = 1024 keys.
// kset_pair_kernel: a workgroup of four waves takes a tile of KSET_TW = 4 row sets x 4 column sets and a range of slices.  Per slice it
// stages the slice of each of the four column sets in LDS (keys and, weighted, counts); wave w then reads the slice of row set w from
// memory once, one key per lane, and looks every key up in the four staged slices by binary search.  The sums of a (row, column) pair
// stay in registers as u64 per lane and are reduced over the wave at the end.  A column slice longer than the chunk is staged in rounds of
// 1024 keys, by POSITION; the row slice is walked again in every round and a key that is not in the staged part is simply not found, so
// there is no seam by key value to get wrong, at the price of re-reading the row slice (from L2) in the rare extra round.
// Where the tiles are too few to fill the machine, the slice range is split over gridDim.z workgroups that add into a zeroed output with
// 64-bit integer atomics (sums of integers: order-free, still exact); otherwise every output word is stored once, plainly.
#include "d2g_internal.h"
#include <algorithm>
#include <cstdio>
#include <new>
#include <vector>

namespace {

constexpr int KSET_TW = 4;             // sets per tile side: one wave per row set
constexpr int KSET_CHUNK = 1024;       // keys of one column set staged per round
constexpr int KSET_THREADS = 64 * KSET_TW;
constexpr int KSET_SLICE_KEYS = 512;   // mean keys per slice of the largest set: at most this, more than half of it
constexpr int KSET_MAX_PBITS = 20;

struct KsetArgs {
    const uint64_t *keys; const uint32_t *counts;
    const uint64_t *slice_off;         // [N][P + 1], absolute positions in keys
    uint32_t P, N;
    uint32_t a0, a1, b0, b1;           // row sets [a0, a1), column sets [b0, b1)
    int ut;                            // 1: only pairs column > row, condensed upper-triangle output of rows [a0, a1) (b0 = a0 + 1, b1 = N)
    int atomic;                        // 1: add into a zeroed output; 0: store
    uint64_t *out;
};

__global__ __launch_bounds__(256) void kset_slice_kernel(const uint64_t *keys, const uint64_t *off, uint64_t *slice_off, uint32_t N, uint32_t p) {
    const uint64_t P1 = (1ull << p) + 1;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)N * P1) return;
    const uint32_t i = (uint32_t)(t / P1);
    const uint64_t s = t % P1;
    uint64_t lo = off[i], hi = off[i + 1];
    if (s == P1 - 1) lo = hi;                                   // the end of the last slice
    else if (s > 0) {
        const uint64_t bound = s << (64 - p);                   // first key of slice s (p >= 1 here)
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < bound) lo = mid + 1; else hi = mid; }
    }
    slice_off[t] = lo;
}

template <bool W> struct KsetLds {
    uint64_t key[KSET_TW][KSET_CHUNK];
    uint32_t cnt[W ? KSET_TW : 1][W ? KSET_CHUNK : 1];
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down((unsigned long long)v, o);
    return v;                                                    // lane 0 holds the sum
}

template <bool W>
__global__ __launch_bounds__(KSET_THREADS) void kset_pair_kernel(KsetArgs a) {
    __shared__ KsetLds<W> sh;
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint32_t ra = a.a0 + blockIdx.y * KSET_TW, cb = a.b0 + blockIdx.x * KSET_TW;
    const uint32_t nrows = min((uint32_t)KSET_TW, a.a1 - ra), ncols = min((uint32_t)KSET_TW, a.b1 - cb);
    if (a.ut && cb + ncols - 1 <= ra) return;                    // no pair of this tile has column > row
    const uint32_t s0 = (uint32_t)((uint64_t)a.P * blockIdx.z / gridDim.z), s1 = (uint32_t)((uint64_t)a.P * (blockIdx.z + 1) / gridDim.z);
    const size_t P1 = (size_t)a.P + 1;
    const uint32_t i = ra + w;
    const bool row = w < nrows;
    uint64_t acc[KSET_TW] = {0, 0, 0, 0};
    for (uint32_t s = s0; s < s1; ++s) {
        uint64_t clo[KSET_TW], clen[KSET_TW], longest = 0;
#pragma unroll
        for (uint32_t c = 0; c < KSET_TW; ++c) {
            clo[c] = clen[c] = 0;
            if (c < ncols) { clo[c] = a.slice_off[(cb + c) * P1 + s]; clen[c] = a.slice_off[(cb + c) * P1 + s + 1] - clo[c]; }
            longest = max(longest, clen[c]);
        }
        uint64_t rlo = 0, rhi = 0;
        if (row) { rlo = a.slice_off[i * P1 + s]; rhi = a.slice_off[i * P1 + s + 1]; }
        for (uint64_t base = 0; base < longest; base += KSET_CHUNK) {       // uniform over the workgroup
            uint32_t staged[KSET_TW];
            __syncthreads();                                                 // the previous round's searches are done
#pragma unroll
            for (uint32_t c = 0; c < KSET_TW; ++c) {
                staged[c] = clen[c] > base ? (uint32_t)min((uint64_t)KSET_CHUNK, clen[c] - base) : 0u;
                for (uint32_t e = tid; e < staged[c]; e += KSET_THREADS) {
                    sh.key[c][e] = a.keys[clo[c] + base + e];
                    if constexpr (W) sh.cnt[c][e] = a.counts[clo[c] + base + e];
                }
            }
            __syncthreads();
            for (uint64_t e = rlo + lane; e < rhi; e += 64) {
                const uint64_t key = a.keys[e];
                uint32_t rw = 1;
                if constexpr (W) rw = a.counts[e];
#pragma unroll
                for (uint32_t c = 0; c < KSET_TW; ++c) {
                    if (staged[c] == 0 || (a.ut && cb + c <= i)) continue;
                    uint32_t lo = 0, hi = staged[c];
                    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sh.key[c][mid] < key) lo = mid + 1; else hi = mid; }
                    if (lo < staged[c] && sh.key[c][lo] == key) {
                        if constexpr (W) acc[c] += min(rw, sh.cnt[c][lo]); else acc[c] += 1;
                    }
                }
            }
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < KSET_TW; ++c) {
        const uint64_t v = wave_sum(acc[c]);
        const uint32_t j = cb + c;
        if (lane != 0 || !row || c >= ncols || (a.ut && j <= i)) continue;
        size_t p;
        if (a.ut) {
            const uint64_t n = i - a.a0, tri1 = (uint64_t)i * (i ? i - 1 : 0) / 2, tri0 = (uint64_t)a.a0 * (a.a0 ? a.a0 - 1 : 0) / 2;
            p = n * ((uint64_t)a.N - 1) - (tri1 - tri0) + (j - i - 1);
        } else p = (size_t)(i - a.a0) * (a.b1 - a.b0) + (j - a.b0);
        if (a.atomic) { if (v) atomicAdd((unsigned long long *)&a.out[p], (unsigned long long)v); }
        else a.out[p] = v;
    }
}

}  // namespace

struct d2g_kset {
    d2g_ctx *ctx = nullptr;
    size_t N = 0;
    uint64_t total = 0;
    bool weighted = false;
    uint32_t p = 0;
    d2g_dev<uint64_t> keys;
    d2g_dev<uint32_t> counts;
    d2g_dev<uint64_t> off;             // [N + 1]
    d2g_dev<uint64_t> slice_off;       // [N][2^p + 1]
    size_t bytes = 0;
};

namespace {

uint32_t kset_pbits(const d2g_ctx *ctx, uint64_t longest) {
    if (ctx->kset.pbits >= 0) return (uint32_t)ctx->kset.pbits;
    uint32_t p = 0;
    while (p < (uint32_t)KSET_MAX_PBITS && (longest >> p) > (uint64_t)KSET_SLICE_KEYS) ++p;
    return p;
}

size_t kset_bytes(size_t N, uint64_t total, bool weighted, uint32_t p) {
    return total * sizeof(uint64_t) + (weighted ? total * sizeof(uint32_t) : 0) + (N + 1) * sizeof(uint64_t) + N * ((size_t(1) << p) + 1) * sizeof(uint64_t);
}

// buffers of a set whose N, total, weighted and p are known; refuses what does not fit, naming both figures
int kset_alloc(d2g_ctx *ctx, d2g_kset *ks) {
    ks->bytes = kset_bytes(ks->N, ks->total, ks->weighted, ks->p);
    size_t free_b = 0, total_b = 0;
    D2G_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    if (ks->bytes > free_b) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "d2g_kset: the sets need %zu bytes of device memory, %zu are free (no out-of-core path)", ks->bytes, free_b);
        ctx->last_error = msg;
        return D2G_ERR_NOMEM;
    }
    if (int rc = ks->keys.alloc(ctx, std::max<uint64_t>(ks->total, 1), "d2g_kset keys")) return rc;
    if (ks->weighted) if (int rc = ks->counts.alloc(ctx, std::max<uint64_t>(ks->total, 1), "d2g_kset counts")) return rc;
    if (int rc = ks->off.alloc(ctx, ks->N + 1, "d2g_kset offsets")) return rc;
    return ks->slice_off.alloc(ctx, ks->N * ((size_t(1) << ks->p) + 1), "d2g_kset slice table");
}

int kset_prepare(d2g_ctx *ctx, d2g_kset *ks, hipStream_t s) {
    const uint64_t nt = (uint64_t)ks->N * ((1ull << ks->p) + 1);
    D2G_CHECK(ctx, div_up<uint64_t>(nt, 256) < (1ull << 31), "d2g_kset: slice table too large");
    d2g_timer tm(ctx, &ctx->ev_ksetprep, s);
    hipLaunchKernelGGL(kset_slice_kernel, dim3((unsigned)div_up<uint64_t>(nt, 256)), dim3(256), 0, s, ks->keys.get(), ks->off.get(), ks->slice_off.get(),
                       (uint32_t)ks->N, ks->p);
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

int kset_launch(d2g_ctx *ctx, const d2g_kset *ks, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, int ut, size_t nout, uint64_t *out, hipStream_t s) {
    const uint32_t nrt = div_up<uint32_t>(a1 - a0, KSET_TW), nct = div_up<uint32_t>(b1 - b0, KSET_TW), P = 1u << ks->p;
    D2G_CHECK(ctx, nrt <= 65535, "d2g_kset: too many row sets in one launch (at most 262140)");
    const uint64_t tiles = (uint64_t)nrt * nct / (ut ? 2 : 1) + 1;
    uint32_t nsplit = (uint32_t)std::min<uint64_t>(P, div_up<uint64_t>((uint64_t)ctx->num_cus * 4, tiles));
    if (ctx->kset.split) nsplit = std::min<uint32_t>(P, (uint32_t)ctx->kset.split);
    KsetArgs a{ks->keys, ks->counts, ks->slice_off, P, (uint32_t)ks->N, a0, a1, b0, b1, ut, 0, out};
    a.atomic = ctx->kset.split ? ctx->kset.split >= 2 : nsplit > 1;
    if (a.atomic) D2G_HIP(ctx, hipMemsetAsync(out, 0, nout * sizeof(uint64_t), s));
    d2g_timer tm(ctx, &ctx->ev_kset, s);
    hipLaunchKernelGGL(ks->weighted ? kset_pair_kernel<true> : kset_pair_kernel<false>, dim3(nct, nrt, nsplit), dim3(KSET_THREADS), 0, s, a);
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

}  // namespace

void d2g_warm_kset() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&kset_slice_kernel));
}

extern "C" {

int d2g_kset_create(d2g_ctx *ctx, const uint64_t *keys, const uint32_t *counts, const uint64_t *set_off, size_t nsets, d2g_kset **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    char err[200] = "";
    if (d2g_kset_check(keys, counts, set_off, nsets, err, sizeof err)) { ctx->last_error = err; return D2G_ERR_INVALID; }
    D2G_CHECK(ctx, nsets < (1ull << 31), "d2g_kset: too many sets");
    D2G_CHECK(ctx, nsets == 0 || set_off[0] == 0, "d2g_kset: set_off must begin at 0");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<d2g_kset> ks(new (std::nothrow) d2g_kset());
    if (!ks) return D2G_ERR_NOMEM;
    uint64_t longest = 0;
    for (size_t i = 0; i < nsets; ++i) longest = std::max(longest, set_off[i + 1] - set_off[i]);
    ks->ctx = ctx; ks->N = nsets; ks->total = nsets ? set_off[nsets] : 0; ks->weighted = counts != nullptr; ks->p = kset_pbits(ctx, longest);
    if (int rc = kset_alloc(ctx, ks.get())) return rc;
    const uint64_t zero = 0;
    if (ks->total) D2G_HIP(ctx, hipMemcpy(ks->keys, keys, ks->total * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (ks->total && counts) D2G_HIP(ctx, hipMemcpy(ks->counts, counts, ks->total * sizeof(uint32_t), hipMemcpyHostToDevice));
    D2G_HIP(ctx, hipMemcpy(ks->off, nsets ? set_off : &zero, (nsets + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (nsets) if (int rc = kset_prepare(ctx, ks.get(), nullptr)) return rc;
    D2G_HIP(ctx, hipStreamSynchronize(nullptr));
    *out = ks.release();
    return D2G_OK;
}

int d2g_kset_create_dev(d2g_ctx *ctx, const uint64_t *keys_dev, const uint32_t *counts_dev, const uint64_t *set_off_dev, size_t nsets, void *stream,
                        d2g_kset **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    D2G_CHECK(ctx, set_off_dev != nullptr, "d2g_kset: null set_off");
    D2G_CHECK(ctx, nsets < (1ull << 31), "d2g_kset: too many sets");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = as_stream(stream);
    std::vector<uint64_t> off(nsets + 1);
    D2G_HIP(ctx, hipMemcpyAsync(off.data(), set_off_dev, (nsets + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    uint64_t longest = 0;
    D2G_CHECK(ctx, off[0] == 0, "d2g_kset: set_off must begin at 0");
    for (size_t i = 0; i < nsets; ++i) {
        D2G_CHECK(ctx, off[i + 1] >= off[i], "d2g_kset: set_off decreases");
        longest = std::max(longest, off[i + 1] - off[i]);
    }
    D2G_CHECK(ctx, off[nsets] == 0 || keys_dev, "d2g_kset: null keys");
    std::unique_ptr<d2g_kset> ks(new (std::nothrow) d2g_kset());
    if (!ks) return D2G_ERR_NOMEM;
    ks->ctx = ctx; ks->N = nsets; ks->total = off[nsets]; ks->weighted = counts_dev != nullptr; ks->p = kset_pbits(ctx, longest);
    if (int rc = kset_alloc(ctx, ks.get())) return rc;
    if (ks->total) D2G_HIP(ctx, hipMemcpyAsync(ks->keys, keys_dev, ks->total * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    if (ks->total && counts_dev) D2G_HIP(ctx, hipMemcpyAsync(ks->counts, counts_dev, ks->total * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(ks->off, set_off_dev, (nsets + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    if (nsets) if (int rc = kset_prepare(ctx, ks.get(), s)) return rc;
    *out = ks.release();
    return D2G_OK;
}

void d2g_kset_destroy(d2g_kset *ks) { delete ks; }
size_t d2g_kset_size(const d2g_kset *ks) { return ks ? ks->N : 0; }
size_t d2g_kset_device_bytes(const d2g_kset *ks) { return ks ? ks->bytes : 0; }
int d2g_kset_slice_bits(const d2g_kset *ks) { return ks ? (int)ks->p : D2G_ERR_INVALID; }

int d2g_kset_isz_ut_dev(d2g_ctx *ctx, const d2g_kset *ks, size_t r0, size_t r1, uint64_t *out_dev, void *stream) {
    if (!ctx || !ks) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ks->ctx == ctx, "d2g_kset belongs to another context");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= ks->N, "d2g_kset_isz_ut_dev: rows out of range");
    const size_t nout = d2g_ut_count(ks->N, r0, r1);
    if (nout == 0) return D2G_OK;
    D2G_CHECK(ctx, out_dev != nullptr, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rl = std::min(r1, ks->N - 1);                 // the last row has no pair
    return kset_launch(ctx, ks, (uint32_t)r0, (uint32_t)rl, (uint32_t)r0 + 1, (uint32_t)ks->N, 1, nout, out_dev, as_stream(stream));
}

int d2g_kset_isz_rect_dev(d2g_ctx *ctx, const d2g_kset *ks, size_t a0, size_t a1, size_t b0, size_t b1, uint64_t *out_dev, void *stream) {
    if (!ctx || !ks) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, ks->ctx == ctx, "d2g_kset belongs to another context");
    D2G_CHECK(ctx, a0 <= a1 && a1 <= ks->N && b0 <= b1 && b1 <= ks->N, "d2g_kset_isz_rect_dev: block out of range");
    if (a0 == a1 || b0 == b1) return D2G_OK;
    D2G_CHECK(ctx, out_dev != nullptr, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    return kset_launch(ctx, ks, (uint32_t)a0, (uint32_t)a1, (uint32_t)b0, (uint32_t)b1, 0, (a1 - a0) * (b1 - b0), out_dev, as_stream(stream));
}

}  // extern "C"
