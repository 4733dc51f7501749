// d2g_k2_planes.hip -- K2 on truncated registers (gfx950): (#a>b, #a<b) of P-bit codes kept as bit planes.
//
// Replaces the compressed branch of the reference's compare() (src/cmp_core.cpp:362-405: sketch::eq::count_gtlt / count_eq on
// uint8/uint16/uint32 registers made by make_compressed, :209-322) inside emit_rectangular's row loops.
//
// Operand: W[tb][p][Nstride] u32 -- bit t%32 of word (tb = t/32, plane p, sketch j) is bit (P-1-p) of code (j, t): most
// significant plane first, registers past S coded 0 on both sides (equal, never counted).  About N * S * P/8 bytes, and ONE copy
// serves both sides: the wave's rows are PL_IW consecutive words of a plane (scalar loads, as in d2g_k2_bitslice.hip), its columns
// one coalesced dword per lane.
//
// Bit-serial comparator.  Most significant plane first it reads  gt |= eq & a & ~b;  eq &= ~(a ^ b)  -- four inputs in the first
// update.  Walked from the LEAST significant plane up, the same order is two three-input functions and needs no eq:
//     gt' = (a ^ b) ? a : gt        lt' = (a ^ b) ? b : lt
// (a more significant plane that differs overrides everything below it), one v_bitop3_b32 each.  Per pair and 32-register group:
// 2P bitop3 (the first plane is two plain ANDs) + 2 accumulating v_bcnt: (2P + 2) / 32 VALU operations per register pair.
#include "d2g_internal.h"
#include "d2g_k2.h"
#include "d2g_k2_shape.h"
#include <new>

namespace {

// Shape of a wave's block of the pair matrix, per code width: PL_IW rows x 64 * JR columns, and how many planes of a group are
// unrolled.  The defaults (8 x 256 everywhere) are what the test suite has run on.  Timed at N = 10 000, S = 1024 with tools/trunc_time.py on
// variants built with tools/build_variant.sh NAME -DD2G_PL_JR16=2 ... (that tool checks a variant's whole triangle against the direct kernel):
//   8 planes:  JR 4: 0.91 ms   JR 2: 0.95 ms
//   16 planes: JR 4: 1.98 ms   JR 2: 1.73 ms (all 16 planes unrolled: 98 VGPRs, but 20 SGPRs spilled; 8 unrolled: no spills, not timed)
//   32 planes: JR 4: 5.33 / 3.98 ms (8 / 32 planes unrolled)   JR 2: 4.55 / 3.39 ms
// The faster shapes at 16 and 32 planes are the next step: they have not been through the suite's row ranges and rectangles.
#ifndef D2G_PL_JR8
#define D2G_PL_JR8 4
#endif
#ifndef D2G_PL_JR16
#define D2G_PL_JR16 4
#endif
#ifndef D2G_PL_JR32
#define D2G_PL_JR32 4
#endif
#ifndef D2G_PL_UNROLL16
#define D2G_PL_UNROLL16 16
#endif
#ifndef D2G_PL_UNROLL32
#define D2G_PL_UNROLL32 8
#endif
constexpr int PL_THREADS = 256;
constexpr int PL_IW = 8;                 // rows per wave: one s_load_dwordx8 per plane
constexpr int PL_CB = 256;               // columns per workgroup tile (the tile grid's column unit)
template <int P> struct PlShape {
    static constexpr int JR = P == 8 ? D2G_PL_JR8 : P == 16 ? D2G_PL_JR16 : D2G_PL_JR32;     // 64-column groups per lane
    static constexpr int UNROLL = P == 8 ? 8 : P == 16 ? D2G_PL_UNROLL16 : D2G_PL_UNROLL32;
    static constexpr int WC = PL_CB / (64 * JR);       // waves side by side along the columns
    static constexpr int RB = (4 / WC) * PL_IW;        // rows per workgroup tile
};
constexpr size_t PL_SLACK = 64;          // words behind Npad in every plane: a wave's row words may start at N - 1

// inputs (a, b, c) = (0xF0, 0xCC, 0xAA)
constexpr unsigned BITOP3_GT = (0xF0 & ~0xCC & 0xFF) | (~(0xF0 ^ 0xCC) & 0xAA & 0xFF);   // (a & ~b) | (~(a ^ b) & c)
constexpr unsigned BITOP3_LT = (~0xF0 & 0xCC & 0xFF) | (~(0xF0 ^ 0xCC) & 0xAA & 0xFF);   // (~a & b) | (~(a ^ b) & c)

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef u32x8 __attribute__((aligned(4))) u32x8_u;

struct StoreEqOfGtLt {
    uint32_t *__restrict__ out;
    __device__ __forceinline__ void put2(size_t pos, uint32_t eq, uint32_t) const { out[pos] = eq; }
};

// ---------------------------------------------------------------- prepare: codes [N][S] -> W[tb][p][Nstride]
// one thread per (sketch j, 32-register group tb): 32 codes in, P words out (coalesced over j).  Every word of the operand is
// written, the slack and the padding sketches as zeros.
template <class T>
__global__ __launch_bounds__(256) void planes_prepare_kernel(const T *__restrict__ codes, size_t N, size_t S, size_t Nstride,
                                                             uint32_t *__restrict__ W) {
    constexpr int P = 8 * sizeof(T);
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t tb = blockIdx.y;
    if (j >= Nstride) return;
    uint32_t w[P];
#pragma unroll
    for (int p = 0; p < P; ++p) w[p] = 0;
    if (j < N) {
        const T *row = codes + j * S + tb * 32;
        const size_t left = S - tb * 32;
        for (int t = 0; t < 32; ++t) {
            const uint32_t c = (size_t)t < left ? (uint32_t)row[t] : 0u;
#pragma unroll
            for (int p = 0; p < P; ++p) w[p] |= ((c >> (P - 1 - p)) & 1u) << t;
        }
    }
    uint32_t *dst = W + tb * P * Nstride + j;
#pragma unroll
    for (int p = 0; p < P; ++p) dst[(size_t)p * Nstride] = w[p];
}

// ---------------------------------------------------------------- pair kernel
template <int P, class Store>
__global__ __launch_bounds__(PL_THREADS) void k2_planes_kernel(const uint32_t *__restrict__ W, size_t Nstride, int ntb, uint32_t S,
                                                               PairShape sh, Store store) {
    constexpr int PL_JR = PlShape<P>::JR, PL_WC = PlShape<P>::WC, PL_RB = PlShape<P>::RB, PL_UNROLL = PlShape<P>::UNROLL;
    unsigned ct, rt;
    if (!tile_of_block(sh, blockIdx.x, ct, rt)) return;
    const size_t i0 = sh.i_lo + (size_t)rt * PL_RB;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const size_t iw0 = i0 + (size_t)(wave / PL_WC) * PL_IW;
    const size_t j0 = (size_t)(sh.ct0 + ct) * PL_CB + (size_t)(wave % PL_WC) * (64 * PL_JR);
    if (iw0 >= sh.i_hi) return;
    if (sh.ut && j0 + 64 * PL_JR - 1 <= iw0) return;

    uint32_t accg[PL_IW][PL_JR], accl[PL_IW][PL_JR];
#pragma unroll
    for (int i = 0; i < PL_IW; ++i)
#pragma unroll
        for (int c = 0; c < PL_JR; ++c) { accg[i][c] = 0; accl[i][c] = 0; }

    // iw0 + PL_IW <= Npad + PL_IW - 1 < Nstride and j0 + 64 * PL_JR - 1 < Npad: every word read lies inside its plane
    typedef const u32x8_u __attribute__((address_space(4))) *row_words_ptr;   // uniform address in constant space: a scalar load
    const uint32_t *arow = W + iw0;
    const uint32_t *bcol = W + j0 + lane;

    for (int tb = 0; tb < ntb; ++tb) {
        const size_t g = (size_t)tb * P * Nstride;
        uint32_t gt[PL_IW][PL_JR], lt[PL_IW][PL_JR];
        {   // least significant plane: nothing below it
            const size_t o = g + (size_t)(P - 1) * Nstride;
            const u32x8_u a = *(row_words_ptr)(uintptr_t)(arow + o);
            uint32_t b[PL_JR];
#pragma unroll
            for (int c = 0; c < PL_JR; ++c) b[c] = bcol[o + 64 * c];
#pragma unroll
            for (int i = 0; i < PL_IW; ++i)
#pragma unroll
                for (int c = 0; c < PL_JR; ++c) { gt[i][c] = a[i] & ~b[c]; lt[i][c] = ~a[i] & b[c]; }
        }
#pragma unroll PL_UNROLL
        for (int p = P - 2; p >= 0; --p) {
            const size_t o = g + (size_t)p * Nstride;
            const u32x8_u a = *(row_words_ptr)(uintptr_t)(arow + o);
            uint32_t b[PL_JR];
#pragma unroll
            for (int c = 0; c < PL_JR; ++c) b[c] = bcol[o + 64 * c];
#pragma unroll
            for (int i = 0; i < PL_IW; ++i)
#pragma unroll
                for (int c = 0; c < PL_JR; ++c) {
                    gt[i][c] = __builtin_amdgcn_bitop3_b32(a[i], b[c], gt[i][c], BITOP3_GT);
                    lt[i][c] = __builtin_amdgcn_bitop3_b32(a[i], b[c], lt[i][c], BITOP3_LT);
                }
        }
#pragma unroll
        for (int i = 0; i < PL_IW; ++i)
#pragma unroll
            for (int c = 0; c < PL_JR; ++c) {
                accg[i][c] += __builtin_popcount(gt[i][c]);
                accl[i][c] += __builtin_popcount(lt[i][c]);
            }
    }

#pragma unroll
    for (int i = 0; i < PL_IW; ++i) {
        const size_t ii = iw0 + i;
        if (ii >= sh.i_hi) break;
#pragma unroll
        for (int c = 0; c < PL_JR; ++c) {
            const size_t jj = j0 + lane + 64 * c;
            if (jj < sh.j_hi && jj >= sh.j_lo && (!sh.ut || jj > ii))
                store.put2(out_pos(sh, ii, jj), S - accg[i][c] - accl[i][c], accg[i][c]);
        }
    }
}

template <int P, class Store>
void launch_planes_p(const d2g_cmp_set *set, const PairShape &sh, Store store, hipStream_t s) {
    hipLaunchKernelGGL((k2_planes_kernel<P, Store>), dim3(sh.per_xcd * 8), dim3(PL_THREADS), 0, s, set->d_cplanes.get(), set->Nstride,
                       set->ntb, (uint32_t)set->S, sh, store);
}

template <class Store>
int launch_planes(d2g_ctx *ctx, const d2g_cmp_set *set, PairShape sh, Store store, hipStream_t s) {
    const unsigned rb = set->cplanes == 8 ? PlShape<8>::RB : set->cplanes == 16 ? PlShape<16>::RB : PlShape<32>::RB;
    if (int rc = finish_shape(ctx, sh, rb)) return rc;
    if (sh.nvalid_total == 0) return D2G_OK;
    d2g_timer tm(ctx, &ctx->ev_k2, s);
    if (set->cplanes == 8) launch_planes_p<8>(set, sh, store, s);
    else if (set->cplanes == 16) launch_planes_p<16>(set, sh, store, s);
    else launch_planes_p<32>(set, sh, store, s);
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

}  // namespace

int d2g_planes_gtlt(d2g_ctx *ctx, const d2g_cmp_set *set, const PairShape &sh, uint32_t *gt, uint32_t *lt, hipStream_t s) {
    return launch_planes(ctx, set, sh, StoreGtLt{gt, lt, (uint32_t)set->S}, s);
}
int d2g_planes_eq(d2g_ctx *ctx, const d2g_cmp_set *set, const PairShape &sh, uint32_t *eq, hipStream_t s) {
    return launch_planes(ctx, set, sh, StoreEqOfGtLt{eq}, s);
}

extern "C" {

int d2g_cmp_set_create_codes_dev(d2g_ctx *ctx, const void *codes_dev, size_t N, size_t S, int regbytes, void *stream, d2g_cmp_set **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    D2G_CHECK(ctx, N >= 1 && S >= 1, "cmp_set_codes: empty matrix");
    D2G_CHECK(ctx, N < (1ull << 30) && S < (1ull << 31), "cmp_set_codes: matrix too large");
    D2G_CHECK(ctx, codes_dev != nullptr, "cmp_set_codes: null codes");
    D2G_CHECK(ctx, regbytes == 1 || regbytes == 2 || regbytes == 4, "cmp_set_codes: register size must be 1, 2 or 4 bytes");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = as_stream(stream);
    std::unique_ptr<d2g_cmp_set, void (*)(d2g_cmp_set *)> set(new (std::nothrow) d2g_cmp_set(), d2g_cmp_set_destroy);
    if (!set) return D2G_ERR_NOMEM;
    set->ctx = ctx; set->N = N; set->S = S;
    set->Npad = div_up<size_t>(N, PL_CB) * PL_CB;
    set->Nstride = set->Npad + PL_SLACK;
    set->ntb = (int)div_up<size_t>(S, 32);
    set->cplanes = 8 * regbytes;
    set->algo = D2G_CMP_PLANES;
    if (int rc = set->d_cplanes.alloc(ctx, (size_t)set->ntb * set->cplanes * set->Nstride, "cmp_set_codes alloc")) return rc;
    const dim3 grid((unsigned)div_up<size_t>(set->Nstride, 256), (unsigned)set->ntb);
    D2G_CHECK(ctx, set->ntb <= 65535, "cmp_set_codes: sketchsize too large");
    d2g_timer tm(ctx, &ctx->ev_k2prep, s);
    if (regbytes == 1)
        hipLaunchKernelGGL(planes_prepare_kernel<uint8_t>, grid, dim3(256), 0, s, static_cast<const uint8_t *>(codes_dev), N, S, set->Nstride, set->d_cplanes.get());
    else if (regbytes == 2)
        hipLaunchKernelGGL(planes_prepare_kernel<uint16_t>, grid, dim3(256), 0, s, static_cast<const uint16_t *>(codes_dev), N, S, set->Nstride, set->d_cplanes.get());
    else
        hipLaunchKernelGGL(planes_prepare_kernel<uint32_t>, grid, dim3(256), 0, s, static_cast<const uint32_t *>(codes_dev), N, S, set->Nstride, set->d_cplanes.get());
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    *out = set.release();
    return D2G_OK;
}

int d2g_cmp_set_create_codes(d2g_ctx *ctx, const void *codes_host, size_t N, size_t S, int regbytes, d2g_cmp_set **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    D2G_CHECK(ctx, codes_host != nullptr && N >= 1 && S >= 1, "cmp_set_codes: bad host matrix");
    D2G_CHECK(ctx, regbytes == 1 || regbytes == 2 || regbytes == 4, "cmp_set_codes: register size must be 1, 2 or 4 bytes");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    d2g_dev<uint8_t> tmp;
    if (int rc = tmp.alloc(ctx, N * S * (size_t)regbytes, "cmp_set_codes staging alloc")) return rc;
    D2G_HIP(ctx, hipMemcpy(tmp, codes_host, N * S * (size_t)regbytes, hipMemcpyHostToDevice));
    const int rc = d2g_cmp_set_create_codes_dev(ctx, tmp, N, S, regbytes, nullptr, out);
    D2G_HIP(ctx, hipStreamSynchronize(nullptr));      // the staging buffer goes away
    return rc;
}

int d2g_cmp_dist_trunc_ut(d2g_ctx *ctx, const double *sigs, const double *cards, size_t N, size_t S, size_t r0, size_t r1,
                          int measure, int k, int regbytes, int bbit, int nthreads, float *out) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, measure >= D2G_SIMILARITY && measure <= D2G_UNION_SIZE, "cmp: unknown measure");
    D2G_CHECK(ctx, r0 <= r1 && r1 <= N, "cmp: row range out of bounds");
    D2G_CHECK(ctx, sigs != nullptr && N >= 1 && S >= 1, "cmp: bad host matrix");
    D2G_CHECK(ctx, regbytes == 1 || regbytes == 2 || regbytes == 4, "cmp: register size must be 1, 2 or 4 bytes");
    if (nthreads < 1) nthreads = 1;
    std::vector<uint8_t> codes(N * S * (size_t)regbytes);
    long double ab[2] = {0.L, 0.L};
    char err[160];
    if (int rc = d2g_regs_truncate(sigs, N, S, regbytes, bbit, codes.data(), ab, nullptr, nthreads, err, sizeof err)) {
        ctx->last_error = err;
        return rc;
    }
    const size_t cnt = d2g_ut_count(N, r0, r1);
    if (!cnt) return D2G_OK;
    D2G_CHECK(ctx, out != nullptr && cards != nullptr, "cmp: null output/cards");
    d2g_cmp_set *raw = nullptr;
    if (int rc = d2g_cmp_set_create_codes(ctx, codes.data(), N, S, regbytes, &raw)) return rc;
    const std::unique_ptr<d2g_cmp_set, void (*)(d2g_cmp_set *)> set(raw, d2g_cmp_set_destroy);
    d2g_dev<uint32_t> d_a, d_b;
    std::vector<uint32_t> ca(cnt), cb;
    if (int rc = d_a.alloc(ctx, cnt, "cmp output alloc")) return rc;
    if (bbit) {
        if (int rc = d2g_cmp_eqcount_ut_dev(ctx, set.get(), r0, r1, d_a, nullptr)) return rc;
        D2G_HIP(ctx, hipMemcpy(ca.data(), d_a, cnt * 4, hipMemcpyDeviceToHost));
    } else {
        if (int rc = d_b.alloc(ctx, cnt, "cmp output alloc")) return rc;
        if (int rc = d2g_cmp_gtlt_ut_dev(ctx, set.get(), r0, r1, d_a, d_b, nullptr)) return rc;
        cb.resize(cnt);
        D2G_HIP(ctx, hipMemcpy(ca.data(), d_a, cnt * 4, hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(cb.data(), d_b, cnt * 4, hipMemcpyDeviceToHost));
    }
    return d2g_epilogue_trunc_ut(ca.data(), bbit ? nullptr : cb.data(), cards, N, S, r0, r1, measure, k, regbytes,
                                 bbit ? nullptr : &ab[1], nthreads, out);
}

}  // extern "C"

void d2g_warm_k2_planes() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&planes_prepare_kernel<uint8_t>));
}
