// d2g_k3_lists.hip -- BagMinHash (BMH-D2G, the process machinery of d2g_k3_device.h) over explicit (id, weight) lists in device memory:
// the list stage every producer of such lists goes through (k3_lists_prepare / k3_lists_walk, d2g_k3.h), the host-array entry points
// d2g_bmh_from_weighted*, and d2g_bmh_device_lists for lists another unit left on the device (K1i's interval runs; K3k calls the stage itself).
#include "d2g_k3_device.h"
#include <cmath>
#include <cstring>

namespace {

// ---------------------------------------------------------------------------------------------
// explicit weighted sets (wsketch.cpp:54-73 minwise_det / 17-51 rowwise CSR): elements come
// from (id, weight) arrays instead of the count table
// ---------------------------------------------------------------------------------------------
struct WsArgs {
    const uint64_t *ids;
    const double *w;             // nullptr => 1.0
    const uint32_t *blk_set;     // set of workgroup
    const uint64_t *blk_lo;      // first element
    const uint32_t *blk_cnt;     // element count
    uint32_t m;
    uint64_t *h;                 // [nsets][m]
    const uint64_t *guess;       // [nsets] pruning bound of this pass
    const uint32_t *redo;        // [nsets] (redo_mode) sets to walk again
    int redo_mode;
    int *status;
    uint64_t *arg;               // argmin pass: [nsets][m] owner positions, pre-set to ~0
    const uint64_t *set_lo;      // argmin pass: [nsets] first element of each set
};

__device__ __forceinline__ bool ws_fetch(const WsArgs &a, uint64_t idx, uint64_t &d, double &w, int *status) {
    d = a.ids[idx];
    w = a.w ? a.w[idx] : 1.0;
    if (!(w > 0.)) return false;                                   // BagMinHash2::update ignores w <= 0
    if (!(w <= 0x1p53)) { atomicExch(status, K3_BAD_WEIGHT); return false; }   // outside the level set (also NaN)
    return true;
}

__global__ __launch_bounds__(K3_THREADS) void k3_bmh_sets_kernel(WsArgs a) {
    const uint32_t set = a.blk_set[blockIdx.x];
    if (a.redo_mode && !a.redo[set]) return;
    const uint64_t lo = a.blk_lo[blockIdx.x], cnt = a.blk_cnt[blockIdx.x];
    const double bound = V(a.guess[set]);
    uint64_t *hg = a.h + (size_t)set * a.m;
    Proc stk[BMH_STACK];
    for (uint64_t e = threadIdx.x; e < cnt; e += K3_THREADS) {
        uint64_t d; double w;
        if (ws_fetch(a, lo + e, d, w, a.status)) walk_element(d, w, a.m, bound, hg, stk, a.status);
    }
}

// after the registers are final: one more walk under the verified bound records, per register, the position
// (within its set) of the element whose point it holds
__global__ __launch_bounds__(K3_THREADS) void k3_bmh_sets_argmin_kernel(WsArgs a) {
    const uint32_t set = a.blk_set[blockIdx.x];
    const uint64_t lo = a.blk_lo[blockIdx.x], cnt = a.blk_cnt[blockIdx.x];
    const double bound = V(a.guess[set]);
    Proc stk[BMH_STACK];
    for (uint64_t e = threadIdx.x; e < cnt; e += K3_THREADS) {
        uint64_t d; double w;
        if (ws_fetch(a, lo + e, d, w, a.status))
            walk_element(d, w, a.m, bound, ArgSink{a.h + (size_t)set * a.m, a.arg + (size_t)set * a.m, lo + e - a.set_lo[set]}, stk, a.status);
    }
}

// per set: max(h) <= guess ?  else raise the guess and flag the set
__global__ __launch_bounds__(K3_THREADS) void k3_sets_verify_kernel(const uint64_t *h, uint32_t m, uint64_t *guess, uint32_t *redo,
                                                                   const double *tw, uint32_t *nredo, int redo_mode) {
    __shared__ uint64_t red[8];
    const uint32_t set = blockIdx.x;
    if (redo_mode && !redo[set]) return;
    const uint64_t hm = block_hmax(h + (size_t)set * m, m, red);
    if (threadIdx.x == 0) {
        const double g = V(guess[set]);
        const bool bad = tw[set] > 0. && !(V(hm) <= g);
        redo[set] = bad;
        if (bad) { guess[set] = dbits(16. * g); atomicAdd(nredo, 1u); }
    }
}

// the first guess of every set's bound from its total weight, as bit patterns (0 for a set without weight: nothing is walked)
std::vector<uint64_t> ws_guesses(const double *tw, size_t nsets, size_t m, double scale) {
    std::vector<uint64_t> guess(nsets);
    const double lnm = std::log((double)m);
    for (size_t i = 0; i < nsets; ++i) {
        const double gv = tw[i] > 0. ? scale * bmh_guess(tw[i], (double)m, lnm) : 0.;
        std::memcpy(&guess[i], &gv, 8);
    }
    return guess;
}
// The passes over explicit sets whose lists, workgroup tables, guesses, total weights and +inf registers are ON THE DEVICE: every set
// under its guess, the verification, the sets that failed it again under a guess 16 times larger, until none is left.  Synchronises
// `s` once per pass, for the two words of d_status; *status_out: the status word as the last pass read it.
int ws_walk(d2g_ctx *ctx, hipStream_t s, WsArgs &a, size_t nsets, size_t nb, uint64_t *d_guess, uint32_t *d_redo, const double *d_tw, int *d_status,
            int *status_out) {
    for (int pass = 0;; ++pass) {
        a.redo_mode = pass > 0;
        if (nb) hipLaunchKernelGGL(k3_bmh_sets_kernel, dim3((unsigned)nb), dim3(K3_THREADS), 0, s, a);
        hipLaunchKernelGGL(k3_sets_verify_kernel, dim3((unsigned)nsets), dim3(K3_THREADS), 0, s, a.h, a.m, d_guess, d_redo, d_tw,
                           reinterpret_cast<uint32_t *>(d_status + 1), a.redo_mode);
        int st2[2] = {0, 0};
        D2G_HIP(ctx, hipMemcpyAsync(st2, d_status, sizeof(st2), hipMemcpyDeviceToHost, s));
        D2G_HIP(ctx, hipStreamSynchronize(s));
        *status_out = st2[0];
        if (st2[0] || !st2[1]) break;
        if (pass >= 40) { ctx->last_error = "internal: BagMinHash bound did not converge"; return D2G_ERR_INTERNAL; }
        D2G_HIP(ctx, hipMemsetAsync(d_status + 1, 0, sizeof(int), s));
    }
    return D2G_OK;
}

}  // namespace

// a first guess below 2^1024 / 16^40 = 2^864 stays finite through every pass of ws_walk (see d2g_bmh_check_weights)
constexpr double BMH_GUESS_LIMIT = 0x1p864;

int k3_lists_prepare(d2g_ctx *ctx, hipStream_t s, const uint64_t *ids_dev, const double *w_dev, const uint64_t *set_off, const double *tw,
                     size_t ng, size_t m, K3ListTables &t, const K3ListRegs &r, K3ListWalk *out) {
    const double scale = ctx->k3_tune.guess_scale, lnm = std::log((double)m);
    for (size_t i = 0; i < ng; ++i)      // d2g_bmh_check_weights' last check, on the totals
        D2G_CHECK(ctx, !(tw[i] > 0.) || scale * bmh_guess(tw[i], (double)m, lnm) < BMH_GUESS_LIMIT,
                  "BagMinHash: total weight too small for the sketch size (the pruning bound would not stay finite)");
    t.guess = ws_guesses(tw, ng, m, scale);
    d2g_ws_plan_blocks(set_off, ng, t.wb);
    const size_t nb = t.wb.set.size();
    D2G_CHECK(ctx, nb < (1ull << 31), "too many workgroups");
    if (int rc = t.lo.grow(ctx, std::max<size_t>(nb, 1), 4096, "weighted lists alloc")) return rc;
    if (int rc = t.set.grow(ctx, std::max<size_t>(2 * nb, 1), 4096, "weighted lists alloc")) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(r.tw, tw, ng * sizeof(double), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(r.guess, t.guess.data(), ng * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (nb) {
        D2G_HIP(ctx, hipMemcpyAsync(t.lo, t.wb.lo.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        D2G_HIP(ctx, hipMemcpyAsync(t.set, t.wb.set.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        D2G_HIP(ctx, hipMemcpyAsync(t.set + nb, t.wb.cnt.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    *out = K3ListWalk{ids_dev, w_dev, &t, r, ng, nb, m};
    return D2G_OK;
}

namespace {
// the kernel arguments of a prepared walk: the only place that fills them
WsArgs ws_args(const K3ListWalk &p) {
    WsArgs a;
    a.ids = p.ids; a.w = p.w; a.blk_set = p.t->set; a.blk_lo = p.t->lo; a.blk_cnt = p.t->set + p.nb;
    a.m = (uint32_t)p.m; a.h = p.r.h; a.guess = p.r.guess; a.redo = p.r.redo; a.redo_mode = 0; a.status = p.r.status;
    a.arg = nullptr; a.set_lo = nullptr;
    return a;
}
}  // namespace

int k3_lists_walk(d2g_ctx *ctx, hipStream_t s, const K3ListWalk &p) {
    WsArgs a = ws_args(p);
    int status = 0;
    if (int rc = ws_walk(ctx, s, a, p.ng, p.nb, p.r.guess, p.r.redo, p.r.tw, p.r.status, &status)) return rc;
    return k3_status_error(ctx, status);
}

extern "C" {

// Every host-side check of the weights of explicit sets, without a context.  The last one keeps the walk finite: a set's first guess of
// its bound is scale * bmh_guess(W), the redo loop of ws_walk multiplies a guess by 16 and gives up after 40 passes, so
// a first guess below 2^1024 / 16^40 = 2^864 (BMH_GUESS_LIMIT) stays finite through every pass.  An infinite bound prunes nothing
// (proc_next ends on P.x <= bound, which inf <= inf satisfies), and the walk of such a set would not end.
int d2g_bmh_check_weights(const double *weights, const uint64_t *set_off, size_t nsets, size_t sketchsize, double scale, char *err,
                          size_t errcap) {
    auto fail = [&](const char *fmt, unsigned long long set) {
        if (err && errcap) std::snprintf(err, errcap, fmt, set);
        return D2G_ERR_INVALID;
    };
    if (err && errcap) err[0] = 0;
    if (!set_off) return fail("null argument", 0);
    if (!(sketchsize >= 1 && sketchsize < (1ull << 24))) return fail("sketchsize out of range", 0);
    if (!(scale > 0.)) return fail("guess scale not positive", 0);
    for (size_t i = 0; i < nsets; ++i) if (!(set_off[i] <= set_off[i + 1])) return fail("set_off not monotone", 0);
    const double m = (double)sketchsize, lnm = std::log(m);
    for (size_t i = 0; i < nsets; ++i) {
        double t = 0.;
        for (uint64_t e = set_off[i]; e < set_off[i + 1]; ++e) {
            const double w = weights ? weights[e] : 1.0;
            if (w > 0.) {
                if (!(w <= 0x1p53)) return fail("BagMinHash weight outside (0, 2^53] (set %llu)", i);
                t += w;
            } else if (w != w) return fail("BagMinHash weight is NaN (set %llu)", i);
        }
        if (t > 0. && !(scale * bmh_guess(t, m, lnm) < BMH_GUESS_LIMIT))
            return fail("BagMinHash set %llu: total weight too small for the sketch size (the pruning bound would not stay finite)", i);
    }
    return D2G_OK;
}

int d2g_bmh_from_weighted(d2g_ctx *ctx, const uint64_t *ids, const double *weights, const uint64_t *set_off, size_t nsets,
                          size_t sketchsize, double *sig_out, double *total_weight_out) {
    return d2g_bmh_from_weighted_ids(ctx, ids, weights, set_off, nsets, sketchsize, sig_out, total_weight_out, nullptr);
}

int d2g_bmh_from_weighted_ids(d2g_ctx *ctx, const uint64_t *ids, const double *weights, const uint64_t *set_off, size_t nsets,
                              size_t sketchsize, double *sig_out, double *total_weight_out, uint64_t *owner_out) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set_off != nullptr && (nsets == 0 || (sig_out && total_weight_out)), "null argument");
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 24), "sketchsize out of range");
    D2G_CHECK(ctx, nsets < (1ull << 31), "too many sets");
    if (nsets == 0) return D2G_OK;
    const uint64_t total = set_off[nsets];
    D2G_CHECK(ctx, total == 0 || ids != nullptr, "null ids");
    {   // every check of the weights, before anything is allocated or launched
        char err[160];
        if (d2g_bmh_check_weights(weights, set_off, nsets, sketchsize, ctx->k3_tune.guess_scale, err, sizeof err) != D2G_OK) {
            ctx->last_error = err;
            return D2G_ERR_INVALID;
        }
    }
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const size_t m = sketchsize;
    // total weights on the host (the caller's arrays are host arrays): the result, and the first guess of the bound
    std::vector<double> tw(nsets, 0.);
    for (size_t i = 0; i < nsets; ++i) {
        const uint64_t lo = set_off[i], hi = set_off[i + 1];
        double t = 0.;
        for (uint64_t e = lo; e < hi; ++e) {
            const double w = weights ? weights[e] : 1.0;
            if (w > 0.) t += w;                                      // the same sum, in the same order, as d2g_bmh_check_weights
        }
        tw[i] = t;
    }
    d2g_dev<uint64_t> d_ids, d_h, d_guess, d_arg, d_setlo;
    d2g_dev<double> d_w, d_tw;
    d2g_dev<uint32_t> d_redo;
    d2g_dev<int> d_status;
    int rc = D2G_OK;
    const char *what = "weighted sets alloc";
    if ((rc = d_ids.alloc(ctx, std::max<uint64_t>(total, 1), what)) ||
        (rc = d_h.alloc(ctx, nsets * m, what)) ||
        (rc = d_guess.alloc(ctx, nsets, what)) ||
        (rc = d_redo.alloc(ctx, nsets, what)) ||
        (rc = d_tw.alloc(ctx, nsets, what)) ||
        (rc = d_status.alloc(ctx, 2, what))) return rc;
    if (weights) { if ((rc = d_w.alloc(ctx, std::max<uint64_t>(total, 1), what))) return rc; D2G_HIP(ctx, hipMemcpy(d_w, weights, total * 8, hipMemcpyHostToDevice)); }
    if (total) D2G_HIP(ctx, hipMemcpy(d_ids, ids, total * 8, hipMemcpyHostToDevice));
    D2G_HIP(ctx, hipMemset(d_status, 0, 2 * sizeof(int)));
    K3ListTables tabs;
    K3ListWalk walk;
    {
        d2g_timer tm(ctx, &ctx->ev_k3, nullptr);
        k3_init_registers(nullptr, d_h, nsets * m, d_tw, d_redo, nsets);
        rc = k3_lists_prepare(ctx, nullptr, d_ids, d_w, set_off, tw.data(), nsets, m, tabs, K3ListRegs{d_h, d_guess, d_redo, d_tw, d_status}, &walk);
        if (!rc) rc = k3_lists_walk(ctx, nullptr, walk);
        if (rc) { (void)hipStreamSynchronize(nullptr); return rc; }          // `tabs` and `tw` are read by copies that may still be in flight
        if (owner_out) {
            if ((rc = d_arg.alloc(ctx, nsets * m, what)) || (rc = d_setlo.alloc(ctx, nsets, what))) return rc;
            D2G_HIP(ctx, hipMemset(d_arg, 0xFF, nsets * m * 8));
            D2G_HIP(ctx, hipMemcpy(d_setlo, set_off, nsets * 8, hipMemcpyHostToDevice));
            WsArgs a = ws_args(walk);
            a.arg = d_arg; a.set_lo = d_setlo;
            if (walk.nb) hipLaunchKernelGGL(k3_bmh_sets_argmin_kernel, dim3((unsigned)walk.nb), dim3(K3_THREADS), 0, nullptr, a);
        }
        tm.stop();
    }
    D2G_HIP(ctx, hipGetLastError());
    int status = 0;                                                          // the owner pass walks once more: its status
    D2G_HIP(ctx, hipMemcpy(&status, d_status, sizeof(int), hipMemcpyDeviceToHost));
    D2G_HIP(ctx, hipMemcpy(sig_out, d_h, nsets * m * 8, hipMemcpyDeviceToHost));
    if (owner_out) D2G_HIP(ctx, hipMemcpy(owner_out, d_arg, nsets * m * 8, hipMemcpyDeviceToHost));
    std::memcpy(total_weight_out, tw.data(), nsets * sizeof(double));
    return k3_status_error(ctx, status);
}

}  // extern "C"

// BagMinHash over lists another unit left on the device (K1i's expanded interval runs, d2g_k1i.hip): d2g_bmh_from_weighted_ids without
// the upload of the lists and without the owner pass; the totals and the checks that need them come from the caller's host arrays.
int d2g_bmh_device_lists(d2g_ctx *ctx, hipStream_t s, const uint64_t *ids_dev, const double *w_dev, const uint64_t *set_off, const double *tw,
                         size_t ng, size_t m, double *sig_out, d2g_evlog *ev) {
    D2G_CHECK(ctx, m >= 1 && m < (1ull << 24), "sketchsize out of range");
    D2G_CHECK(ctx, ng < (1ull << 31), "too many sets");
    if (ng == 0) return D2G_OK;
    d2g_dev<uint64_t> d_h, d_guess;
    d2g_dev<double> d_tw;
    d2g_dev<uint32_t> d_redo;
    d2g_dev<int> d_status;
    int rc = D2G_OK;
    const char *what = "weighted lists alloc";
    if ((rc = d_h.alloc(ctx, ng * m, what)) || (rc = d_guess.alloc(ctx, ng, what)) || (rc = d_redo.alloc(ctx, ng, what)) ||
        (rc = d_tw.alloc(ctx, ng, what)) || (rc = d_status.alloc(ctx, 2, what))) return rc;
    D2G_HIP(ctx, hipMemsetAsync(d_status, 0, 2 * sizeof(int), s));
    K3ListTables tabs;
    K3ListWalk walk;
    {
        d2g_timer tm(ctx, ev, s);
        k3_init_registers(s, d_h, ng * m, d_tw, d_redo, ng);
        rc = k3_lists_prepare(ctx, s, ids_dev, w_dev, set_off, tw, ng, m, tabs, K3ListRegs{d_h, d_guess, d_redo, d_tw, d_status}, &walk);
        if (!rc) rc = k3_lists_walk(ctx, s, walk);
        tm.stop();
    }
    if (rc) { (void)hipStreamSynchronize(s); return rc; }              // `tabs` and the caller's `tw` are read by copies that may still be in flight
    D2G_HIP(ctx, hipGetLastError());
    D2G_HIP(ctx, hipMemcpyAsync(sig_out, d_h, ng * m * 8, hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return D2G_OK;
}

void d2g_warm_k3_lists() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k3_bmh_sets_kernel));
}
