// cmp_dense.cpp -- the dense outputs of `dashing2 cmp` / `sketch --cmpout`: condensed triangle, square matrix, panel.  Mirrors
//   cmp_core (densify)       src/cmp_core.cpp:686-718,746-751
//   emit_rectangular         src/emitrect.cpp:108-403
// on one GPU or, rows dealt round-robin, on several (D2G_DEVICES).  Four jobs -- registers on one GPU, on several, exact sets, edit
// distances -- each: set-up, the two callbacks it hands to the one row-batch loop (row_batches.h), a report.
#include "cli_common.h"
#include "fmtfloat.h"
#include "row_batches.h"
#include <deque>

namespace d2h {

namespace {

// ------------------------------------------------------------------------------------ emit
struct Emitter {
    const Options &o;
    const Result &res;
    std::FILE *fp = nullptr;
    bool own = false;
    // Binary matrices leave through ONE buffered stream.  Measured and dropped: (round 3) a shared mapping of the output filled by
    // all threads -- copy 0.74 -> 0.57 s for config 4's 5 GB, but unmapping the dirty pages cost another 0.51 s on the box's overlay
    // file system; (round 4) the batch cut into 4 MiB pieces that 8 threads pwrite() at their offsets -- no gain at all (config 3:
    // 22 ms either way, config 4: 0.50 s either way, ~10 GB/s): buffered writes to one file serialise on its inode lock.
    Emitter(const Options &oo, const Result &r) : o(oo), res(r) {
        const std::string outp = (o.cmpout.empty() || o.cmpout.front() == '-') ? "/dev/stdout" : o.cmpout;   // emitrect.cpp:114-115
        if (outp == "/dev/stdout") fp = stdout;
        else { fp = std::fopen(outp.c_str(), "wb"); own = true; }
        if (!fp) die("Failed to open path " + outp + " for writing");
        static std::vector<char> buf(1 << 22);
        std::setvbuf(fp, buf.data(), _IOFBF, buf.size());
    }
    ~Emitter() { if (fp) { std::fflush(fp); if (own) std::fclose(fp); } }
    void header() {                                                     // emitrect.cpp:136-151
        if (o.of != HUMAN_READABLE) return;
        const size_t ns = res.names.size();
        if (o.ok == PHYLIP) { std::fprintf(fp, "%zu\n", ns); return; }
        const char *label = o.ok == ASYMMETRIC_ALL_PAIRS ? "Asymmetric pairwise" : o.ok == PANEL ? "Panel (Query/Refernce)" : "Symmetric pairwise";
        std::fprintf(fp, "#Dashing2 %s Output\n", label);
        std::fprintf(fp, "#Dashing2Options: %s\n", o.to_string().c_str());
        // not a reference line: written only when --fmt-compat was given, so that the default output stays byte-identical to
        // emitrect.cpp:138-147 while a deliberate choice of float layout is on record in the file it shaped
        if (o.fmt_compat) std::fprintf(fp, "#Dashing2FloatText: fmt-compat=%d\n", o.fmt_compat);
        std::fputs("#Sources", fp);
        for (size_t i = 0; i < ns; ++i) { std::fputc('\t', fp); std::fwrite(res.names[i].data(), 1, res.names[i].size(), fp); }
        std::fputc('\n', fp);
    }
    // the rows of one batch; row i has sh.nvals(i) values, one row after the other in `data`
    void rows(const Batch &bt, const float *data, const CmpShape &sh) {
        const size_t r0 = bt.r0, r1 = bt.r1;
        if (o.of == MACHINE_READABLE) {                                  // emitrect.cpp:189-192
            if (std::fwrite(data, sizeof(float), bt.cnt, fp) != bt.cnt) die("Failed to write rows " + std::to_string(r0) + "-" + std::to_string(r1) + " to disk");
            return;
        }
        const size_t n = r1 - r0;
        std::vector<size_t> off(n + 1, 0);
        for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + sh.nvals(r0 + i);
        std::vector<std::string> text(n);
#ifdef _OPENMP
        #pragma omp parallel for schedule(dynamic, 8) num_threads(o.workers())
#endif
        for (size_t r = 0; r < n; ++r) {                                 // emitrect.cpp:172-187
            const size_t i = r0 + r;
            std::string &s = text[r];
            std::string fn = (res.names.size() > i && !res.names[i].empty()) ? res.names[i] : std::string("E") + std::to_string(i);
            if (fn.size() < 9) fn.append(9 - fn.size(), ' ');
            const size_t nv = off[r + 1] - off[r];
            s.reserve(fn.size() + 2 * (i + 1) + nv * 12 + 2);
            s = fn;
            if (o.ok == SYMMETRIC_ALL_PAIRS) for (size_t t = 0; t < i + 1; ++t) s += "\t-";     // print_tabs, emitrect.cpp:40-66
            char buf[FMT_MAX_FLOAT_CHARS + 1];
            const float *p = data + off[r];
            for (size_t j = 0; j < nv; ++j) {
                buf[0] = '\t';
                const size_t l = format_float(p[j], buf + 1);
                s.append(buf, l + 1);
            }
            s += '\n';
        }
        for (const auto &s : text)
            if (std::fwrite(s.data(), 1, s.size(), fp) != s.size()) die("Failed to write text rows");
    }
};

// values per row batch: a slot is one batch's staging; the slots cycle device -> host epilogue -> emitter (row_batches.h).  Small jobs
// take small slots (more batches cost little: the pair kernel is launched per row range), big jobs 64 MiB ones.
size_t cmp_slot_values(size_t total_vals) {
    size_t v = std::min<size_t>(size_t(1) << 24, std::max<size_t>(size_t(1) << 22, total_vals / 12));
    if (const char *e = std::getenv("D2G_CMP_SLOT_VALUES")) { const long long x = std::atoll(e); if (x >= 1) v = size_t(x); }   // tests: tiny slots
    return v;
}

// ------------------------------------------------------------------------------------ the job
// the shape of the dense job that an Options / Result pair asks for, and the values per row batch it runs with
struct JobShape : CmpShape {
    const size_t cap;
    JobShape(const Options &o, const Result &res)
        : CmpShape(o.ok == SYMMETRIC_ALL_PAIRS || o.ok == PHYLIP, o.ok == PANEL, res.names.size(), res.nq), cap(slot_cap(cmp_slot_values(total_vals))) {}
};
// the one loop of every dense job: the rows of a finished batch go to the emitter on the queue's thread
template <class Launch, class Finish>
RowBatchRun emit_row_batches(const JobShape &sh, Emitter &em, int W, size_t nslots, Launch launch, Finish finish) {
    return run_row_batches(sh, sh.cap, W, int(nslots), launch, finish, [&](const Batch &bt, const float *data) { em.rows(bt, data, sh); });
}

// One dense job: what is counted on the device and how a count becomes the float that is written.
//   have_lut   the value is a table of the equality count alone (a triangle then comes back from the device as floats: `fused`)
//   need_gtlt  the value needs (gt, lt) counts: a sketch size that is not a power of two, setsketch-truncated registers
//   trunc      --fastcmp: the registers were truncated to o.regbytes; trunc_b: the setsketch base (null for b-bit codes)
struct DenseJob {
    const Options &o;
    const JobShape sh;
    const size_t S;
    const double *cards;
    const bool have_lut, need_gtlt, trunc, multiset;
    const std::vector<float> &lut;
    const long double *trunc_b;
    DenseJob(const Options &oo, const Result &res, bool lutv, bool gtlt, bool tr, bool ms, const std::vector<float> &l, const long double *tb)
        : o(oo), sh(oo, res), S(oo.sketchsize), cards(res.cardinalities.data()), have_lut(lutv), need_gtlt(gtlt), trunc(tr), multiset(ms), lut(l), trunc_b(tb) {}
    bool fused() const { return have_lut && sh.symmetric; }
};
// where one GPU computes its batches: the operand, the table, the counts of the batch in flight
struct DenseDevice {
    d2g_ctx *ctx; const d2g_cmp_set *set;
    DevBuf dlut, da, db;                                                // db: the lt counts of a (gt, lt) job
    DenseDevice(const DenseJob &j, d2g_ctx *c, const d2g_cmp_set *s)
        : ctx(c), set(s), dlut(c, (j.S + 1) * sizeof(float)), da(c, j.sh.cap * 4), db(c, j.need_gtlt ? j.sh.cap * 4 : 0) {
        if (j.have_lut) check(ctx, d2g_memcpy_h2d(ctx, dlut.p, j.lut.data(), (j.S + 1) * sizeof(float), nullptr), "h2d lut");
    }
};
// One slot's staging: what comes back from the device (`raw`: counts, intersection sizes, distances; `raw2`: the lt counts of a
// (gt, lt) job) and the floats made of it.  Plain memory: nothing to page-lock, nothing for a helper thread to do
struct HostSlot {
    HostBuf out, raw, raw2;
    HostSlot(size_t out_bytes, size_t raw_bytes, size_t raw2_bytes) : out(out_bytes), raw(raw_bytes), raw2(raw2_bytes) {}
};
struct HostSlots : std::deque<HostSlot> {                               // the 2 W + 1 slots of a job on W lanes
    HostSlots(int W, size_t out_bytes, size_t raw_bytes, size_t raw2_bytes = 0) { for (int i = 0; i < 2 * W + 1; ++i) emplace_back(out_bytes, raw_bytes, raw2_bytes); }
    HostSlots(int W, const DenseJob &j) : HostSlots(W, j.sh.cap * 4, j.fused() ? 0 : j.sh.cap * 4, j.need_gtlt ? j.sh.cap * 4 : 0) {}
};

// counts of a rectangular batch -> floats (emitrect.cpp:211-268 call compare(i, j) per cell: cmp_core.cpp:458-517)
void rect_epilogue(const DenseJob &j, const Batch &bt, const uint32_t *ca, const uint32_t *cb, float *out) {
    const Options &o = j.o;
    const CmpShape &sh = j.sh;
    const size_t S = j.S;
#ifdef _OPENMP
    #pragma omp parallel for schedule(dynamic, 4) num_threads(o.workers())
#endif
    for (size_t i = bt.r0; i < bt.r1; ++i)
        for (size_t c = sh.c0; c < sh.c1; ++c) {
            const size_t p = (i - bt.r0) * sh.ncol + (c - sh.c0);
            out[p] = j.have_lut ? j.lut[ca[p]]
                   : j.multiset ? d2g_epilogue_neq(ca[p], S, j.cards[i], j.cards[c], o.measure, o.k)
                   : j.need_gtlt ? d2g_epilogue_gtlt(ca[p], cb[p], S, j.cards[i], j.cards[c], o.measure, o.k)
                                 : d2g_epilogue_gtlt(S - ca[p], 0, S, j.cards[i], j.cards[c], o.measure, o.k);
        }
}

// starts the pair kernel of one batch on a device (asynchronous): triangle rows emitrect.cpp:290-323, rectangle rows :211-268
void launch_batch(const DenseJob &j, DenseDevice &d, const Batch &bt) {
    uint32_t *a = (uint32_t *)d.da.p, *b = (uint32_t *)d.db.p;
    if (j.sh.symmetric) {
        if (j.have_lut) check(d.ctx, d2g_cmp_lut_ut_dev(d.ctx, d.set, bt.r0, bt.r1, (const float *)d.dlut.p, (float *)d.da.p, nullptr), "d2g_cmp_lut_ut_dev");
        else if (j.need_gtlt) check(d.ctx, d2g_cmp_gtlt_ut_dev(d.ctx, d.set, bt.r0, bt.r1, a, b, nullptr), "d2g_cmp_gtlt_ut_dev");
        else check(d.ctx, d2g_cmp_eqcount_ut_dev(d.ctx, d.set, bt.r0, bt.r1, a, nullptr), "d2g_cmp_eqcount_ut_dev");
    } else {
        if (j.need_gtlt) check(d.ctx, d2g_cmp_gtlt_rect_dev(d.ctx, d.set, bt.r0, bt.r1, j.sh.c0, j.sh.c1, a, b, nullptr), "d2g_cmp_gtlt_rect_dev");
        else check(d.ctx, d2g_cmp_eqcount_rect_dev(d.ctx, d.set, bt.r0, bt.r1, j.sh.c0, j.sh.c1, a, nullptr), "d2g_cmp_eqcount_rect_dev");
    }
}

// copies the batch back into a host slot and finishes it there (x87 epilogue on the host: cmp_core.cpp:458-517; truncated
// registers: 406-448) -> the floats of its rows
const float *finish_batch(const DenseJob &j, DenseDevice &d, const Batch &bt, HostSlot &sl) {
    const Options &o = j.o;
    const CmpShape &sh = j.sh;
    const size_t ns = sh.ns, S = j.S;
    float *out = sl.out.as<float>();
    uint32_t *ca = sl.raw.as<uint32_t>(), *cb = j.need_gtlt ? sl.raw2.as<uint32_t>() : nullptr;
    if (bt.cnt && j.fused()) check(d.ctx, d2g_memcpy_d2h(d.ctx, out, d.da.p, bt.cnt * 4, nullptr), "d2h");
    else if (bt.cnt) {
        if (cb) check(d.ctx, d2g_memcpy_d2h(d.ctx, cb, d.db.p, bt.cnt * 4, nullptr), "d2h");
        check(d.ctx, d2g_memcpy_d2h(d.ctx, ca, d.da.p, bt.cnt * 4, nullptr), "d2h");
        const int nt = int(o.workers());
        if (sh.symmetric && j.trunc) check(d.ctx, d2g_epilogue_trunc_ut(ca, cb, j.cards, ns, S, bt.r0, bt.r1, o.measure, o.k, o.regbytes, j.trunc_b, nt, out), "d2g_epilogue_trunc_ut");
        else if (sh.symmetric) check(d.ctx, d2g_epilogue_ut(ca, cb, j.cards, ns, S, bt.r0, bt.r1, o.measure, o.k, j.multiset, nt, out), "d2g_epilogue_ut");
        else if (j.trunc) check(d.ctx, d2g_epilogue_trunc_rect(ca, cb, j.cards, ns, S, bt.r0, bt.r1, sh.c0, sh.c1, o.measure, o.k, o.regbytes, j.trunc_b, nt, out), "d2g_epilogue_trunc_rect");
        else rect_epilogue(j, bt, ca, cb, out);
    }
    return out;
}

// ------------------------------------------------------------------------------------ --gpu-stats
// a long double as a JSON number with every digit (the setsketch parameters a and b)
std::string ldstr(long double v) { char b[64]; std::snprintf(b, sizeof b, "%.21Lg", v); return b; }

// what the sparse-tile path did on the last upper-triangle launch of the set (include/d2g.h: d2g_cmp_set_sparse_info)
std::string sparse_json(d2g_ctx *ctx, const d2g_cmp_set *set) {
    uint32_t i4[4] = {0, 0, 0, 0};
    if (d2g_cmp_set_sparse_info(ctx, set, nullptr, i4) != D2G_OK) return "null";
    return Json::object().boolean("sorted_operand", i4[0]).integer("tiles_listed_last_launch", i4[1]).boolean("dense_decided_by_prepare", i4[2] & 1)
        .boolean("dense_kernel_ran", i4[2] & 2).boolean("tiles_and_pair_list", i4[2] & 4).boolean("callers_order_kept", i4[2] & 8).integer("pairs_listed", i4[3]).text();
}
std::string planes_json(d2g_ctx *ctx, const d2g_cmp_set *set) {
    unsigned md = 0; int nb = 0; float mean = 0;
    if (d2g_cmp_set_planes(ctx, set, nullptr, &md, &nb, &mean) != D2G_OK) return "null";
    return Json::object().integer("max", nb).num("mean", mean).integer("max_shared_values_per_column_plus1", md).text();
}
Json k2_device_json(int dev, d2g_ctx *ctx) {
    Json e = device_json(dev);
    e.raw("k2", kernel_json(ctx, "k2")).raw("k2prep", kernel_json(ctx, "k2prep"));
    return e;
}

// ------------------------------------------------------------------------------------ several GPUs
// A dense comparison job over several GPUs from ONE process (the reference's seam is the single call
// emit_rectangular(opts, result), src/cmp_core.cpp:746-751).  Every GPU gets a contiguous block of rows of the signature matrix; one
// exchange (d2g_allpairs_prepare_all: all-to-all of column slices, sharded prepare, all-gather of the bit planes over RCCL/xGMI)
// leaves the whole bit-sliced operand on every GPU; row batches -- of the condensed triangle (emitrect.cpp:290-323), of the square
// matrix (--square, :249-268) or of the reference x query panel (-Q, :211-247) -- are then dealt to the GPUs round-robin, computed
// concurrently, and emitted in row order through the slot queue: byte-identical to the single-GPU output.
// Returns false (nothing emitted yet) when the sharded bit-sliced prepare overflowed its rank table on some rank -- an adversarial /
// extremely skewed register column at N > 21 845: the caller then takes the single-GPU path, whose AUTO algorithm falls back to the
// direct kernel.
struct MultiGpu {
    const int W;
    std::vector<d2g_ctx *> ctxs;
    std::vector<d2g_comm *> comms;
    std::vector<d2g_allpairs *> engs;
    explicit MultiGpu(const std::vector<int> &devs) : W(int(devs.size())), ctxs(W, nullptr), comms(W, nullptr), engs(W, nullptr) {
        for (int r = 0; r < W; ++r) {
            const int rc = d2g_ctx_create(devs[r], &ctxs[r]);
            if (rc != D2G_OK) die(std::string("D2G_DEVICES: d2g_ctx_create(") + std::to_string(devs[r]) + "): " + d2g_strerror(rc));
            if (g_stats.on) (void)d2g_set_timing(ctxs[r], TIME_ALL);
        }
        check(ctxs[0], d2g_comm_create_all(ctxs.data(), W, comms.data()), "d2g_comm_create_all");
    }
    // uploads every rank's block of rows and runs the exchange; false: the prepare overflowed on some rank
    bool prepare(const uint64_t *bits, size_t ns, size_t S) {
        std::vector<const uint64_t *> rows(W, nullptr);
        std::vector<void *> rowbuf(W, nullptr);
        for (int r = 0; r < W; ++r) {
            check(ctxs[r], d2g_allpairs_create(ctxs[r], comms[r], ns, S, &engs[r]), "d2g_allpairs_create");
            size_t lo = 0, hi = 0;
            d2g_allpairs_rows_held(engs[r], &lo, &hi);
            check(ctxs[r], d2g_malloc(ctxs[r], std::max<size_t>((hi - lo) * S, 1) * 8, &rowbuf[r]), "d2g_malloc");
            if (hi > lo) check(ctxs[r], d2g_memcpy_h2d(ctxs[r], rowbuf[r], bits + lo * S, (hi - lo) * S * 8, nullptr), "h2d rows");
            rows[r] = static_cast<const uint64_t *>(rowbuf[r]);
        }
        check(ctxs[0], d2g_allpairs_prepare_all(engs.data(), W, rows.data(), nullptr), "d2g_allpairs_prepare_all");
        bool overflow = false;
        for (int r = 0; r < W; ++r) {
            const int st = d2g_allpairs_status(engs[r], nullptr);      // every rank sees every rank's status word
            if (st == D2G_ERR_INTERNAL) overflow = true;
            else check(ctxs[r], st, "d2g_allpairs_status");
            check(ctxs[r], d2g_free(ctxs[r], rowbuf[r]), "d2g_free");
        }
        return !overflow;
    }
    const char *transport() const { return d2g_comm_is_rccl(comms[0]) ? "RCCL" : "loopback"; }
    ~MultiGpu() { for (int r = 0; r < W; ++r) { d2g_allpairs_destroy(engs[r]); d2g_comm_destroy(comms[r]); d2g_ctx_destroy(ctxs[r]); } }
};

bool cmp_core_multi(const DenseJob &job, Result &res, const std::vector<int> &devs) {
    const Options &o = job.o;
    const JobShape &sh = job.sh;
    const size_t ns = sh.ns, S = job.S;
    const double t0 = now();
    MultiGpu mg(devs);
    const int W = mg.W;
    if (!mg.prepare(reinterpret_cast<const uint64_t *>(res.sigs()), ns, S)) {
        std::fprintf(stderr, "[d2g] multi-GPU bit-sliced prepare overflowed on a skewed register column: falling back to one GPU\n");
        return false;
    }
    const double t_prep = now() - t0;
    Emitter em(o, res);
    em.header();
    std::deque<DenseDevice> dd;
    for (int r = 0; r < W; ++r) dd.emplace_back(job, mg.ctxs[r], d2g_allpairs_operand(mg.engs[r]));
    HostSlots slots(W, job);
    const RowBatchRun run = emit_row_batches(sh, em, W, slots.size(),
                                             [&](int r, const Batch &bt) { launch_batch(job, dd[r], bt); },
                                             [&](int r, const Batch &bt, int si) { return finish_batch(job, dd[r], bt, slots[si]); });
    if (o.verbosity) std::fprintf(stderr, "[d2g] cmp on %d GPUs (%s): %zu sketches x S=%zu: upload+exchange+prepare %.3fs, %zu batches %.3fs wall (device+D2H+epilogue %.3fs busy, emit %.3fs busy, overlapped)\n",
                                  W, mg.transport(), ns, S, t_prep, run.nbatches, run.t_wall, run.t_dev_busy, run.t_emit_busy);
    if (g_stats.on) {
        Json dj = Json::array();
        for (int r = 0; r < W; ++r) dj.push(k2_device_json(devs[r], mg.ctxs[r]));
        g_stats.nest("cmp", Json::object().integer("sketches", ns).integer("sketchsize", S).integer("values", sh.total_vals).str("shape", sh.name()).str("algo", "bitslice")
                     .str("transport", mg.transport()).integer("exchange_chunks", d2g_allpairs_chunks(mg.engs[0])).raw("bit_planes", planes_json(mg.ctxs[0], d2g_allpairs_operand(mg.engs[0])))
                     .num("algorithmic_bytes", 8.0 * double(S) * double(ns) + 4.0 * double(sh.total_vals)).integer("batches", run.nbatches).integer("slot_values", sh.cap).nest("devices", dj)
                     .nest("wall_s", Json::object().num("upload_exchange_prepare", t_prep).num("batches", run.t_wall).num("device_d2h_epilogue_busy", run.t_dev_busy).num("emit_busy", run.t_emit_busy)));
    }
    return true;
}

// ------------------------------------------------------------------------------------ one GPU
// `codes`: the truncated registers of a --fastcmp job (consumed), else empty
void cmp_core_single(const DenseJob &job, Result &res, d2g_ctx *ctx, std::vector<uint8_t> &codes, const long double *trunc_ab, double t_densify) {
    const Options &o = job.o;
    const JobShape &sh = job.sh;
    const size_t ns = sh.ns, S = job.S;
    d2g_cmp_set *set = nullptr;
    const double t0 = now();
    HostSlots slots(1, job);
    Emitter em(o, res);
    em.header();
    if (job.trunc) check(ctx, d2g_cmp_set_create_codes(ctx, codes.data(), ns, S, o.regbytes, &set), "d2g_cmp_set_create_codes");
    else check(ctx, d2g_cmp_set_create(ctx, reinterpret_cast<const uint64_t *>(res.sigs()), ns, S, job.need_gtlt ? int(D2G_CMP_DIRECT) : int(D2G_CMP_AUTO), &set), "d2g_cmp_set_create");
    std::vector<uint8_t>().swap(codes);
    const double t_set = now();
    DenseDevice dev(job, ctx, set);
    const double t_bufs = now();
    if (o.verbosity) std::fprintf(stderr, "[d2g] cmp set-up: host slots + header + operand upload + prepare %.3fs, device buffers %.3fs (slots of %zu values)\n",
                                  t_set - t0, t_bufs - t_set, sh.cap);
    const RowBatchRun run = emit_row_batches(sh, em, 1, slots.size(),
                                             [&](int, const Batch &bt) { launch_batch(job, dev, bt); },
                                             [&](int, const Batch &bt, int si) { return finish_batch(job, dev, bt, slots[si]); });
    if (o.verbosity) std::fprintf(stderr, "[d2g] cmp: %zu sketches x S=%zu: upload+prepare+buffers %.3fs, %zu batches %.3fs wall (device+D2H+epilogue %.3fs busy, emit %.3fs busy, "
                                          "overlapped) (algo %s)\n", ns, S, t_bufs - t0, run.nbatches, run.t_wall, run.t_dev_busy, run.t_emit_busy,
                                  d2g_cmp_set_algo(set) == D2G_CMP_BITSLICE ? "bitslice" : d2g_cmp_set_algo(set) == D2G_CMP_PLANES ? "planes" : "direct");
    if (g_stats.on) {
        const bool bs = d2g_cmp_set_algo(set) == D2G_CMP_BITSLICE, ab = job.trunc && job.need_gtlt;
        Json dj = Json::array();
        g_stats.nest("cmp", Json::object().integer("sketches", ns).integer("sketchsize", S).integer("values", sh.total_vals).str("shape", sh.name())
                     .str("algo", bs ? "bitslice" : job.trunc ? "planes" : "direct").integer("regbytes", o.regbytes)
                     .raw("truncation", !job.trunc ? "null" : ab ? "\"setsketch\"" : "\"bbit\"").raw("a", ab ? ldstr(trunc_ab[0]) : "null").raw("b", ab ? ldstr(trunc_ab[1]) : "null")
                     .raw("bit_planes", bs ? planes_json(ctx, set) : "null").raw("sparse_tiles", bs ? sparse_json(ctx, set) : "null")
                     .num("algorithmic_bytes", double(o.regbytes) * double(S) * double(ns) + 4.0 * double(sh.total_vals)).integer("batches", run.nbatches).integer("slot_values", sh.cap)
                     .nest("devices", dj.push(k2_device_json(o.device, ctx)))
                     .nest("wall_s", Json::object().num("densify_scan", t_densify).num("slots_header_upload_prepare", t_set - t0).num("batches", run.t_wall)
                           .num("device_d2h_epilogue_busy", run.t_dev_busy).num("emit_busy", run.t_emit_busy)));
    }
    if (g_release_at_exit) d2g_cmp_set_destroy(set);
}

}  // namespace

// the D2G_* switches the context resolved when it was created (include/d2g.h: d2g_ctx_tuning)
std::string context_switches_json(d2g_ctx *ctx) {
    const int n = d2g_ctx_tuning(ctx, nullptr, 0);
    if (n < 0) return "null";
    std::string buf((size_t)n + 1, '\0');
    d2g_ctx_tuning(ctx, &buf[0], buf.size());
    buf.resize((size_t)n);
    return buf;
}

// --set / --countdict: the same dense outputs from EXACT intersections.  Replaces the exact branch of compare() (cmp_core.cpp:518-575:
// per pair, both files opened and merged with one fread per element) -- the sets go to the device once (d2g_kset), row batches of
// u64 intersection sizes come back (d2g_kset_isz_*_dev), d2g_epilogue_exact_* turns them into the measure in double, as CORRECT_RES does.
void cmp_core_exact(const Options &o, Result &res, d2g_ctx *ctx, const ExactSets &es) {
    const JobShape sh(o, res);
    const size_t ns = sh.ns;
    const double t0 = now();
    std::vector<uint64_t> off(ns + 1, 0);
    for (size_t i = 0; i < ns; ++i) off[i + 1] = off[i] + es.keys[i].size();
    std::vector<uint64_t> keys(std::max<uint64_t>(off[ns], 1));
    std::vector<uint32_t> counts(es.weighted ? std::max<uint64_t>(off[ns], 1) : 0);
    for (size_t i = 0; i < ns; ++i) {
        std::copy(es.keys[i].begin(), es.keys[i].end(), keys.begin() + off[i]);
        if (es.weighted) std::copy(es.counts[i].begin(), es.counts[i].end(), counts.begin() + off[i]);
    }
    d2g_kset *ks = nullptr;
    check(ctx, d2g_kset_create(ctx, keys.data(), es.weighted ? counts.data() : nullptr, off.data(), ns, &ks), "d2g_kset_create");
    std::vector<uint64_t>().swap(keys); std::vector<uint32_t>().swap(counts);
    const double t_set = now();
    Emitter em(o, res);
    em.header();
    DevBuf d(ctx, sh.cap * 8);
    HostSlots slots(1, sh.cap * 4, sh.cap * 8);
    const int nt = int(o.workers());
    const RowBatchRun run = emit_row_batches(sh, em, 1, slots.size(),
        [&](int, const Batch &bt) {
            if (sh.symmetric) check(ctx, d2g_kset_isz_ut_dev(ctx, ks, bt.r0, bt.r1, (uint64_t *)d.p, nullptr), "d2g_kset_isz_ut_dev");
            else check(ctx, d2g_kset_isz_rect_dev(ctx, ks, bt.r0, bt.r1, sh.c0, sh.c1, (uint64_t *)d.p, nullptr), "d2g_kset_isz_rect_dev");
        },
        [&](int, const Batch &bt, int si) -> const float * {
            uint64_t *isz = slots[si].raw.as<uint64_t>();
            float *out = slots[si].out.as<float>();
            if (!bt.cnt) return out;
            check(ctx, d2g_memcpy_d2h(ctx, isz, d.p, bt.cnt * 8, nullptr), "d2h");
            if (sh.symmetric) check(ctx, d2g_epilogue_exact_ut(isz, res.cardinalities.data(), ns, bt.r0, bt.r1, o.measure, o.k, nt, out), "d2g_epilogue_exact_ut");
            else check(ctx, d2g_epilogue_exact_rect(isz, res.cardinalities.data(), ns, bt.r0, bt.r1, sh.c0, sh.c1, o.measure, o.k, nt, out), "d2g_epilogue_exact_rect");
            return out;
        });
    if (o.verbosity) std::fprintf(stderr, "[d2g] exact cmp: %zu sets, %llu keys (%zu bytes resident, 2^%d slices): upload + slice table %.3fs, %zu batches %.3fs\n", ns,
                                  (unsigned long long)off[ns], d2g_kset_device_bytes(ks), d2g_kset_slice_bits(ks), t_set - t0, run.nbatches, now() - t_set);
    if (g_stats.on) {
        Json dj = Json::array();
        Json e = device_json(o.device);
        e.raw("kset", kernel_json(ctx, "kset")).raw("ksetprep", kernel_json(ctx, "ksetprep"));
        g_stats.nest("cmp", Json::object().integer("sets", ns).integer("keys", off[ns]).integer("values", sh.total_vals).str("shape", sh.name())
                     .str("algo", es.weighted ? "exact count dictionaries" : "exact k-mer sets").integer("resident_bytes", d2g_kset_device_bytes(ks))
                     .integer("slice_bits", d2g_kset_slice_bits(ks)).integer("batches", run.nbatches).integer("slot_values", sh.cap).nest("devices", dj.push(e))
                     .nest("wall_s", Json::object().num("upload_slice_table", t_set - t0).num("batches", now() - t_set)));
    }
    if (g_release_at_exit) d2g_kset_destroy(ks);
}

// --edit-distance --compute-edit-distance: the same dense outputs from exact edit distances.  Replaces one edlibAlign per pair
// (cmp_core.cpp:331-347,450-457): the records go to the device once (d2g_seqset), row batches of u32 distances come back
// (d2g_edit_*_dev) and become the float32 the writers take -- exactly: a distance is at most 65 535 < 2^24.  --square takes the rect form,
// as the reference's asymmetric route calls compare(i, j) for every cell: the diagonal comes out of the kernel as 0 and no batch has
// to wait for rows of the triangle that lie in another one.
void cmp_core_edit(const Options &o, Result &res, d2g_ctx *ctx, const d2g_seqrecs *sr, double t_read) {
    const JobShape sh(o, res);
    const size_t ns = sh.ns;
    const uint64_t *off = d2g_seqrecs_off(sr);
    const double t0 = now();
    d2g_seqset *ss = nullptr;
    check(ctx, d2g_seqset_create(ctx, d2g_seqrecs_bytes(sr), off, ns, off[ns], &ss), "d2g_seqset_create");
    const double t_set = now();
    Emitter em(o, res);
    em.header();
    DevBuf d(ctx, sh.cap * 4);
    HostSlots slots(1, sh.cap * 4, sh.cap * 4);
    long double cells = 0;
    std::vector<uint64_t> suffix(ns + 1, 0);                        // symbols of records [i, ns)
    for (size_t i = ns; i-- > 0;) suffix[i] = suffix[i + 1] + (off[i + 1] - off[i]);
    const RowBatchRun run = emit_row_batches(sh, em, 1, slots.size(),
        [&](int, const Batch &bt) {
            if (sh.symmetric) check(ctx, d2g_edit_ut_dev(ctx, ss, bt.r0, bt.r1, (uint32_t *)d.p, nullptr), "d2g_edit_ut_dev");
            else check(ctx, d2g_edit_rect_dev(ctx, ss, bt.r0, bt.r1, sh.c0, sh.c1, (uint32_t *)d.p, nullptr), "d2g_edit_rect_dev");
        },
        [&](int, const Batch &bt, int si) -> const float * {
            uint32_t *dist = slots[si].raw.as<uint32_t>();
            float *out = slots[si].out.as<float>();
            if (bt.cnt) check(ctx, d2g_memcpy_d2h(ctx, dist, d.p, bt.cnt * 4, nullptr), "d2h");
            for (size_t e = 0; e < bt.cnt; ++e) out[e] = float(dist[e]);
            for (size_t i = bt.r0; i < bt.r1; ++i) cells += (long double)(off[i + 1] - off[i]) * (long double)(sh.symmetric ? suffix[i + 1] : suffix[sh.c0] - suffix[sh.c1]);
            return out;
        });
    if (o.verbosity) std::fprintf(stderr, "[d2g] edit distances: %zu records, %llu symbols over %d letters (%zu bytes resident): read %.3fs, upload + recoding %.3fs, %zu batches %.3fs\n",
                                  ns, (unsigned long long)off[ns], d2g_seqset_alphabet_size(ss), d2g_seqset_device_bytes(ss), t_read, t_set - t0, run.nbatches, now() - t_set);
    if (g_stats.on) {
        Json dj = Json::array();
        Json e = device_json(o.device);
        e.raw("edit", kernel_json(ctx, "edit")).raw("editprep", kernel_json(ctx, "editprep"));
        g_stats.nest("cmp", Json::object().integer("values", sh.total_vals).str("shape", sh.name()).str("algo", "exact edit distances (bit-parallel, K2h)")
                     .nest("edit", Json::object().integer("records", ns).integer("symbols", off[ns]).integer("alphabet", d2g_seqset_alphabet_size(ss))
                           .integer("cells", (unsigned long long)cells).integer("batches", run.nbatches).integer("resident_bytes", d2g_seqset_device_bytes(ss)))
                     .integer("slot_values", sh.cap).nest("devices", dj.push(e))
                     .nest("wall_s", Json::object().num("read", t_read).num("upload_recode", t_set - t0).num("batches", now() - t_set)));
    }
    if (g_release_at_exit) d2g_seqset_destroy(ss);
}

void cmp_core(const Options &o, Result &res, d2g_ctx *ctx) {      // src/cmp_core.cpp:615-751
    const size_t ns = res.names.size(), S = o.sketchsize;
    if (res.nsigs() != ns * S) die("Empty signatures; trying to compare but don't have any");
    const bool multiset = o.sspace != SPACE_SET;
    double t_densify = 0;
    if (o.kmer_result == ONE_PERM) {                                // cmp_core.cpp:686-718
        size_t nfilled = 0;
        const double td = now();
        check(ctx, d2g_densify(res.sigs(), ns, S, &nfilled, int(o.workers())), "d2g_densify");
        t_densify = now() - td;
        if (o.verbosity) std::fprintf(stderr, "[d2g] densify scan %.3fs\n", t_densify);
        if (o.verbosity && nfilled) std::fprintf(stderr, "Densified a total of %zu/%zu entries\n", nfilled, S * ns);
    }
    std::vector<float> lut(S + 1);
    // --fastcmp <4|2|1>: make_compressed (cmp_core.cpp:741) truncates the registers and compare() takes its compressed branch
    // (:362-449), whatever the sketch space: (gt, lt) of setsketch codes, equal b-bit codes
    const bool trunc = o.regbytes < 8, trunc_gtlt = trunc && !o.bbit_sigs;
    std::vector<uint8_t> codes;
    long double trunc_ab[2] = {0.L, 0.L};
    if (trunc) {
        if (!ns) die("Empty signatures; trying to compress registers but don't have any");
        codes.resize(ns * S * size_t(o.regbytes));
        double mm[2] = {0, 0};
        char err[200];
        if (d2g_regs_truncate(res.sigs(), ns, S, o.regbytes, o.bbit_sigs, codes.data(), trunc_ab, mm, int(o.workers()), err, sizeof err) != D2G_OK)
            die(std::string("dashing2 (MI355X): ") + err);
        if (trunc_gtlt)                                             // cmp_core.cpp:262
            std::fprintf(stderr, "Truncated via setsketch, a = %0.20Lg and b = %0.24Lg from min, max regs %Lg, %Lg\n", trunc_ab[0], trunc_ab[1],
                         static_cast<long double>(mm[0]), static_cast<long double>(mm[1]));
    }
    const bool have_lut = !trunc && d2g_epilogue_lut(S, o.measure, o.k, multiset, lut.data()) == D2G_OK;
    const bool need_gtlt = trunc ? trunc_gtlt : (!multiset && (S & (S - 1)) != 0);
    if (const char *sparse = sparse_job_name(o)) {                  // cmp_core.cpp:776-805
        refuse_sparse_job_out_of_scope(sparse, o, S);
        if (!have_lut) refuse_out_of_scope(std::string(sparse) + " of values that are not a function of the equality count");
        if (o.ok == DEDUP) { note_devices_ignored(o, "the greedy clustering runs on one GPU"); cmp_core_dedup(o, res, ctx, lut, t_densify); }
        else { note_devices_ignored(o, "the nearest-neighbour selection runs on one GPU"); cmp_core_knn(o, res, ctx, lut, t_densify); }
        return;
    }
    const DenseJob job(o, res, have_lut, need_gtlt, trunc, multiset, lut, trunc_gtlt ? &trunc_ab[1] : nullptr);
    const std::vector<int> devs = job_devices(o);
    if (devs.size() > 1 && !need_gtlt && !trunc && ns >= 2) {
        if (cmp_core_multi(job, res, devs)) return;
    } else note_devices_ignored(o, trunc ? "truncated registers (--fastcmp) are compared on one GPU"
                                   : need_gtlt ? "a sketch size that is not a power of two needs (gt, lt) counts from the raw registers, which the gathered bit-plane operand does not hold"
                                               : "fewer than two sketches");
    cmp_core_single(job, res, ctx, codes, trunc_ab, t_densify);
}

}  // namespace d2h
