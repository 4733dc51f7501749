// cli_common.h -- what the jobs of the `dashing2` CLI share: the sketching result, error exits, --gpu-stats, the device list,
// the lazily created GPU context, owned device / host buffers, and the entry points of the jobs themselves
// (sketch_cmd.cpp, cmp_dense.cpp, cmp_sparse.cpp; dispatched from dashing2_main.cpp).
#pragma once
#include "../../include/d2g.h"
#include "d2_options.h"
#include "fileutil.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#ifndef DASHING2_VERSION
#define DASHING2_VERSION "v2.1.20-mi355x"
#endif

namespace d2h {

struct Result {                              // SketchingResult, src/fastxsketch.h:23-58 (in-scope fields)
    std::vector<std::string> names, destination_files;
    std::vector<double> cardinalities;
    std::vector<double> signatures;          // [N][S] row-major
    double *sigs() { return signatures.data(); }
    const double *sigs() const { return signatures.data(); }
    size_t nsigs() const { return signatures.size(); }
    std::vector<uint64_t> kmers;             // kmers_ [N][S]: the masked k-mer behind every register (-s / -N with -o)
    std::vector<float> kmercounts;           // kmercounts_ [N][S] (-N with -o): floats, src/fastxsketch.h:45
    std::vector<std::string> kmercountfiles; // kmercountfiles_ [N] (-N): named in <out>.names.txt, never written for OPH
    size_t nq = 0;
};

// the exact k-mer sets of an --set / --countdict job, input by input (keys ascending); Result carries their names and cardinalities
struct ExactSets {
    bool weighted = false;                   // --countdict: counts[i] runs beside keys[i]
    std::vector<std::vector<uint64_t>> keys;
    std::vector<std::vector<uint32_t>> counts;
};

// The process leaves through _exit once its outputs are closed (main): releasing device memory and unpinning hundreds of MB
// one buffer at a time just before that costs tens of milliseconds and buys nothing.  D2G_FULL_TEARDOWN=1 releases everything.
inline const bool g_release_at_exit = std::getenv("D2G_FULL_TEARDOWN") != nullptr;

[[noreturn]] inline void die(const std::string &msg) {          // THROW_EXCEPTION: src/enums.h:59-63
    std::fprintf(stderr, "Exception %s\n", msg.c_str());
    std::exit(1);
}
inline void check(d2g_ctx *ctx, int rc, const char *what) {
    if (rc == D2G_OK) return;
    die(std::string(what) + ": " + d2g_strerror(rc) + (ctx ? std::string(" (") + d2g_last_error(ctx) + ")" : std::string()));
}
// a job (or a part of one) that this build does not do
[[noreturn]] inline void refuse_out_of_scope(const std::string &what) {
    std::fprintf(stderr, "dashing2 (MI355X): %s is outside the hot-path scope of this build.\n", what.c_str());
    std::exit(1);
}

// A JSON object or array, rendered as it is built: {"k": v, "k2": v2} / [v, v2].  Numbers are "%.9g" (null when not finite).
class Json {
    std::string s_;
    char close_;
    explicit Json(char open) : s_(1, open), close_(open == '{' ? '}' : ']') {}
    std::string &slot(const char *key) {                       // key == nullptr: the next element of an array
        if (s_.size() > 1) s_ += ", ";
        if (key) { s_ += esc(key); s_ += ": "; }
        return s_;
    }
public:
    static Json object() { return Json('{'); }
    static Json array() { return Json('['); }
    static std::string esc(const std::string &x) {
        std::string r = "\"";
        for (unsigned char c : x) {
            if (c == '"' || c == '\\') { r += '\\'; r += char(c); }
            else if (c < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", c); r += b; }
            else r += char(c);
        }
        return r + "\"";
    }
    static std::string numstr(double v) { char b[40]; if (!std::isfinite(v)) return "null"; std::snprintf(b, sizeof b, "%.9g", v); return b; }
    Json &raw(const char *k, const std::string &json) { slot(k) += json; return *this; }        // a value already rendered
    Json &num(const char *k, double v) { return raw(k, numstr(v)); }
    template <class I> Json &integer(const char *k, I v) { return raw(k, std::to_string(v)); }
    Json &str(const char *k, const std::string &v) { return raw(k, esc(v)); }
    Json &boolean(const char *k, bool v) { return raw(k, v ? "true" : "false"); }
    Json &null(const char *k) { return raw(k, "null"); }
    Json &nest(const char *k, const Json &v) { return raw(k, v.text()); }                       // nested object / array
    Json &push(const Json &v) { return raw(nullptr, v.text()); }                                // array element
    std::string text() const { return s_ + close_; }
};

// --gpu-stats FILE (SURVEY 5 "Metrics / logging"; the reference only has its verbosity levels, src/enums.h:106-111, and the
// banner of src/d2.cpp:136): what -v prints, machine-readable -- ONE JSON object per run with the device(s), the HIP-event
// milliseconds of every timed kernel family (d2g_set_timing / d2g_kernel_ms), bit-plane counts, algorithmic bytes, wall phases.
struct Stats {
    bool on = false;
    std::string path;
    std::mutex mu;
    Json root = Json::object();                               // guarded by mu
    void raw(const char *k, const std::string &json) { if (!on) return; std::lock_guard<std::mutex> lk(mu); root.raw(k, json); }
    void num(const char *k, double v) { raw(k, Json::numstr(v)); }
    void str(const char *k, const std::string &v) { raw(k, Json::esc(v)); }
    void nest(const char *k, const Json &v) { raw(k, v.text()); }
    void write() {
        if (!on) return;
        std::FILE *fp = std::fopen(path.c_str(), "wb");
        if (!fp) { std::fprintf(stderr, "dashing2 (MI355X): cannot write --gpu-stats file %s\n", path.c_str()); return; }
        std::fprintf(fp, "%s\n", root.text().c_str());
        std::fclose(fp);
    }
};
inline Stats g_stats;
constexpr int TIME_ALL = D2G_TIME_EDIT | D2G_TIME_K0 | D2G_TIME_K1 | D2G_TIME_K2 | D2G_TIME_K2PREP | D2G_TIME_K3 | D2G_TIME_KNN | D2G_TIME_DEDUP | D2G_TIME_FILTER | D2G_TIME_KSET | D2G_TIME_SCREEN;

// One timed kernel family on one context: launches and HIP-event milliseconds; ok == false: the library does not know the family
struct KAcc {
    bool ok = false; int launches = 0; float avg_ms = 0, last_ms = 0; double total_ms = 0;
    KAcc &operator+=(const KAcc &k) { launches += k.launches; total_ms += k.total_ms; return *this; }
    Json json() const { return Json::object().integer("launches", launches).num("total_ms", total_ms); }   // {"launches": n, "total_ms": t}
};
// reads (and by default resets) the family's log; synchronises on its events
inline KAcc kernel_acc(d2g_ctx *ctx, const char *which, bool reset = true) {
    KAcc k;
    if (d2g_kernel_ms(ctx, which, reset, &k.launches, &k.avg_ms, &k.last_ms) != D2G_OK) return KAcc();
    k.ok = true; k.total_ms = double(k.avg_ms) * k.launches;
    return k;
}
// {"launches": n, "avg_ms": a, "total_ms": n a}; null for an unknown family
inline std::string kernel_json(d2g_ctx *ctx, const char *which, bool reset = true) {
    const KAcc k = kernel_acc(ctx, which, reset);
    return k.ok ? Json::object().integer("launches", k.launches).num("avg_ms", k.avg_ms).num("total_ms", k.total_ms).text() : "null";
}
// D2G_GROUP_BYTES: the packed bytes after which `sketch` closes a group of inputs (tests: many small groups); else the job's default
inline size_t group_bytes_limit(size_t default_bytes) {
    if (const char *e = std::getenv("D2G_GROUP_BYTES")) { const long long v = std::atoll(e); if (v >= 1) return size_t(v); }
    return default_bytes;
}

// D2G_DEVICES = "all" | "0,1,2": the GPUs a job may spread over -- `sketch` deals its input groups to them (no collectives),
// `cmp` shards the rows of the matrix (one exchange).  Default: the one device D2G_DEVICE names.  A list that repeats
// a device is allowed (cmp: loopback transport; used by the tests on one GPU).
inline std::vector<int> job_devices(const Options &o) {
    std::vector<int> d;
    const char *e = std::getenv("D2G_DEVICES");
    if (!e || !*e) return {o.device};
    if (std::strcmp(e, "all") == 0) { for (int i = 0; i < d2g_device_count(); ++i) d.push_back(i); }
    else for (const char *p = e; *p;) { char *q; const long v = std::strtol(p, &q, 10); if (q == p) break; d.push_back(int(v)); p = *q == ',' ? q + 1 : q; }
    if (d.empty()) d.push_back(o.device);
    return d;
}
// said without -v: the user asked for several GPUs and gets one
inline void note_devices_ignored(const Options &o, const char *why) {
    if (job_devices(o).size() > 1) std::fprintf(stderr, "[d2g] D2G_DEVICES ignored for this job (%s): it runs on GPU %d alone\n", why, o.device);
}
inline std::string device_label(int dev) {
    char b[256];
    return d2g_device_name(dev, b, sizeof b) == D2G_OK ? std::string(b) : std::string("?");
}
// the start of a "devices" entry of --gpu-stats; the job adds what it timed on that device
inline Json device_json(int dev) { Json j = Json::object(); j.integer("index", dev).str("name", device_label(dev)); return j; }

inline d2g_ctx *make_ctx(const Options &o) {
    d2g_ctx *ctx = nullptr;
    const int rc = d2g_ctx_create(o.device, &ctx);
    if (rc) die(std::string("dashing2 (MI355X) needs a gfx950 GPU; d2g_ctx_create: ") + d2g_strerror(rc) + " (there is no CPU fallback)");
    return ctx;
}
// The GPU context (HIP runtime start-up, 0.06-0.2 s) is created on a helper thread as soon as the options are parsed, while
// this thread stats / reads / parses the inputs; get() joins.  There is still no CPU fallback: a failure ends the process.
struct LazyCtx {
    const Options &o; std::thread th; d2g_ctx *ctx = nullptr; double t_create = 0, t_warm = 0;
    // `warm`: one-time costs the helper pays right after the context exists (D2G_WARM_*): the first host<->device copy of a process
    // costs ~30 ms whatever its size (tools/cmp_setup_time2.py), code objects ~1 ms per kernel family -- under the input reading
    LazyCtx(const Options &oo, int warm) : o(oo) {
        th = std::thread([this, warm] {
            double t = now();
            ctx = make_ctx(o);
            t_create = now() - t;
            t = now();
            if (warm) (void)d2g_warmup(ctx, warm);
            if (g_stats.on) (void)d2g_set_timing(ctx, TIME_ALL);
            t_warm = now() - t;
        });
    }
    d2g_ctx *get() { if (th.joinable()) th.join(); return ctx; }
    // the context is only torn down on request: main() leaves through _exit once every output is flushed and closed (the HIP
    // runtime's orderly shutdown costs tens of milliseconds that buy a CLI process nothing); D2G_FULL_TEARDOWN=1 keeps it
    ~LazyCtx() { get(); if (ctx && g_release_at_exit) d2g_ctx_destroy(ctx); }
};

struct DevBuf {
    d2g_ctx *ctx; void *p = nullptr;
    DevBuf(d2g_ctx *c, size_t n) : ctx(c) { check(c, d2g_malloc(c, n ? n : 4, &p), "d2g_malloc"); }
    ~DevBuf() { if (g_release_at_exit) d2g_free(ctx, p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};
// Host staging of a row batch: PLAIN page-aligned memory.  Rounds 2-3 page-locked these slots (hipHostMalloc); measured on MI355X /
// ROCm 7 (tools/cmp_setup_time2.py): a pageable D2H of 16 MiB takes 0.32 ms (1.1 ms the first time a buffer is touched) -- the
// same 50 GB/s as from page-locked memory -- while page-locking costs 0.2-0.28 ms per MiB (3 x 64 MiB = 56 ms) AND serialises
// with the operand upload inside the runtime (the upload of config 3 took 86 ms next to it instead of 30).
struct HostBuf {
    void *p = nullptr;
    explicit HostBuf(size_t n) { if (posix_memalign(&p, 4096, std::max<size_t>(n, 4096)) != 0) die("out of memory (row-batch staging)"); }
    ~HostBuf() { if (g_release_at_exit) std::free(p); }
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    template <class T> T *as() { return static_cast<T *>(p); }
};

// ------------------------------------------------------------------------------------ the jobs
// sketch_cmd.cpp
void sketch_core(Result &res, const Options &o, LazyCtx &lctx);
void sketch_core_byseq(Result &res, const Options &o, LazyCtx &lctx);
void sketch_core_bed(Result &res, const Options &o, LazyCtx &lctx);   // --bed: interval files (K1i)
int sketch_main(int argc, char **argv);
// --set / --countdict: per input, the key file (and count file) is loaded -- --presketched, or --cache and a complete file set -- or
// the input's exact set is computed on the GPU and the files are written
void exact_sets_job(Result &res, const Options &o, LazyCtx &lctx, ExactSets &es);
// --parse-by-seq --edit-distance --compute-edit-distance (K2h): the records of the one input file, read and checked on the host (no GPU
// is asked for before every refusal has had its say), then the context, the resident set and the dense outputs of their edit distances
int edit_distance_job(const Options &o);
void cmp_core_edit(const Options &o, Result &res, d2g_ctx *ctx, const d2g_seqrecs *sr, double t_read);   // cmp_dense.cpp
void apply_fmt_compat(Options &o);                                 // dashing2_main.cpp
// cmp_dense.cpp: every cmp output of an Options / Result pair; hands nearest neighbours and clustering on to cmp_sparse.cpp
void cmp_core(const Options &o, Result &res, d2g_ctx *ctx);
void cmp_core_exact(const Options &o, Result &res, d2g_ctx *ctx, const ExactSets &es);   // the same outputs from exact intersections
std::string context_switches_json(d2g_ctx *ctx);
// cmp_sparse.cpp: --topk / --similarity-threshold / --greedy (the values are a table of the equality count: `lut`)
const char *sparse_job_name(const Options &o);                     // "nearest neighbours" / "greedy clustering"; null: a dense job
void refuse_sparse_job_out_of_scope(const char *job, const Options &o, size_t S);   // returns when the job is in scope
void cmp_core_knn(const Options &o, const Result &res, d2g_ctx *ctx, const std::vector<float> &lut, double t_densify);
void cmp_core_dedup(const Options &o, const Result &res, d2g_ctx *ctx, const std::vector<float> &lut, double t_densify);

}  // namespace d2h
