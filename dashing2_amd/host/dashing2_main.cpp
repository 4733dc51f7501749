// dashing2_main.cpp -- drop-in `dashing2 sketch` / `dashing2 cmp` for the MI355X hot paths.
// Host C++ over the C ABI of libd2g.so (include/d2g.h); the jobs live in a file each (cli_common.h lists their entry points):
//   main / dispatch          src/d2.cpp:133-151                      this file
//   cmp_main / load_results  src/cmp_main.cpp:24-198,200-366         this file
//   sketch_main, sketch_core src/sketch_main.cpp:23-152 ...          sketch_cmd.cpp (host ingest: ingest_pipeline.h, bounded_queue.h)
//   cmp_core, dense outputs  src/cmp_core.cpp:686-751, emitrect.cpp  cmp_dense.cpp (row_batches.h, slot_queue.h)
//   neighbours, clustering   src/emitnn.cpp, src/dedup_core.cpp      cmp_sparse.cpp
//   contain_main             src/contain_main.cpp:133-299            contain_cmd.cpp (contain_files.h)
#include "cli_common.h"
#include "exact_files.h"
#include "fmtfloat.h"
#include <fstream>
#include <unistd.h>

namespace d2h {

int wsketch_main(int argc, char **argv);                          // wsketch_main.cpp
int contain_main(int argc, char **argv);                          // contain_cmd.cpp

namespace {

void load_results(Options &o, Result &res) {               // src/cmp_main.cpp:24-198
    const auto &paths = o.paths;
    if (paths.empty()) die("No paths provided to --presketched");
    const std::string &pf = paths.front();
    if (paths.size() == 1) {
        const std::string namesf = pf + ".names.txt";
        if (isfile(namesf)) {
            std::ifstream ifs(namesf);
            for (std::string l; std::getline(ifs, l);) {
                if (l.empty() || l.front() == '#') continue;
                res.names.emplace_back(l.substr(0, l.find_first_of('\t')));
            }
        }
        std::FILE *fp = std::fopen(pf.c_str(), "rb");
        if (!fp) die("Failed to open " + pf);
        uint64_t hdr[2];
        if (filesize(pf) < 16 || std::fread(hdr, 8, 2, fp) != 2)
            die("Failed to read num_entities from file " + pf + " of size " + std::to_string(filesize(pf)));
        const size_t N = hdr[0], S = hdr[1];
        o.sketchsize = S;
        if (res.names.empty()) for (size_t i = 0; i < N; ++i) res.names.push_back(std::to_string(i));
        res.cardinalities.resize(N);
        if (std::fread(res.cardinalities.data(), 8, N, fp) != N) die("Failed to read cardinalities from disk");
        const size_t nreg = (filesize(pf) - (N + 2) * 8) / 8;
        // (a private mapping of the file instead of this copy was measured: the page faults it moves into densify and the
        // upload cost more than the read -- config 4: 1.26 -> 1.43 s)
        res.signatures.resize(nreg);
        if (std::fread(res.signatures.data(), 8, nreg, fp) != nreg) die("Failed to read signatures from disk");
        std::fclose(fp);
        if (nreg != N * S) die("stacked sketch file " + pf + " has " + std::to_string(nreg) + " registers, expected " + std::to_string(N * S));
    } else {
        const size_t N = paths.size();
        std::vector<size_t> fs(N);
        for (size_t i = 0; i < N; ++i) {
            if (!isfile(paths[i])) { std::fprintf(stderr, "File does not exist at %s/%zu\n", paths[i].c_str(), i); std::exit(EXIT_FAILURE); }
            fs[i] = (filesize(paths[i]) - 8) / 8;
        }
        if (!std::all_of(fs.begin(), fs.end(), [&](size_t x) { return x == fs[0]; }))
            die("presketched files have uneven sizes; only sketches (not k-mer sets) are in this build's scope");
        o.sketchsize = fs[0];
        std::fprintf(stderr, "Sketchsize is now %zd\n", o.sketchsize);
        res.signatures.resize(N * fs[0]);
        res.cardinalities.resize(N);
        for (size_t i = 0; i < N; ++i) {
            std::FILE *fp = std::fopen(paths[i].c_str(), "rb");
            if (!fp || std::fread(&res.cardinalities[i], 8, 1, fp) != 1 ||
                std::fread(&res.signatures[i * fs[0]], 8, fs[0], fp) != fs[0]) {
                std::fprintf(stderr, "Failed to read at path %s\n", paths[i].c_str());
                std::exit(1);
            }
            std::fclose(fp);
        }
        // the reference leaves names_ empty here, so rows/sources are printed as E<i> (emitrect.cpp:145,176)
        for (size_t i = 0; i < N; ++i) res.names.push_back("E" + std::to_string(i));
    }
}

// the sketch size a --presketched job will find in its file(s) (load_results), from their sizes alone; 0: unknown
size_t presketched_sketchsize(const Options &o) {
    if (o.paths.empty()) return 0;
    if (o.paths.size() > 1) { const size_t fs = filesize(o.paths.front()); return fs >= 8 ? (fs - 8) / 8 : 0; }
    uint64_t hdr[2] = {0, 0};
    std::FILE *fp = std::fopen(o.paths.front().c_str(), "rb");
    if (!fp) return 0;
    const bool ok = std::fread(hdr, 8, 2, fp) == 2;
    std::fclose(fp);
    return ok ? size_t(hdr[1]) : 0;
}

// suffix sniffing, cmp_main.cpp:305-351: what the name of the first --presketched file says about the sketches
void sniff_presketched_suffix(Options &o) {
    const std::string &p0 = o.paths.empty() ? std::string() : o.paths.front();
    const auto dot = p0.find_last_of('.');
    const std::string suf = dot == std::string::npos ? std::string() : p0.substr(dot);
    if (suf == ".bmh" || suf == ".d2gbmh") {
        // stock BagMinHash sketches compare fine among themselves (equality counting does not care how registers were
        // drawn); what must never happen is one matrix over both kinds
        o.sspace = SPACE_MULTISET; o.kmer_result = FULL_SETSKETCH;
        for (const auto &p : o.paths) {
            const auto d2 = p.find_last_of('.');
            const std::string s2 = d2 == std::string::npos ? std::string() : p.substr(d2);
            if ((s2 == ".bmh" || s2 == ".d2gbmh") && s2 != suf)
                die("cannot compare stock dashing2 BagMinHash sketches (.bmh) with this build's BMH-D2G sketches (.d2gbmh): "
                    "their registers are drawn differently (see README)");
        }
    }
    else if (suf == ".pmh") { o.sspace = SPACE_PSET; o.kmer_result = FULL_SETSKETCH; }
    else if (suf == ".ss") { o.sspace = SPACE_SET; o.kmer_result = FULL_SETSKETCH; }
    else if (suf == ".opss") { o.sspace = SPACE_SET; o.kmer_result = ONE_PERM; }
    // cmp_main.cpp:335,343 compare the suffix with "mmerseq64" without its dot and the .kmerset64 arm never selects the count dictionary:
    // *.kmerset64 is --set unless --countdict was given
    else if (suf == ".kmerset64") { if (!o.exact) o.exact = 1; }
    else if (suf == ".kmerset128") die("128-bit k-mer set comparison is outside this build's hot-path scope");
}

int cmp_main(int argc, char **argv) {                             // src/cmp_main.cpp:200-366
    Options o;
    o.is_cmp = true;
    if (int rc = parse_options(argc, argv, o)) return rc - 1;
    apply_fmt_compat(o);
    const double t_begin = now();
    o.device = job_devices(o)[0];
    g_stats.on = !o.gpu_stats.empty(); g_stats.path = o.gpu_stats;
    g_stats.str("command", "cmp");
    if (o.edit) {
        if (o.paths.empty()) { std::fprintf(stderr, "No paths provided. See usage.\n"); cmp_usage(); return 1; }
        return edit_distance_job(o);
    }
    if (o.presketched) sniff_presketched_suffix(o);
    if (o.exact && sparse_job_name(o)) refuse_out_of_scope(std::string(sparse_job_name(o)) + " of exact k-mer sets (*.kmerset64)");
    if (o.exact && o.presketched)                                   // a missing file is named before a context is asked for
        for (const auto &p : o.paths) {
            uint64_t sz = 0;
            if (!exact_file_size(p, &sz)) die("File does not exist at " + p);
            if (o.exact == 2 && !exact_file_size(exact_count_file(p), &sz)) die("File does not exist at " + exact_count_file(p));
        }
    if (const char *sparse = sparse_job_name(o))                    // refused before a context exists
        if (const size_t S = o.presketched ? presketched_sketchsize(o) : o.sketchsize) refuse_sparse_job_out_of_scope(sparse, o, S);
    LazyCtx lctx(o, D2G_WARM_COPY | (o.exact ? D2G_WARM_KSET : D2G_WARM_K2) | (o.presketched ? 0 : o.bed ? D2G_WARM_K1I | (o.sspace == SPACE_MULTISET ? D2G_WARM_K3 : 0) : (o.sspace == SPACE_MULTISET || o.exact ? D2G_WARM_K3 : D2G_WARM_K1)));   // under the reading of the sketch file(s)
    Result res;
    ExactSets es;
    if (o.exact) {
        if (o.paths.empty()) { std::fprintf(stderr, "No paths provided. See usage.\n"); cmp_usage(); return 1; }
        exact_sets_job(res, o, lctx, es);
        res.nq = o.presketched ? 0 : o.nq;
    } else if (o.presketched) {
        load_results(o, res);
    } else {
        if (o.paths.empty()) { std::fprintf(stderr, "No paths provided. See usage.\n"); cmp_usage(); return 1; }
        if (o.bed) sketch_core_bed(res, o, lctx);
        else if (o.parse_by_seq) sketch_core_byseq(res, o, lctx); else sketch_core(res, o, lctx);
        res.nq = o.nq;
    }
    const double t_wait = now();
    d2g_ctx *ctx = lctx.get();
    if (o.verbosity) std::fprintf(stderr, "[d2g] inputs loaded in %.3fs; GPU context %.3fs + warm-up (first copy, code objects) %.3fs on a helper thread (%.3fs of it after the inputs were loaded)\n",
                                  t_wait - t_begin, lctx.t_create, lctx.t_warm, now() - t_wait);
    g_stats.nest("context", Json::object().num("create_s", lctx.t_create).num("warmup_s", lctx.t_warm).num("inputs_loaded_s", t_wait - t_begin)
                 .num("waited_for_context_s", now() - t_wait).raw("switches", context_switches_json(ctx)));
    const double t_cmp = now();
    if (o.exact) cmp_core_exact(o, res, ctx, es); else cmp_core(o, res, ctx);
    if (o.verbosity) std::fprintf(stderr, "[d2g] cmp_core %.3fs in all (densify, upload, batches, closing the output)\n", now() - t_cmp);
    return 0;
}

int main_usage() {                                                // src/d2.cpp:112-128
    std::fprintf(stderr, "dashing2 has several subcommands: sketch, cmp, wsketch, and contain.\n");
    std::fprintf(stderr, "Usage can be seen in those subcommands. (e.g., `dashing2 sketch -h`)\n\n");
    std::fprintf(stderr, "\tsketch: converts FastX into k-mer sets/sketches; also contains functionality from cmp, for one-step sketch and comparisons\n");
    std::fprintf(stderr, "\tcmp: compares previously sketched/decomposed k-mer sets and emits results. alias: dist\n\n");
    std::fprintf(stderr, "\twsketch: Takes a tuple of [1-3] input binary files [(u32 or u64), (float or double), (u32 or u64)] and performs weighted minhash sketching.\n");
    std::fprintf(stderr, "This MI355X build implements the sketch and cmp hot paths and wsketch's BagMinHash selections and contain (printmin is out of scope).\n");
    return 1;
}

}  // namespace

// D2_FMT_EXP_UPPER was the round-2 switch for the float text layout (7 = fmt >= 11, 16 = fmt < 11); --fmt-compat replaced it.  It is
// still honoured -- with a warning -- when --fmt-compat is not given, so that scripts written against round 2 keep their output.
void apply_fmt_compat(Options &o) {
    if (!o.fmt_compat)
        if (const char *e = std::getenv("D2_FMT_EXP_UPPER")) {
            const int v = std::atoi(e);
            if (v == 7 || v == 16) {
                o.fmt_compat = v == 7 ? 11 : 10;
                std::fprintf(stderr, "dashing2 (MI355X): D2_FMT_EXP_UPPER=%d is deprecated; use --fmt-compat %d\n", v, o.fmt_compat);
            } else std::fprintf(stderr, "dashing2 (MI355X): D2_FMT_EXP_UPPER=%s ignored (7 or 16; use --fmt-compat 10|11)\n", e);
        }
    if (o.fmt_compat) set_fmt_compat(o.fmt_compat);
}

}  // namespace d2h

int main(int argc, char **argv) {                                 // src/d2.cpp:133-151
    using namespace d2h;
    char cwd[4096];
    std::string cmd = argv[0][0] == '/' ? std::string(argv[0]) : (getcwd(cwd, sizeof cwd) ? std::string(cwd) + "/" + argv[0] : std::string(argv[0]));
    for (char **s = argv + 1; *s; ++s) cmd += std::string(" ") + *s;
    std::fprintf(stderr, "#Calling Dashing2 version %s with command '%s'\n", DASHING2_VERSION, cmd.c_str());
    if (argc > 1) {
        const bool is_sketch = std::strcmp(argv[1], "sketch") == 0, is_cmp = std::strcmp(argv[1], "cmp") == 0 || std::strcmp(argv[1], "dist") == 0;
        if (is_sketch || is_cmp) {
            const double t0 = now();
            const int rc = is_sketch ? sketch_main(argc - 1, argv + 1) : cmp_main(argc - 1, argv + 1);
            // every output file has been flushed and closed by now (Emitter / write_stacked go out of scope inside)
            std::fflush(nullptr);
            g_stats.num("in_process_s", now() - t0);
            g_stats.str("version", DASHING2_VERSION);
            g_stats.write();
            if (std::getenv("D2G_VERBOSE_EXIT")) std::fprintf(stderr, "[d2g] in-process time %.3fs\n", now() - t0);
            if (!g_release_at_exit) _exit(rc);
            return rc;
        }
        if (std::strcmp(argv[1], "wsketch") == 0) return wsketch_main(argc - 1, argv + 1);
        if (std::strcmp(argv[1], "contain") == 0) {
            const int rc = contain_main(argc - 1, argv + 1);
            std::fflush(nullptr);                                  // the output is closed; leave as sketch and cmp do
            if (!g_release_at_exit) _exit(rc);
            return rc;
        }
        if (std::strcmp(argv[1], "printmin") == 0) {
            std::fprintf(stderr, "dashing2 (MI355X): subcommand %s is outside the hot-path scope of this build.\n", argv[1]);
            return 1;
        }
    }
    return main_usage();
}
