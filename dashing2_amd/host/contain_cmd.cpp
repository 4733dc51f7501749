// contain_cmd.cpp -- `dashing2 contain`: reads screened against a k-mer database (reference src/contain_main.cpp:133-299, its
// mash-screen).  The database is the <out>.kmer64 of `sketch -s -o out`; per query file and reference the share of the reference's
// S sampled k-mers that occur in the query, and the floor of their mean count.  The per-k-mer lookup runs on the GPU (K1s,
// d2g_screen.hip); this file is the argument parser, the refusals, the query loop and the output.
#include "cli_common.h"
#include "contain_files.h"
#include <fstream>
#include <memory>
#include <unistd.h>

namespace d2h {

namespace {

int contain_usage() {                                             // src/contain_main.cpp:12-23
    std::fprintf(stderr, "Usage: dashing2 contain <flags> database.kmers <input.fq> <input2.fq>...\n"
                         "This application is inspired by mash screen.\n"
                         "Flags:\n"
                         "-h: help\n"
                         "-p: set number of threads. [1]\n"
                         "-o: Set output [stdout]\n"
                         "-b: Emit binary output instead of human-readable.\n"
                         "-F: read input paths from file at <arg>\n");
    return EXIT_FAILURE;
}

// a whole file of `len` bytes into page-aligned memory (the device parser's input); null: it could not be read
struct FreeDeleter { void operator()(void *p) const { std::free(p); } };
std::unique_ptr<uint8_t, FreeDeleter> read_whole(const std::string &path, size_t len) {
    void *p = nullptr;
    if (posix_memalign(&p, 4096, len + 64) != 0) die("out of memory (query file " + path + ")");
    std::unique_ptr<uint8_t, FreeDeleter> buf(static_cast<uint8_t *>(p));
    std::FILE *fp = std::fopen(path.c_str(), "rb");
    if (!fp) return nullptr;
    const size_t got = std::fread(buf.get(), 1, len, fp);
    std::fclose(fp);
    if (got != len) return nullptr;
    return buf;
}

}  // namespace

int contain_main(int argc, char **argv) {
    int nthreads = 1;
    bool binary_output = false;
    const char *outpath = nullptr;
    std::vector<std::string> queries;
    optind = 1;
    for (int c; (c = getopt(argc, argv, "bh?p:o:F:")) >= 0;) switch (c) {
        case 'h': case '?': return contain_usage();
        case 'p': nthreads = std::max(std::atoi(optarg), 1); break;
        case 'b': binary_output = true; break;
        case 'o': outpath = optarg; break;
        case 'F': {
            std::ifstream ifs(optarg);
            for (std::string line; std::getline(ifs, line);) queries.emplace_back(line);
            break;
        }
    }
    (void)nthreads;                                               // the lookup is the GPU's; the host packs one query at a time
    if (argc - optind == 0) return contain_usage();
    const std::string dbfile = argv[optind];
    queries.insert(queries.end(), argv + optind + 1, argv + argc);
    if (queries.empty()) {
        queries.push_back("/dev/stdin");
        std::fprintf(stderr, "No input files provided; this defaults to stdin. If this is in error, cancel dashing2.\n");
    }
    const size_t nq = queries.size();

    ContainDb db;
    std::string err;
    if (!load_contain_db(dbfile, db, err)) die(err);
    // what this build does not screen, said before a GPU context is asked for
    if (db.dtype != 0) refuse_out_of_scope("contain over a database that is not DNA (data type " + std::to_string(db.dtype) + " in its header)");
    if (db.S == 0) refuse_out_of_scope("contain over a database of sketch size 0");
    if (db.k > 32 || db.k == 0) refuse_out_of_scope("contain with k = " + std::to_string(db.k) + " (k-mers of 1 .. 32 bases are exact 64-bit keys; longer ones are rolling hashes)");
    // a header w <= k (0 included) is every k-mer.  A database of windowed minimizers (w > k, what `sketch -s -w` writes) stays refused
    // here: the library screens minimizers (d2g_sketcher_set_window + d2g_sketcher_run_screen), this command does not ask it to yet
    if (db.w > db.k) refuse_out_of_scope("contain over windowed minimizers (window " + std::to_string(db.w) + ", k " + std::to_string(db.k) + ")");
    if (db.nrefs > D2G_SCREEN_MAX_KEYS / db.S) refuse_out_of_scope("contain over a database of more than 2^30 keys (" + std::to_string(db.nrefs) + " references x " + std::to_string(db.S) + ")");
    Options o;
    if (const char *d = std::getenv("D2G_DEVICE")) o.device = std::atoi(d);
    if (const char *e = std::getenv("D2G_DEVICES")) {             // by its text, as the exact jobs do: counting devices would start the runtime
        if (*e && (std::strcmp(e, "all") == 0 || std::strchr(e, ','))) refuse_out_of_scope("contain with D2G_DEVICES naming several GPUs (a screen is resident on one)");
        if (*e) o.device = std::atoi(e);
    }

    const size_t nrefs = db.nrefs, S = db.S;
    const int k = int(db.k), canon = db.canon;
    const uint64_t xormask = d2g_seed_mask(db.seed);
    d2g_ctx *ctx = make_ctx(o);
    (void)d2g_warmup(ctx, D2G_WARM_COPY | D2G_WARM_SCREEN);

    // Q rows of counters, sized from the memory that is free: at most 4 N S bytes a row (every key distinct); the table, its ids,
    // the reference ids and the upload of the keys take at most 56 N S + a little.  Half of what is free stays for the queries.
    size_t free_b = 0, total_b = 0;
    check(ctx, d2g_mem_info(ctx, &free_b, &total_b), "d2g_mem_info");
    const size_t nkeys = std::max<size_t>(nrefs * S, 1), fixed = 56 * nkeys + (1u << 20), row_bytes = 4 * nkeys;
    size_t Q = free_b / 2 > fixed ? (free_b / 2 - fixed) / row_bytes : 1;
    Q = std::max<size_t>(1, std::min(Q, nq));
    if (const char *e = std::getenv("D2G_CONTAIN_ROWS")) { const long long v = std::atoll(e); if (v >= 1) Q = std::min<size_t>(size_t(v), nq); }   // debugging switch (README): fewer rows, more groups
    d2g_screen *screen = nullptr;
    check(ctx, d2g_screen_create(ctx, db.keys.data(), nrefs, S, k, canon, xormask, Q, &screen), "d2g_screen_create");
    d2g_sketcher *sk = nullptr;
    check(ctx, d2g_sketcher_create(ctx, &sk), "d2g_sketcher_create");
    d2g_seqpack *sp = nullptr;
    check(ctx, d2g_seqpack_create(k, &sp), "d2g_seqpack_create");
    const bool device_parse = std::getenv("D2G_DEVICE_PARSE") != nullptr && std::getenv("D2G_HOST_PARSE") == nullptr;

    size_t n_device_parsed = 0;
    std::vector<float> coverage(nq * nrefs), depth(nq * nrefs);
    std::vector<uint32_t> matches(Q * nrefs), matchsums(Q * nrefs);
    for (size_t q0 = 0; q0 < nq; q0 += Q) {
        const size_t nrow = std::min(Q, nq - q0);
        if (q0) check(ctx, d2g_screen_reset(ctx, screen), "d2g_screen_reset");
        for (size_t r = 0; r < nrow; ++r) {
            const std::string &path = queries[q0 + r];            // one path, one query: never split at spaces
            const uint32_t row = uint32_t(r);
            bool done = false;
            if (device_parse) {                                   // plain FASTA goes through K0; everything else through the host parser
                const size_t fsz = isfile(path) ? filesize(path) : 0;
                if (fsz && fsz < (size_t(1) << 31)) {
                    if (const auto raw = read_whole(path, fsz)) {
                        const uint64_t foff = 0, flen = fsz, gfo[2] = {0, 1};
                        const int rc = d2g_sketcher_ingest_fasta(sk, raw.get(), fsz, &foff, &flen, 1, gfo, 1, k);
                        if (rc == D2G_OK) {
                            const uint64_t *rs = nullptr, *go = nullptr; const uint32_t *rl = nullptr; size_t nrun = 0; uint64_t nb = 0;
                            check(ctx, d2g_sketcher_ingested_runs(sk, &rs, &rl, &nrun, &go, nullptr, &nb), "d2g_sketcher_ingested_runs");
                            check(ctx, d2g_sketcher_run_screen(sk, nullptr, 0, rs, rl, nrun, go, 1, k, canon, screen, &row), "d2g_sketcher_run_screen");
                            done = true;
                            ++n_device_parsed;
                        } else if (rc != D2G_ERR_UNSUPPORTED) check(ctx, rc, "d2g_sketcher_ingest_fasta");
                    }
                }
            }
            if (!done) {
                d2g_seqpack_clear(sp);
                if (d2g_seqpack_add_file(sp, path.c_str()) != D2G_OK) die("Failed to open " + path);
                check(ctx, d2g_sketcher_run_screen(sk, d2g_seqpack_packed(sp), d2g_seqpack_packed_bytes(sp), d2g_seqpack_run_start(sp), d2g_seqpack_run_len(sp),
                                                   d2g_seqpack_nruns(sp), d2g_seqpack_genome_run_off(sp), 1, k, canon, screen, &row), "d2g_sketcher_run_screen");
            }
        }
        check(ctx, d2g_screen_result(ctx, screen, 0, nrow, matches.data(), matchsums.data()), "d2g_screen_result");
        if (nrefs) check(ctx, d2g_epilogue_contain(matches.data(), matchsums.data(), nrow * nrefs, S, coverage.data() + q0 * nrefs, depth.data() + q0 * nrefs), "d2g_epilogue_contain");
    }

    // whoever asked for the device parser is told how often it applied (it takes plain FASTA; the host parser takes the rest)
    if (device_parse) std::fprintf(stderr, "[d2g] contain: %zu of %zu queries parsed on the device\n", n_device_parsed, nq);
    std::FILE *ofp = outpath ? std::fopen(outpath, "wb") : stdout;
    if (!ofp) die(std::string("Failed to open ") + outpath + " for writing.");
    const bool ok = binary_output ? write_contain_binary(ofp, nrefs, nq, coverage.data(), depth.data())
                                  : write_contain_text(ofp, db.names, queries, coverage.data(), depth.data());
    if (!ok) die("Failed to write the output");
    if (ofp != stdout) std::fclose(ofp);
    if (g_release_at_exit) { d2g_seqpack_destroy(sp); d2g_sketcher_destroy(sk); d2g_screen_destroy(screen); d2g_ctx_destroy(ctx); }
    return 0;
}

}  // namespace d2h
