// sketch_cmd.cpp -- `dashing2 sketch`: FASTX on disk -> stacked sketches, cache files, names.  Mirrors, for the in-scope options,
//   sketch_main              src/sketch_main.cpp:23-152
//   sketch_core + formats    src/sketch_core.cpp:14-31,108-161 ; src/fastxsketch.cpp:302-424,554-610
//   makedest (cache names)   src/fastxmerge.cpp:70-120
//   --parse-by-seq           src/fastxsketchbyseq.cpp:102-268,270-531
#include "cli_common.h"
#include "exact_files.h"
#include "ingest_pipeline.h"
#include <array>
#include <cinttypes>
#include <memory>
#include <new>

namespace d2h {

namespace {

// src/fastxmerge.cpp:70-120 for DNA, unspaced: OPH set sketches and exact-counting multiset sketches
std::string makedest(const Options &o, const std::string &path) {
    std::string ret = path.substr(0, path.find_first_of(' '));
    if (!o.outprefix.empty()) ret = o.outprefix + '/' + trim_folder(path);
    if (o.seedseed != 0) ret += ".seed" + std::to_string(o.seedseed);
    if (o.canon) ret += ".rc_canon";
    ret += ".sketchsize" + std::to_string(o.sketchsize);
    ret += ".k" + std::to_string(o.k);
    if (o.w > o.k) ret += ".w" + std::to_string(o.w);     // fastxmerge.cpp:87-90
    if (o.count_threshold > 0) {
        // fastxmerge.cpp:91-95 prints std::to_string(double) when fmod(threshold, 1) != 0 -- but Dashing2Options::count_threshold_ is a
        // uint32_t (d2.h:103) filled by std::atoi (options.h:352), so that branch cannot be reached from the reference's CLI
        // either: `-m 2.7` is 2 there and here.  The integer branch: std::to_string(int(count_threshold_)).
        ret += ".ct_threshold" + std::to_string(int(o.count_threshold));
    }
    // to_string(ct()), src/enums.cpp:47-48; fastxmerge.cpp:96-100.  opts.ct() is COUNTMIN_COUNTING whenever cssize > 0 (d2.h:207), whichever flag gave it
    if (o.sspace != SPACE_SET) ret += o.cssize ? ".CountMinCounting" + std::to_string(o.cssize) : std::string(".ExactCounting");
    ret += o.sspace == SPACE_SET ? ".SetSpace" : ".MultisetSpace";   // to_string(sspace), src/enums.cpp:40-46
    ret += std::string(".") + d2g_alphabet_name(o.alphabet);   // bns::to_string(rht_) (absent bonsai; "DNA", or the names of python/parse.py:8-23)
    // to_suffix, src/enums.cpp:28-38, gives ".bmh" for BagMinHash.  Multiset sketches of this build follow the repository's
    // BMH-D2G spec (the reference's sketch/bmh.h is absent): same layout, incomparable register values.  They get their own
    // suffix so that a --cache directory shared with a stock dashing2 can never mix the two silently.
    ret += o.sspace == SPACE_SET ? ".opss" : ".d2gbmh";
    return ret;
}

// one cached sketch: [f64 card][f64 x S]   (src/fastxsketch.cpp:60-112,556-607)
bool load_cached(const std::string &path, double *sig, double *card, size_t S) {
    if (filesize(path) != 8 + 8 * S) {
        if (isfile(path)) std::fprintf(stderr, "Expected %zu bytes of sketch, found %zu\n", S * 8, filesize(path) - 8);
        return false;
    }
    std::FILE *fp = std::fopen(path.c_str(), "rb");
    if (!fp) return false;
    const bool ok = std::fread(card, 8, 1, fp) == 1 && std::fread(sig, 8, S, fp) == S;
    std::fclose(fp);
    return ok;
}
void write_cached(const std::string &path, const double *sig, double card, size_t S) {
    std::FILE *fp = std::fopen(path.c_str(), "wb");
    if (!fp) die("Failed to open file " + path + " for writing sketch.");
    if (std::fwrite(&card, 8, 1, fp) != 1 || std::fwrite(sig, 8, S, fp) != S) die("Failed to write sketch " + path);
    std::fclose(fp);
}

// does this job save the k-mers (and counts) behind the registers?  Only next to a stacked output file (fastxsketch.cpp:236-244);
// without one the reference keeps them in memory and drops them
bool saves_kmers(const Options &o) { return o.save_kmers && !o.outfile.empty() && o.outfile != "-" && o.outfile != "/dev/stdout"; }

// <out>.kmer64: [u32 dtype = alphabet id (DNA 0) | canon << 8][u32 S][u32 k][u32 w][u64 seedseed], then N x S u64 (fastxsketch.cpp:245-259,619-620);
// <out>.kmer64.names.txt: the input lines (:260-263); <out>.kmercounts.f64: N x S float32 (sketch_core.cpp:162-171)
void write_kmer_files(const Result &res, const Options &o) {
    if (res.kmers.empty() && res.kmercounts.empty()) return;
    std::FILE *fp;
    if (!res.kmers.empty()) {
        const std::string kf = o.outfile + ".kmer64", nf = kf + ".names.txt";
        if (!(fp = std::fopen(kf.c_str(), "wb"))) die("Failed to open " + kf + " for writing.");
        const uint32_t hdr[4] = {uint32_t(o.alphabet) | (uint32_t(o.canon) << 8), uint32_t(o.sketchsize), uint32_t(o.k), uint32_t(o.w < 0 ? o.k : o.w)};
        const uint64_t seed = o.seedseed;
        if (std::fwrite(hdr, 4, 4, fp) != 4 || std::fwrite(&seed, 8, 1, fp) != 1 ||
            std::fwrite(res.kmers.data(), 8, res.kmers.size(), fp) != res.kmers.size()) die("Failed to write " + kf);
        std::fclose(fp);
        if (!(fp = std::fopen(nf.c_str(), "wb"))) die("Failed to open " + nf + " for writing.");
        for (const auto &n : res.names) { std::fwrite(n.data(), 1, n.size(), fp); std::fputc('\n', fp); }
        std::fclose(fp);
    }
    if (!res.kmercounts.empty()) {
        const std::string cf = o.outfile + ".kmercounts.f64";
        if (!(fp = std::fopen(cf.c_str(), "wb"))) return;                 // the reference fails silently here (sketch_core.cpp:168-170)
        if (std::fwrite(res.kmercounts.data(), sizeof(float), res.kmercounts.size(), fp) != res.kmercounts.size()) die("Failed to write " + cf);
        std::fclose(fp);
    }
}

// stacked output: [u64 N][u64 S][f64 card x N][f64 x N*S]   (sketch_core.cpp:130-140, fastxsketch.cpp:236-240)
void write_stacked(const Result &res, const Options &o) {
    const size_t N = res.names.size(), S = o.sketchsize;
    if (o.outfile.empty()) return;
    if (o.outfile == "-" || o.outfile == "/dev/stdout")
        die("Not yet supported: writing stacked sketches to file streams. This may change.");     // sketch_core.cpp:141-144
    std::FILE *fp = std::fopen(o.outfile.c_str(), "wb");
    if (!fp) die("Failed to open file " + o.outfile + " for in-place modification");
    const uint64_t hdr[2] = {uint64_t(N), uint64_t(S)};
    if (std::fwrite(hdr, 8, 2, fp) != 2 || std::fwrite(res.cardinalities.data(), 8, N, fp) != N ||
        std::fwrite(res.signatures.data(), 8, N * S, fp) != N * S) die("Failed to write " + o.outfile);
    std::fclose(fp);
    // <out>.names.txt (sketch_core.cpp:146-161, enums.h:160 "%0.24g")
    const std::string nf = o.outfile + ".names.txt";
    if (!(fp = std::fopen(nf.c_str(), "wb"))) die("Failed to open outfile at " + nf);
    std::fputs("#Name\tCardinality\n", fp);
    for (size_t i = 0; i < N; ++i) {
        std::fwrite(res.names[i].data(), 1, res.names[i].size(), fp);
        std::fprintf(fp, "\t%0.24g", res.cardinalities[i]);
        if (!res.kmercountfiles.empty()) { std::fputc('\t', fp); std::fwrite(res.kmercountfiles[i].data(), 1, res.kmercountfiles[i].size(), fp); }   // sketch_core.cpp:156-157
        std::fputc('\n', fp);
    }
    std::fclose(fp);
    write_kmer_files(res, o);
}

// A packed run stream as the d2g_sketcher_run_* / d2g_kmer_filter_create_* calls take it: the symbols, the runs of valid ones, the runs
// of each of the n genomes (goff[0 .. n]).  packed == NULL: the stream the sketcher ingested on the device (d2g_sketcher_ingest_fasta).
struct RunStream {
    const uint8_t *packed = nullptr; size_t packed_bytes = 0;
    const uint64_t *run_start = nullptr; const uint32_t *run_len = nullptr; size_t nrun = 0;
    const uint64_t *goff = nullptr; size_t n = 0; uint64_t nbases = 0;
    static RunStream of(d2g_seqpack *sp) {
        return {d2g_seqpack_packed(sp), d2g_seqpack_packed_bytes(sp), d2g_seqpack_run_start(sp), d2g_seqpack_run_len(sp), d2g_seqpack_nruns(sp),
                d2g_seqpack_genome_run_off(sp), d2g_seqpack_ngenomes(sp), d2g_seqpack_nbases(sp)};
    }
};

// --filterset (Dashing2Options::filterset, src/d2.cpp:45-98; asked per k-mer at src/fastxsketch.cpp:387): the filter file(s) are
// parsed and 2-bit-packed ONCE per job, as one sketch input line is; every GPU context of the job builds its own table from that
// stream (a table lives in one context's device memory) and attaches it to its sketcher before the first batch.
struct JobFilter {
    d2g_seqpack *sp = nullptr;                            // null: no --filterset
    std::mutex mu;
    bool reported = false;                                // --gpu-stats "filter": the first table built speaks for all
    explicit JobFilter(const Options &o) {
        if (o.filterset.empty()) return;
        check(nullptr, d2g_seqpack_create_alphabet(o.k, o.alphabet, &sp), "d2g_seqpack_create");    // the filter file under the job's alphabet
        if (d2g_seqpack_add_path(sp, o.filterset.c_str()) != D2G_OK) die("Failed to open file " + o.filterset + " for reading");   // d2.cpp:63
        o.filterset_built = true;
        o.filterset_size = 0;                             // occurrences: the reference sorts but never deduplicates (filterset.h:82);
        const uint32_t *rl = d2g_seqpack_run_len(sp);     // with -w the filter file's minimizers, one per window position (options.h:556)
        for (size_t r = 0, nr = d2g_seqpack_nruns(sp); r < nr; ++r) o.filterset_size += d2g_run_emissions(rl[r], o.k, o.w);
        if (o.cache) std::fprintf(stderr, "dashing2 (MI355X): warning: --cache with --filterset: cache file names do not carry the filter "
                                          "(fastxmerge.cpp:70-120); existing caches are loaded as they are, filtered or not.\n");
    }
    ~JobFilter() { if (sp) d2g_seqpack_destroy(sp); }
    // the table of one context, attached to its sketcher (JobSketcher, which also releases it)
    d2g_kmer_filter *attach(d2g_ctx *ctx, d2g_sketcher *sk, const Options &o) {
        if (!sp) return nullptr;
        d2g_kmer_filter *f = nullptr;
        const RunStream s = RunStream::of(sp);
        if (o.alphabet) check(ctx, d2g_kmer_filter_create_alphabet(ctx, s.packed, s.packed_bytes, s.run_start, s.run_len, s.nrun, o.k, o.alphabet, &f), "d2g_kmer_filter_create");
        else check(ctx, d2g_kmer_filter_create_windowed(ctx, s.packed, s.packed_bytes, s.run_start, s.run_len, s.nrun, o.k, o.canon, o.w, &f), "d2g_kmer_filter_create");
        check(ctx, d2g_sketcher_set_filter(sk, f), "d2g_sketcher_set_filter");
        std::lock_guard<std::mutex> lk(mu);
        if (g_stats.on && !reported) {
            reported = true;
            uint64_t nocc = 0, ndist = 0; size_t bytes = 0;
            check(ctx, d2g_kmer_filter_info(ctx, f, &nocc, &ndist, &bytes), "d2g_kmer_filter_info");
            g_stats.nest("filter", Json::object().integer("kmers", nocc).integer("distinct", ndist).integer("table_bytes", bytes).num("build_ms", kernel_acc(ctx, "filter").last_ms));
        }
        return f;
    }
};

// The sketcher of one job on one context, set up as every sketching job wants it: the window (-w > k: minimizers, K1w), the alphabet
// (--protein...: amino-acid k-mers, K1a) and the job's --filterset table, attached before the first batch.  Sketcher and table are
// released only on request, like everything else the process holds when it leaves (g_release_at_exit).
struct JobSketcher {
    d2g_ctx *const ctx; const Options &o;
    d2g_sketcher *sk = nullptr; d2g_kmer_filter *kf = nullptr;
    JobSketcher(d2g_ctx *c, const Options &oo, JobFilter &filter) : ctx(c), o(oo) {
        check(ctx, d2g_sketcher_create(ctx, &sk), "d2g_sketcher_create");
        check(ctx, d2g_sketcher_set_window(sk, o.w), "d2g_sketcher_set_window");
        check(ctx, d2g_sketcher_set_alphabet(sk, o.alphabet), "d2g_sketcher_set_alphabet");
        kf = filter.attach(ctx, sk, o);
    }
    ~JobSketcher() { if (g_release_at_exit) { d2g_sketcher_destroy(sk); d2g_kmer_filter_destroy(kf); } }
    JobSketcher(const JobSketcher &) = delete;
    JobSketcher &operator=(const JobSketcher &) = delete;
    operator d2g_sketcher *() const { return sk; }
    // one of the d2g_sketcher_run_* entry points over a stream: they all begin (sketcher, stream, k, canon, seed mask: d2.h:224 -> enums.cpp:131-140)
    template <class Fn, class... Tail> void run(Fn fn, const char *what, const RunStream &s, Tail... tail) const {
        check(ctx, fn(sk, s.packed, s.packed_bytes, s.run_start, s.run_len, s.nrun, s.goff, s.n, o.k, o.canon, d2g_seed_mask(o.seedseed), tail...), what);
    }
};

// x87 finalisation (getcard / data, src/oph.h:240-263) and cache files leave the device threads through a small queue
struct Fin { size_t g; std::vector<uint64_t> regs; std::vector<double> sigs, cards; std::vector<uint32_t> counts; };   // counts: [n][m] with -N

constexpr int NSK = 7, NSK_ALWAYS = 3, NSK_CS = 4;
// k1count: reported only by jobs that count (-N with -o); k3k, k3kcompact, k3kbmh: only by --multiset -c jobs (the count-sketch chain)
constexpr const char *SKETCH_KERNELS[NSK] = {"k0", "k1", "k3", "k1count", "k3k", "k3kcompact", "k3kbmh"};

// What the device threads of one sketch job share.  `const` members and what they point to are read-only while the threads run.
struct DeviceSide {
    const Options &o;
    const std::vector<size_t> &todo;
    const GroupPlan &plan;
    IngestPipeline &pipe;
    BoundedQueue<Fin> &finq;
    JobFilter &filter;
    const std::vector<int> devs;
    const bool count_kmers;                               // -N with -o: K1 is followed by its count pass
    d2g_ctx *const first_ctx;                             // the context of thread 0; every other thread makes its own
    std::mutex mu;                                        // guards everything below: each thread adds its sums once, as it ends
    double t_gpu = 0;
    uint64_t total_bases = 0;
    size_t n_dev_groups = 0, n_host_groups = 0;
    std::vector<std::array<KAcc, NSK>> kacc;              // per device: k0, k1, k3, k1count
    std::vector<size_t> groups_of;                        // per device
    uint64_t cs_table_bytes = 0, cs_groups = 0, cs_batches = 0;   // -c: the largest count-sketch table of any thread, the table groups and batches of all

    // sketches one group: the raw bytes parsed on the device, or the stream the host parser packed -> Fin; true: parsed on the device
    bool sketch_group(d2g_ctx *ctx, const JobSketcher &sk, IngestGroup &r, Fin &f, uint64_t &nb) {
        const size_t S = o.sketchsize, b = plan.groups[r.g].first, e = plan.groups[r.g].second, n = e - b;
        // the packed run stream of the group: parsed on the device (packed == NULL below), or by the host parser
        RunStream s;
        bool on_device = false;
        if (r.buf >= 0) {
            const int rc = d2g_sketcher_ingest_fasta(sk, r.raw, r.raw_bytes, r.foff.data(), r.flen.data(), r.foff.size(), r.gfo.data(), n, o.k);
            if (rc == D2G_OK) check(ctx, d2g_sketcher_ingested_runs(sk, &s.run_start, &s.run_len, &s.nrun, &s.goff, nullptr, &s.nbases), "d2g_sketcher_ingested_runs");
            pipe.release_buffer(r);
            if (rc == D2G_ERR_UNSUPPORTED) {                            // e.g. a '+' line further down: the host parser takes the group
                check(ctx, d2g_seqpack_create_alphabet(o.k, o.alphabet, &r.sp), "d2g_seqpack_create");
                for (size_t x = b; x < e; ++x)
                    if (d2g_seqpack_add_path(r.sp, o.paths[todo[x]].c_str()) != D2G_OK) die("Failed to open " + o.paths[todo[x]]);
            } else check(ctx, rc, "d2g_sketcher_ingest_fasta");
            on_device = rc == D2G_OK;
        }
        if (r.sp) s = RunStream::of(r.sp);
        s.n = n;
        nb = s.nbases;
        if (o.sspace == SPACE_MULTISET) {
            // fastxsketch.cpp:425-445: Counter -> BagMinHash; cardinality = total weight, signature = data()[0..S)
            f.sigs.resize(n * S); f.cards.resize(n);
            if (o.cssize)                                               // -c: Counter(cssize), counter.h:74-75,131-137 (K3k)
                sk.run(d2g_sketcher_run_bmh_cs, "d2g_sketcher_run_bmh_cs", s, S, o.cssize, double(o.count_threshold), f.sigs.data(), f.cards.data());
            else sk.run(d2g_sketcher_run_bmh, "d2g_sketcher_run_bmh", s, S, double(o.count_threshold), f.sigs.data(), f.cards.data());
        } else {
            f.regs.resize(n * d2g_oph_m(S));
            if (count_kmers) f.counts.resize(n * d2g_oph_m(S));         // -N with -o: idcounts(), fastxsketch.cpp:590-591
            uint32_t *const counts = count_kmers ? f.counts.data() : nullptr;
            if (o.count_threshold >= 2)                                 // fastxsketch.cpp:192: set_mincount(count_threshold_); with -N idcounts() too
                sk.run(d2g_sketcher_run_mincount, "d2g_sketcher_run_mincount", s, S, o.count_threshold, f.regs.data(), counts);
            else if (count_kmers) sk.run(d2g_sketcher_run_counts, "d2g_sketcher_run_counts", s, S, f.regs.data(), counts);
            else sk.run(d2g_sketcher_run, "d2g_sketcher_run", s, S, f.regs.data());
        }
        return on_device;
    }

    // one device thread: its own context + sketcher (a d2g_ctx is used by one thread at a time), groups until the pipeline ends
    void run(d2g_ctx *ctx, size_t di) {
        if (!ctx) {                                                         // every thread but the first makes its own context, in parallel
            const int rc = d2g_ctx_create(devs[di], &ctx);
            if (rc != D2G_OK) die(std::string("d2g_ctx_create (device thread, GPU ") + std::to_string(devs[di]) + "): " + d2g_strerror(rc));
            if (g_stats.on) (void)d2g_set_timing(ctx, TIME_ALL);
        }
        double gpu = 0; uint64_t bases = 0; size_t ndevg = 0, nhostg = 0;
        std::array<KAcc, NSK> mine;
        uint64_t cs_b = 0, cs_g = 0, cs_n = 0;
        {
            JobSketcher sk(ctx, o, filter);                                 // the filter table is attached before the first group
            for (IngestGroup r; pipe.next(r);) {
                if (r.failed()) continue;                                   // error recorded by the pipeline; drain the queue
                const double t1 = now();
                Fin f{r.g, {}, {}, {}, {}};
                uint64_t nb = 0;
                ++(sketch_group(ctx, sk, r, f, nb) ? ndevg : nhostg);
                gpu += now() - t1; bases += nb;
                finq.push(std::move(f));
                pipe.release(r);
            }
            if (g_stats.on) for (int x = 0; x < NSK; ++x) mine[x] = kernel_acc(ctx, SKETCH_KERNELS[x]);
            if (g_stats.on && o.cssize) (void)d2g_countsketch_stats(ctx, &cs_b, &cs_g, &cs_n);
        }                                                                   // the sketcher goes before its context
        if (g_release_at_exit && ctx != first_ctx) d2g_ctx_destroy(ctx);
        std::lock_guard<std::mutex> lk(mu);
        cs_table_bytes = std::max(cs_table_bytes, cs_b); cs_groups += cs_g; cs_batches += cs_n;
        t_gpu += gpu; total_bases += bases; n_dev_groups += ndevg; n_host_groups += nhostg;
        groups_of[di] += ndevg + nhostg;
        for (int x = 0; x < NSK; ++x) kacc[di][x] += mine[x];
    }
};

}  // namespace

// Host ingest pipeline (ingest_pipeline.h).  Reader threads read() whole groups of FASTA files into staging
// buffers, or parse and pack them themselves; device threads own a GPU context each: one uploads a group's raw bytes, K0 parses
// and 2-bit-packs them on the device (d2g_sketcher_ingest_fasta), K1 / K3 sketch the stream; a finisher thread finalises the
// registers (x87) and writes the cache files.  Inputs the device parser refuses (gz members, FASTQ, leading junk: first byte is
// not '>') are parsed by the host parser (d2g_seqpack) on the reader thread instead, group by group.
// WHICH PARSER IS THE DEFAULT -- measured, 1000 x 5 Mbp FASTA in the page cache, 16 usable cores (profiles/r03_e2e_cli.txt):
// read()ing a group into staging costs a core as much as read()ing + packing it (22 vs 19 ms per 43 MB: the copy out of the
// page cache into memory that is not cache-resident is the expensive half, and the packer works on a 5 MB buffer that
// stays in L2), the device threads are not the bottleneck either way, and 0.8 GB of page-locked staging adds ~0.07 s of
// teardown when the process exits.  So the device parser buys nothing end to end on this host and the HOST parser stays
// the default; D2G_DEVICE_PARSE=1 selects the hybrid (device parser whenever a staging buffer is free).
// The staging buffers are plain memory the readers fill at once; they are page-locked (d2g_host_register) as soon as the
// GPU context exists, so neither the context creation nor the pinning delays the reading.
void sketch_core(Result &res, const Options &o, LazyCtx &lctx) {
    const double t_enter = now();
    const size_t N = o.paths.size(), S = o.sketchsize, m = d2g_oph_m(S);
    if (!N) die("Can't sketch empty path set");
    res.names = o.paths;                                                // fastxsketch.cpp:625
    res.destination_files.resize(N);
    res.cardinalities.assign(N, -1.);
    res.signatures.assign(N * S, 0.);
    const bool want_ids = saves_kmers(o), want_counts = want_ids && o.save_kmercounts;
    JobFilter filter(o);
    if (o.save_kmercounts) res.kmercountfiles.resize(N);                // fastxsketch.cpp:280-282
    if (want_ids) res.kmers.assign(N * S, 0);                           // :293-298
    if (want_counts) res.kmercounts.assign(N * S, 0.f);
    std::vector<size_t> todo;
    std::vector<std::string> lines;                                     // o.paths[todo[t]]
    for (size_t i = 0; i < N; ++i) {
        res.destination_files[i] = makedest(o, o.paths[i]);
        if (o.save_kmercounts) {                                        // fastxsketch.cpp:314,317,326: named, never written for OPH
            const std::string &d = res.destination_files[i];
            res.kmercountfiles[i] = d.substr(0, d.find_last_of('.')) + ".kmercounts.f64";
        }
        // with -s / -N the reference's cache test also wants per-input k-mer files (fastxsketch.cpp:327-331), which its OPH branch
        // never writes: it always sketches again.  So does this build; the caches are still written.
        if (o.cache && !o.save_kmers && isfile(res.destination_files[i]) &&
            load_cached(res.destination_files[i], &res.signatures[i * S], &res.cardinalities[i], S))
            continue;                                                   // fastxsketch.cpp:327-373
        todo.push_back(i);
        lines.push_back(o.paths[i]);
    }
    const GroupPlan plan = plan_groups(lines, group_bytes_limit(size_t(48) << 20));
    const auto &groups = plan.groups;
    const double t_setup = now();
    const std::vector<int> devs = job_devices(o);
    const bool force_host = std::getenv("D2G_DEVICE_PARSE") == nullptr || std::getenv("D2G_HOST_PARSE") != nullptr || devs.size() > 1 ||
                            o.alphabet != 0;                            // K0 parses DNA: amino-acid inputs go through the host parser
    const IngestConfig cfg = ingest_config(plan, o.k, size_t(o.workers()), force_host, o.alphabet);
    std::unique_ptr<IngestPipeline> pipe;
    try { pipe.reset(new IngestPipeline(lines, plan, cfg)); } catch (const std::bad_alloc &) { die("out of memory (ingest staging)"); }
    d2g_ctx *ctx = lctx.get();                                          // the readers are busy: now wait for the GPU context
    double t_pin = now();
    for (const auto &b : pipe->buffers()) check(ctx, d2g_host_register(ctx, b.first, b.second), "d2g_host_register");
    t_pin = now() - t_pin;
    BoundedQueue<Fin> finq(groups.size() + 1);                          // never full: the device threads do not wait for the finisher
    double t_fin = 0;                                                   // written by the finisher only, read after its join
    std::thread finisher([&] {
        std::vector<uint64_t> ids;
        for (Fin f; finq.pop(f);) {
            const double t0 = now();
            const size_t b = groups[f.g].first, e = groups[f.g].second, n = e - b;
            if (!f.regs.empty()) {
                f.sigs.resize(n * S); f.cards.resize(n);
                check(nullptr, d2g_oph_finalize(f.regs.data(), n, m, S, f.sigs.data(), f.cards.data(), 2), "d2g_oph_finalize");
            }
            if (want_ids) {                                             // ids(): oph.h:264-271
                ids.resize(n * S);
                check(nullptr, d2g_oph_kmer_ids(f.regs.data(), n, m, S, ids.data()), "d2g_oph_kmer_ids");
            }
            for (size_t t = b; t < e; ++t) {                            // results land by input index
                const size_t i = todo[t];
                if (want_ids) std::memcpy(&res.kmers[i * S], &ids[(t - b) * S], S * sizeof(uint64_t));         // fastxsketch.cpp:619-620
                if (want_counts) for (size_t r = 0; r < S; ++r) res.kmercounts[i * S + r] = float(f.counts[(t - b) * m + r]);   // :621-622
                std::memcpy(&res.signatures[i * S], &f.sigs[(t - b) * S], S * sizeof(double));   // fastxsketch.cpp:610
                res.cardinalities[i] = f.cards[t - b];
                if (o.cache) write_cached(res.destination_files[i], &f.sigs[(t - b) * S], f.cards[t - b], S);
            }
            t_fin += now() - t0;
        }
    });
    // Device threads: two per GPU, each with its own context + sketcher -- the upload of one group overlaps the kernels and the
    // synchronisations of the other.  D2G_DEVICES names several GPUs: every GPU gets its pair of threads and all of them take groups
    // from the one pipeline (inputs dealt to the GPUs as they come free: file-sharded, no collectives -- SURVEY 8e; the loop being
    // sharded is the reference's `for` over files, src/fastxsketch.cpp:302); the stacked output is in input order whatever GPU
    // sketched a group.
    int ndev = groups.size() > 1 ? 2 : 1;
    if (const char *e = std::getenv("D2G_DEVICE_THREADS")) { const int v = std::atoi(e); if (v >= 1 && v <= 8) ndev = v; }
    const size_t nthreads_dev = std::max<size_t>(1, std::min<size_t>(size_t(ndev) * devs.size(), std::max<size_t>(groups.size(), 1)));
    DeviceSide ds{o, todo, plan, *pipe, finq, filter, devs, want_counts, ctx, {}, 0, 0, 0, 0, std::vector<std::array<KAcc, NSK>>(devs.size()), std::vector<size_t>(devs.size(), 0)};
    std::vector<std::thread> more;
    const double t_dev0 = now();
    for (size_t t = 1; t < nthreads_dev; ++t) more.emplace_back([&ds, t, ndev] { ds.run(nullptr, t / size_t(ndev)); });
    const double t_dev1 = now();
    ds.run(ctx, 0);
    for (auto &th : more) th.join();
    const double t_dev2 = now();
    finq.close();
    finisher.join();
    if (o.verbosity) std::fprintf(stderr, "[d2g] device side: %zu device threads over %zu GPU(s) (started in %.3fs), device loops %.3fs wall, drain of the finisher %.3fs\n", nthreads_dev,
                                  devs.size(), t_dev1 - t_dev0, t_dev2 - t_dev1, now() - t_dev2);
    pipe->join();
    const double t_pipe = now();
    // the staging buffers stay page-locked until the process ends (it leaves through _exit): unpinning 0.8 GB costs more than
    // the whole device work of a small job; D2G_FULL_TEARDOWN=1 releases them
    if (g_release_at_exit) for (const auto &b : pipe->buffers()) (void)d2g_host_unregister(ctx, b.first);
    else pipe->abandon_buffers();
    if (!pipe->error().empty()) die(pipe->error());
    if (o.verbosity) std::fprintf(stderr, "[d2g] sketched %zu inputs (%" PRIu64 " bases in the packed streams) in %zu groups (%zu parsed on the device, %zu by the host "
                                          "parser): reader threads %.3fs in all (%.3fs reading raw groups, %.3fs reading + packing, the rest waiting for queue space) over %zu threads, device threads: H2D+K0+K1+D2H %.3fs busy in all, finisher thread: x87 finalise+cache %.3fs; "
                                          "%zu staging buffers of %zu MiB page-locked in %.3fs\n",
                                  todo.size(), ds.total_bases, groups.size(), ds.n_dev_groups, ds.n_host_groups, pipe->t_readers(), pipe->t_read_raw(), pipe->t_host_pack(), cfg.readers,
                                  ds.t_gpu, t_fin, cfg.nbufs, cfg.buf_bytes >> 20, t_pin);
    if (o.verbosity) std::fprintf(stderr, "[d2g] sketch wall: setup (stat, cache probe) %.3fs, ingest pipeline %.3fs\n", t_setup - t_enter, t_pipe - t_setup);
    if (g_stats.on) {
        const bool multiset = o.sspace == SPACE_MULTISET, countsketch = multiset && o.cssize != 0;
        Json dj = Json::array();
        for (size_t d = 0; d < devs.size(); ++d) {
            Json e = device_json(devs[d]);
            e.integer("groups", ds.groups_of[d]);
            for (int x = 0; x < NSK; ++x) {
                if (x == NSK_ALWAYS ? !want_counts : x >= NSK_CS ? !countsketch : false) continue;
                e.nest(SKETCH_KERNELS[x], ds.kacc[d][x].json());
            }
            dj.push(e);
        }
        if (countsketch)
            g_stats.nest("countsketch", Json::object().integer("cells", o.cssize).integer("table_bytes", ds.cs_table_bytes).integer("table_groups", ds.cs_groups)
                         .integer("batches", ds.cs_batches));
        // ceil(L/4) + 8 m per input (set sketches), + 8 for the total weight of a multiset sketch
        const double alg = double((ds.total_bases + 3) / 4) + double(todo.size()) * (8.0 * double(multiset ? S : m) + (multiset ? 8.0 : 0.0));
        g_stats.nest("sketch", Json::object().integer("inputs", N).integer("sketched", todo.size()).integer("from_cache", N - todo.size()).integer("k", o.k)
                     .integer("sketchsize", S).str("space", countsketch ? "multiset (K3k: count-sketch + BagMinHash)" : multiset ? "multiset (K3: counts + BagMinHash)" : "set (K1: OPH)").integer("groups", groups.size())
                     .integer("groups_parsed_on_device", ds.n_dev_groups).integer("bases", ds.total_bases).num("algorithmic_bytes", alg)
                     .integer("device_threads", nthreads_dev).integer("parser_threads", cfg.readers).nest("devices", dj)
                     .nest("wall_s", Json::object().num("setup", t_setup - t_enter).num("ingest_pipeline", t_pipe - t_setup).num("device_loops", t_dev2 - t_dev1)
                           .num("device_threads_busy_sum", ds.t_gpu).num("parser_threads_sum", pipe->t_readers()).num("finisher_x87_and_cache", t_fin)));
    }
    pipe.reset();
    write_stacked(res, o);
}

// --parse-by-seq (sketch_core.cpp:23-29 -> fastxsketchbyseq.cpp:102-268,270-531): one sketch per record of
// ONE input file; OPH set sketches (cardinality = exact distinct k-mer count when the estimate is below
// 10 S, lines 415-430) or multiset sketches; names are the record names.
void sketch_core_byseq(Result &res, const Options &o, LazyCtx &lctx) {
    if (o.paths.size() != 1)
        die("parse-by-seq currently only handles one file at a time. To process multiple files, simply concatenate them into one file, and run dashing2 on that.");
    const size_t S = o.sketchsize, m = d2g_oph_m(S);
    d2g_seqpack *sp = nullptr;
    check(nullptr, d2g_seqpack_create_alphabet(o.k, o.alphabet, &sp), "d2g_seqpack_create");
    const uint64_t per_byte = o.alphabet ? 1 : 4;                                  // symbols per stream byte: a byte per residue, four bases
    if (d2g_seqpack_add_path_by_record(sp, o.paths[0].c_str()) != D2G_OK) die("Failed to read from " + o.paths[0]);
    d2g_ctx *ctx = lctx.get();
    const size_t N = d2g_seqpack_ngenomes(sp);
    res.names.resize(N);
    for (size_t i = 0; i < N; ++i) res.names[i] = d2g_seqpack_name(sp, i);
    res.destination_files.assign(N, std::string());
    res.cardinalities.assign(N, 0.);
    res.signatures.assign(N * S, 0.);
    const RunStream all = RunStream::of(sp);
    JobFilter filter(o);
    JobSketcher sk(ctx, o, filter);                                                // fastxsketchbyseq.cpp:327,370,383,420-423
    std::vector<uint64_t> regs, rs_rel, goff_rel, ndist;
    std::vector<double> sigs, cards;
    const size_t max_rec = std::max<size_t>(1, (size_t(64) << 20) / m);            // <= 512 MiB of registers per launch
    for (size_t g0 = 0; g0 < N;) {
        // batch [g0, g1): bounded by records and by packed bytes (the slice is re-based so that only it is uploaded)
        size_t g1 = g0;
        const uint64_t r0 = all.goff[g0];
        const uint64_t base0 = r0 < all.goff[N] ? (all.run_start[r0] & ~uint64_t(15)) : 0;
        while (g1 < N && g1 - g0 < max_rec) {
            const uint64_t r1 = all.goff[g1 + 1];
            const uint64_t endb = r1 > r0 ? all.run_start[r1 - 1] + all.run_len[r1 - 1] : base0;
            if (g1 > g0 && endb - base0 > (uint64_t(192) << 20)) break;            // ~48 MB of packed bases
            ++g1;
        }
        const size_t n = g1 - g0, r1 = all.goff[g1], nrun = r1 - r0;
        rs_rel.resize(nrun); goff_rel.resize(n + 1);
        for (size_t r = 0; r < nrun; ++r) rs_rel[r] = all.run_start[r0 + r] - base0;
        for (size_t g = 0; g <= n; ++g) goff_rel[g] = all.goff[g0 + g] - r0;
        const uint64_t endb = nrun ? all.run_start[r1 - 1] + all.run_len[r1 - 1] : base0;
        // the slice + its 64 readable pad bytes; base0 is a multiple of 16 symbols: 4-byte aligned either way
        const RunStream b{all.packed + base0 / per_byte, std::min<size_t>(all.packed_bytes - base0 / per_byte, (endb - base0 + per_byte - 1) / per_byte + 64),
                          rs_rel.data(), all.run_len + r0, nrun, goff_rel.data(), n, 0};
        sigs.resize(n * S); cards.resize(n);
        if (o.sspace == SPACE_MULTISET) {
            sk.run(d2g_sketcher_run_bmh, "d2g_sketcher_run_bmh", b, S, double(o.count_threshold), sigs.data(), cards.data());
        } else {
            regs.resize(n * m);
            sk.run(d2g_sketcher_run, "d2g_sketcher_run", b, S, regs.data());
            check(ctx, d2g_oph_finalize(regs.data(), n, m, S, sigs.data(), cards.data(), int(o.workers())), "d2g_oph_finalize");
            bool need = false;
            for (size_t i = 0; i < n; ++i) {
                if (std::isnan(cards[i])) cards[i] = 0.;                              // fastxsketchbyseq.cpp:410-414
                need |= cards[i] < 10. * double(S);
            }
            if (need) {                                                               // lines 415-430: exact distinct count
                ndist.resize(n);
                sk.run(d2g_sketcher_run_distinct, "d2g_sketcher_run_distinct", b, ndist.data());
                for (size_t i = 0; i < n; ++i) if (cards[i] < 10. * double(S)) cards[i] = double(ndist[i]);
            }
        }
        std::memcpy(&res.signatures[g0 * S], sigs.data(), n * S * sizeof(double));
        std::memcpy(&res.cardinalities[g0], cards.data(), n * sizeof(double));
        g0 = g1;
    }
    d2g_seqpack_destroy(sp);
    write_stacked(res, o);
}

// --parse-by-seq --edit-distance --compute-edit-distance: the reference keeps every record's bytes (sequences_, fastxsketchbyseq.cpp:243-246),
// OrderMinHash-sketches them (:296-312; not built) and compare() calls edlib on the bytes (cmp_core.cpp:450-457).  Here the
// records are read by the walker of sketch_core_byseq in its raw form (d2g_seqrecs: the same names and boundaries) and go to the device
// as they are; nothing is sketched.  Every refusal that depends on the file comes before a GPU context is asked for.
int edit_distance_job(const Options &o) {
    if (o.paths.size() != 1)
        die("parse-by-seq currently only handles one file at a time. To process multiple files, simply concatenate them into one file, and run dashing2 on that.");
    const double t0 = now();
    d2g_seqrecs *sr = nullptr;
    check(nullptr, d2g_seqrecs_create(&sr), "d2g_seqrecs_create");
    if (d2g_seqrecs_add_path(sr, o.paths[0].c_str()) != D2G_OK) die("Failed to read from " + o.paths[0]);
    const size_t N = d2g_seqrecs_nrecords(sr);
    const uint64_t *off = d2g_seqrecs_off(sr);
    Result res;
    res.names.resize(N);
    for (size_t i = 0; i < N; ++i) res.names[i] = d2g_seqrecs_name(sr, i);
    for (size_t i = 0; i < N; ++i)
        if (off[i + 1] == off[i]) {                                                  // fastxsketchbyseq.cpp:302-305
            std::fprintf(stderr, "EMPTY SEQ at idx %zu for %s in path %s\n", i, res.names[i].c_str(), o.paths[0].c_str());
            std::exit(1);
        }
    for (size_t i = 0; i < N; ++i)
        if (off[i + 1] - off[i] > D2G_EDIT_MAX_LEN)
            refuse_out_of_scope("record " + res.names[i] + " of " + std::to_string(off[i + 1] - off[i]) + " symbols (an edit distance between records of more than " +
                                std::to_string(D2G_EDIT_MAX_LEN) + " symbols, D2G_EDIT_MAX_LEN)");
    char err[200] = "";
    if (d2g_seqset_check(d2g_seqrecs_bytes(sr), off, N, off[N], err, sizeof err) != D2G_OK) die(err);
    const double t_read = now() - t0;
    LazyCtx lctx(o, D2G_WARM_COPY | D2G_WARM_EDIT);
    d2g_ctx *ctx = lctx.get();
    g_stats.nest("context", Json::object().num("create_s", lctx.t_create).num("warmup_s", lctx.t_warm).num("inputs_loaded_s", t_read).raw("switches", context_switches_json(ctx)));
    cmp_core_edit(o, res, ctx, sr, t_read);
    d2g_seqrecs_destroy(sr);
    return 0;
}

// --set / --countdict (fastxsketch.cpp:425-441,462-524): Counter::finalize(vector&, vector&, threshold) per input, on the GPU
// (d2g_sketcher_run_sets: K3's exact counts, sorted on the device), the key file and the count file per input -- always written, with
// or without --cache (:462).  Inputs are parsed by the host parser and go to the device in batches of about 32 MB of packed bases.
// Loaded instead: every path of a --presketched job; with --cache an input whose file set is complete (the count file too under
// --countdict).  A loaded set's cardinality never comes from the key file's header (exact_files.h).
void exact_sets_job(Result &res, const Options &o, LazyCtx &lctx, ExactSets &es) {
    const size_t N = o.paths.size();
    if (!N) die(o.presketched ? "No paths provided to --presketched" : "Can't sketch empty path set");
    const bool weighted = o.exact == 2;
    const ExactNameOpts no{o.k, o.canon, o.seedseed, o.count_threshold, o.outprefix, o.w, d2g_alphabet_name(o.alphabet)};
    es.weighted = weighted;
    es.keys.assign(N, {}); es.counts.assign(N, {});
    res.destination_files.resize(N);
    res.cardinalities.assign(N, 0.);
    if (weighted) res.kmercountfiles.resize(N);
    std::string err;
    std::vector<size_t> todo;
    for (size_t i = 0; i < N; ++i) {
        const std::string kf = o.presketched ? o.paths[i] : exact_key_file(no, o.paths[i]);
        res.destination_files[i] = kf;
        if (weighted) res.kmercountfiles[i] = exact_count_file(kf);
        uint64_t sz = 0;
        const bool complete = exact_file_size(kf, &sz) && (!weighted || exact_file_size(res.kmercountfiles[i], &sz));
        if (o.presketched || (o.cache && complete)) {
            if (!exact_load(kf, weighted, es.keys[i], es.counts[i], res.cardinalities[i], err)) die(err);
        } else todo.push_back(i);
    }
    // names: the input lines (fastxsketch.cpp:625); --presketched: the reference leaves names_ empty, rows print as E<i> (emitrect.cpp:145,176)
    res.names.clear();
    for (size_t i = 0; i < N; ++i) res.names.push_back(o.presketched ? "E" + std::to_string(i) : o.paths[i]);
    size_t nbatches = 0; uint64_t nkeys = 0;
    const double t0 = now();
    if (!todo.empty()) {
        JobFilter filter(o);
        d2g_ctx *ctx = lctx.get();
        JobSketcher sk(ctx, o, filter);
        const size_t limit = group_bytes_limit(size_t(32) << 20);
        d2g_seqpack *sp = nullptr;
        check(ctx, d2g_seqpack_create_alphabet(o.k, o.alphabet, &sp), "d2g_seqpack_create");
        std::vector<uint64_t> keys, off, cards;
        std::vector<uint32_t> counts;
        for (size_t t0i = 0; t0i < todo.size();) {
            d2g_seqpack_clear(sp);
            size_t t1 = t0i;
            while (t1 < todo.size() && (t1 == t0i || d2g_seqpack_packed_bytes(sp) < limit)) {
                if (d2g_seqpack_add_path(sp, o.paths[todo[t1]].c_str()) != D2G_OK) die("Failed to open " + o.paths[todo[t1]]);
                ++t1;
            }
            const size_t n = t1 - t0i;
            uint64_t cap = 0;
            for (size_t g = 0; g < n; ++g) cap += d2g_seqpack_nkmers(sp, g);
            keys.resize(std::max<uint64_t>(cap, 1)); off.resize(n + 1); cards.resize(2 * n);
            if (weighted) counts.resize(std::max<uint64_t>(cap, 1));
            sk.run(d2g_sketcher_run_sets, "d2g_sketcher_run_sets", RunStream::of(sp), double(o.count_threshold), keys.data(), weighted ? counts.data() : nullptr,
                   cap, off.data(), cards.data());
            for (size_t g = 0; g < n; ++g) {
                const size_t i = todo[t0i + g], ne = size_t(off[g + 1] - off[g]);
                es.keys[i].assign(keys.begin() + off[g], keys.begin() + off[g + 1]);
                if (weighted) es.counts[i].assign(counts.begin() + off[g], counts.begin() + off[g + 1]);
                res.cardinalities[i] = double(cards[2 * g + (weighted ? 1 : 0)]);   // fastxsketch.cpp:439-441: also the header that is written
                std::fprintf(stderr, "Writing saved sketch to %s\n", res.destination_files[i].c_str());   // :463
                if (!exact_write(res.destination_files[i], res.cardinalities[i], es.keys[i].data(), weighted ? es.counts[i].data() : nullptr, ne, err)) die(err);
                nkeys += ne;
            }
            ++nbatches;
            t0i = t1;
        }
        d2g_seqpack_destroy(sp);
    }
    if (o.verbosity) std::fprintf(stderr, "[d2g] exact k-mer sets: %zu inputs, %zu loaded, %zu computed in %zu batches (%" PRIu64 " keys) in %.3fs\n", N, N - todo.size(), todo.size(),
                                  nbatches, nkeys, now() - t0);
    if (g_stats.on)
        g_stats.nest("sketch", Json::object().integer("inputs", N).integer("sketched", todo.size()).integer("from_cache", N - todo.size()).integer("k", o.k)
                     .str("space", weighted ? "exact count dictionaries (K3 counts + K3s sort)" : "exact k-mer sets (K3 counts + K3s sort)").integer("batches", nbatches)
                     .integer("keys", nkeys).nest("k3", kernel_acc(lctx.get(), "k3").json()).nest("k3s", kernel_acc(lctx.get(), "k3s").json()).num("wall_s", now() - t0));
}

// --bed (sketch_core.cpp:48-62 -> bed2sketch, src/bedsketch.cpp:5-103): one sketch per interval file.  The files are a few MB of text
// that stand for 10^7 - 10^9 positions each: they are read and parsed here, on this thread (d2g_bed_parse: the reference's line rules),
// and every position is sketched on the GPU -- K1i registers finalised like K1's, or with --multiset the sweep's runs expanded and fed to
// BagMinHash (d2g_interval_bmh_sketch).  Names and signatures are both in input order (the reference fills names_ in size-sorted order,
// sketch_core.cpp:58-61: SURVEY F32).
// Cache files: <input>.opss ([f64 card][f64 x S]; .d2gbmh in multiset space, as elsewhere in this build) next to the input or under
// --outprefix, written ALWAYS (bedsketch.cpp:57 writes without --cache too) -- the name carries neither S nor the space's options.
// --cache loads a file of exactly 8 (S + 1) bytes; any other size is sketched again and rewritten (the reference's loader appends to
// an already sized vector and recomputes the cardinality, bedsketch.cpp:26-32: SURVEY F31).
void sketch_core_bed(Result &res, const Options &o, LazyCtx &lctx) {
    const double t_enter = now();
    const size_t N = o.paths.size(), S = o.sketchsize, m = d2g_oph_m(S);
    const bool multiset = o.sspace == SPACE_MULTISET;
    if (!N) die("Can't sketch empty path set");
    res.names = o.paths;
    res.destination_files.resize(N);
    res.cardinalities.assign(N, -1.);
    res.signatures.assign(N * S, 0.);
    std::vector<size_t> todo;
    std::vector<uint64_t> chrhash, start, stop, file_off(1, 0);
    uint64_t nlines = 0;
    std::string buf;
    for (size_t i = 0; i < N; ++i) {
        const std::string &path = o.paths[i];
        res.destination_files[i] = (o.outprefix.empty() ? path : o.outprefix + '/' + trim_folder(path)) + (multiset ? ".d2gbmh" : ".opss");
        if (o.cache && isfile(res.destination_files[i])) {
            if (filesize(res.destination_files[i]) == 8 + 8 * S && load_cached(res.destination_files[i], &res.signatures[i * S], &res.cardinalities[i], S)) continue;
            std::fprintf(stderr, "[d2g] %s does not hold a sketch of size %zu: sketching %s again\n", res.destination_files[i].c_str(), S, path.c_str());
        }
        std::FILE *fp = std::fopen(path.c_str(), "rb");
        if (!fp) die("Failed to open file " + path + " for reading");
        buf.resize(filesize(path));
        const size_t got = buf.empty() ? 0 : std::fread(&buf[0], 1, buf.size(), fp);
        std::fclose(fp);
        buf.resize(got);
        size_t nl = 0;
        char err[600] = "";
        const size_t cap = size_t(std::count(buf.begin(), buf.end(), '\n')) + 1, at = chrhash.size();
        chrhash.resize(at + cap); start.resize(at + cap); stop.resize(at + cap);
        if (d2g_bed_parse(buf.data(), buf.size(), 1, &chrhash[at], &start[at], &stop[at], cap, &nl, err, sizeof err) != D2G_OK)
            die(std::string(err) + " (" + path + ")");                   // "Malformed line: ...", bedsketch.cpp:40
        chrhash.resize(at + nl); start.resize(at + nl); stop.resize(at + nl);
        file_off.push_back(at + nl);
        nlines += nl;
        todo.push_back(i);
    }
    const double t_parse = now();
    uint64_t npositions = 0, nruns = 0;
    if (!todo.empty()) {
        d2g_ctx *ctx = lctx.get();
        const size_t n = todo.size();
        d2g_interval_plan *plan = nullptr;
        check(ctx, d2g_interval_plan_create(ctx, chrhash.data(), start.data(), stop.data(), chrhash.size(), file_off.data(), n, &plan), "d2g_interval_plan_create");
        npositions = d2g_interval_plan_npositions(plan);
        std::vector<double> sigs(n * S), cards(n);
        if (multiset) {
            check(ctx, d2g_interval_bmh_sketch(ctx, plan, o.normalize_intervals, S, sigs.data(), cards.data()), "d2g_interval_bmh_sketch");
            if (g_stats.on) {
                std::vector<uint64_t> roff(n + 1);
                size_t nr = 0;
                (void)d2g_interval_runs(plan, o.normalize_intervals, nullptr, nullptr, nullptr, nullptr, 0, roff.data(), &nr);
                nruns = nr;
            }
        } else {
            std::vector<uint64_t> regs(n * m);
            check(ctx, d2g_interval_oph_sketch(ctx, plan, S, regs.data()), "d2g_interval_oph_sketch");
            check(ctx, d2g_oph_finalize(regs.data(), n, m, S, sigs.data(), cards.data(), int(o.workers())), "d2g_oph_finalize");
        }
        for (size_t t = 0; t < n; ++t) {
            const size_t i = todo[t];
            std::memcpy(&res.signatures[i * S], &sigs[t * S], S * sizeof(double));
            res.cardinalities[i] = cards[t];
            write_cached(res.destination_files[i], &sigs[t * S], cards[t], S);
        }
        if (g_release_at_exit) d2g_interval_plan_destroy(plan);
    }
    if (o.verbosity) std::fprintf(stderr, "[d2g] sketched %zu interval files (%" PRIu64 " lines, %" PRIu64 " positions; %zu from cache): read + parse %.3fs, device %.3fs\n",
                                  todo.size(), nlines, npositions, N - todo.size(), t_parse - t_enter, now() - t_parse);
    if (g_stats.on) {
        Json dev = device_json(o.device);
        for (const char *kernel : {"k1i", "k1iexpand", "k1ibmh"}) dev.nest(kernel, kernel_acc(lctx.get(), kernel).json());
        g_stats.nest("sketch", Json::object().integer("inputs", N).integer("sketched", todo.size()).integer("from_cache", N - todo.size()).integer("sketchsize", S)
                     .str("space", multiset ? "multiset (K1i: interval runs + BagMinHash)" : "set (K1i: OPH over positions)")
                     .nest("intervals", Json::object().integer("lines", nlines).integer("positions", npositions).integer("runs", nruns))
                     .nest("devices", Json::array().push(dev))
                     .nest("wall_s", Json::object().num("read_and_parse", t_parse - t_enter).num("device", now() - t_parse)));
    }
    write_stacked(res, o);
}

int sketch_main(int argc, char **argv) {                          // src/sketch_main.cpp:23-152
    Options o;
    if (int rc = parse_options(argc, argv, o)) return rc - 1;
    apply_fmt_compat(o);
    if (o.paths.empty()) { std::fprintf(stderr, "No paths provided. See usage.\n"); sketch_usage(); return 1; }
    o.device = job_devices(o)[0];
    g_stats.on = !o.gpu_stats.empty(); g_stats.path = o.gpu_stats;
    g_stats.str("command", "sketch");
    if (o.edit) return edit_distance_job(o);
    LazyCtx lctx(o, D2G_WARM_COPY | (o.bed ? D2G_WARM_K1I | (o.sspace == SPACE_MULTISET ? D2G_WARM_K3 : 0) : o.sspace == SPACE_MULTISET || o.count_threshold >= 2 || o.exact ? D2G_WARM_K3 : D2G_WARM_K1) | (o.cmpout.empty() ? 0 : o.exact ? D2G_WARM_KSET : D2G_WARM_K2));
    Result res;
    ExactSets es;
    if (o.exact) exact_sets_job(res, o, lctx, es);
    else if (o.bed) sketch_core_bed(res, o, lctx);
    else if (o.parse_by_seq) sketch_core_byseq(res, o, lctx); else sketch_core(res, o, lctx);
    if (o.verbosity) std::fprintf(stderr, "[d2g] GPU context %.3fs + warm-up %.3fs on a helper thread, under the host ingest\n", lctx.t_create, lctx.t_warm);
    res.nq = o.nq;
    if (!o.cmpout.empty()) { if (o.exact) cmp_core_exact(o, res, lctx.get(), es); else cmp_core(o, res, lctx.get()); }   // sketch_main.cpp:144-148
    g_stats.nest("context", Json::object().num("create_s", lctx.t_create).num("warmup_s", lctx.t_warm).raw("switches", context_switches_json(lctx.get())));
    return 0;
}

}  // namespace d2h
