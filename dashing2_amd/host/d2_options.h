// d2_options.h -- option structs and parsing of the drop-in `dashing2 sketch|cmp` CLI.
// Flag names, defaults and validation mirror the reference: src/options.h:63-171 (SHARED_OPTS),
// :175-304 (VALID_LONG_OPTION_STRINGS / validate_options), :308-449 (SHARED_FIELDS),
// src/sketch_main.cpp:23-152, src/cmp_main.cpp:200-366.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace d2h {

enum OutputKind { SYMMETRIC_ALL_PAIRS, PHYLIP, ASYMMETRIC_ALL_PAIRS, KNN_GRAPH, NN_GRAPH_THRESHOLD, PANEL, DEDUP };  // enums.h:86-94
enum OutputFormat { MACHINE_READABLE, HUMAN_READABLE };                                                             // enums.h:96-100
enum KmerResult { ONE_PERM = 0, FULL_SETSKETCH = 1 };                                                                // enums.h:70-84 (in scope)
enum SketchSpace { SPACE_SET = 0, SPACE_MULTISET = 1, SPACE_PSET = 2 };                                              // enums.h:35-42

struct Options {
    bool is_cmp = false;
    int k = -1, w = -1, nt = -1;
    bool canon = true, cache = false, presketched = false;
    bool save_kmers = false;              // -s/--save-kmers (options.h:347): <out>.kmer64 + <out>.kmer64.names.txt, the masked k-mer behind every OPH register
    bool save_kmercounts = false;         // -N/--save-kmercounts (options.h:346; sets save_kmers too): <out>.kmercounts.f64, how often that k-mer occurred
    bool parse_by_seq = false;            // --parse-by-seq (options.h:378): one sketch per FASTX record of ONE input file
    size_t sketchsize = 1024;
    uint64_t seedseed = 0;
    size_t batch_size = 0;
    unsigned count_threshold = 0;         // -m/--threshold/--count-threshold (d2.h:103): --multiset keeps count > c, set sketches count >= c
    std::string ffile, qfile, outfile, cmpout, outprefix;
    OutputKind ok = SYMMETRIC_ALL_PAIRS;
    OutputFormat of = HUMAN_READABLE;
    int measure = 0;                      // d2g_measure / cmp_main.h:8-17
    KmerResult kmer_result = ONE_PERM;
    SketchSpace sspace = SPACE_SET;
    int verbosity = 0;
    std::vector<std::string> paths;       // references then queries
    size_t nq = 0;                        // number of query paths (-Q)
    int device = 0;                       // D2G_DEVICE env (not a reference flag)
    std::string gpu_stats;                // --gpu-stats FILE (not a reference flag): machine-readable record of the run (SURVEY 5 "Metrics")
    int regbytes = 8;                     // --fastcmp/--regsize/--regbytes <8|4|2|1> (options.h:321-327): below 8 the comparison runs on truncated registers (cmp_core.cpp:209-322)
    bool bbit_sigs = false;               // --bbit-sigs (options.h:101): b-bit truncation instead of the logarithmic (setsketch) one; no effect at 8 bytes
    int topk = -1;                        // cmp --topk/--top-k K (options.h:308): ok = KNN_GRAPH, the K nearest neighbours of every sketch, ties with the K-th kept
    double min_similarity = -1.;          // cmp --similarity-threshold T (options.h:309): ok = NN_GRAPH_THRESHOLD, every pair at T or beyond
    bool greedy = false;                  // cmp --greedy T[E] (options.h:310-318): ok = DEDUP, greedy clustering in input order; always the exhaustive route (the E suffix is accepted, the LSH route is out of scope)
    double greedy_t = 0.;                 // ... its threshold as parsed (printed in the header); <= 0 clusters at the reference's default of 0.9 (dedup_core.cpp:264)
    std::string filterset_arg;            // --filterset <arg> as given (options.h:509-511)
    std::string filterset;                // ... and its sequence path line (d2.cpp:45-49): the k-mers of these FASTX files are skipped by every sketch
    mutable bool filterset_built = false; // the sketching leg has built the filter (it runs on a const Options) ...
    mutable uint64_t filterset_size = 0;  // ... of this many k-mer occurrences: FilterSet::data_.size(), printed by to_string()
    int exact = 0;                        // --set/-H = 1 (FULL_MMER_SET), --countdict/-J = 2 (FULL_MMER_COUNTDICT) (options.h:153,348-349): no sketch, the exact
                                          // k-mer set / count dictionary of every input; kept iff count > count_threshold; cmp gives exact values
    int alphabet = 0;                     // --protein/--protein20/--enable-protein = 2, --protein8 = 3, --protein14 = 4, --protein6 = 5 (options.h:143-148,328-331;
                                          // ids of python/parse.py:8-23 = D2G_ALPHABET_*): amino-acid k-mers (K1a), canon forced off, default k = the alphabet's largest
    uint64_t cssize = 0;                  // -c/--countsketch-size/--countmin-size cells (options.h:78-79,357; d2.h:107): with --multiset the k-mers are counted in a
                                          // single-row count-sketch of that many cells (K3k) instead of exactly; 0 = exact counting.  Elsewhere only to_string() shows it
    bool bed = false;                     // --bed (options.h:149; DataType BED, sketch_core.cpp:48-62): every input is an interval file, a position of a line is an element (K1i)
    bool normalize_intervals = false;     // --normalize-intervals (options.h:150): with --bed --multiset a line adds 1 / (stop - start) to each of its positions
    bool edit_space = false;              // --edit-distance (options.h:134,337): sketch space SPACE_EDIT_DISTANCE
    bool compute_edit = false;            // --compute-edit-distance (options.h:110): measure M_EDIT_DISTANCE
    bool edit = false;                    // both, with --parse-by-seq and a matrix output: exact edit distances between the records of one file (K2h);
                                          // every other use of the two flags is refused by parse_options
    int fmt_compat = 0;                   // --fmt-compat {10,11} (not a reference flag): float text layout of fmt < 11 / >= 11; 0 = not given (10)

    unsigned nthreads() const { return nt < 1 ? 1u : unsigned(nt); }      // as requested (-p / OMP_NUM_THREADS): what is printed
    // threads actually started: the request, cut to the CPUs this process may use (affinity mask, cgroup CPU quota -- a
    // container that shows 256 CPUs and grants 16 makes 112 requested threads throttle each other: 0.70 s instead of 0.36 s
    // for 5 GB of FASTA).  D2G_NO_CPU_CAP=1 keeps the request.
    unsigned workers() const;
    std::string to_string() const;        // Dashing2Options::to_string, src/d2.cpp:10-43
};

// returns 0 to continue, or the process exit code (+1) when parsing decided to stop (usage/errors)
int parse_options(int argc, char **argv, Options &o);
void sketch_usage();
void cmp_usage();

}  // namespace d2h
