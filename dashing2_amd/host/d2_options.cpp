#include "d2_options.h"
#include <sched.h>
#include <cstdio>
#include <fstream>
#include <thread>
#include "../../include/d2g.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <getopt.h>
#include <set>

namespace d2h {

// every --long flag the reference accepts (src/options.h:175-286); anything else is rejected with
// the reference's message (src/options.h:290-304).
static const char *const VALID_LONG[] = {
    "128bit", "BMH", "PMH", "asymmetric", "asymmetric-all-pairs", "bagminhash", "batch-size", "bbit-sigs", "bed",
    "bigwig", "binary", "binary-output", "bmh", "by-chrom", "cache", "cache-sketches", "cmp-outfile", "cmpout",
    "compute-edit-distance", "containment", "count-threshold", "countdict", "countmin-size", "countsketch-size",
    "distance", "distout", "doph", "downsample", "edit-distance", "emit-binary", "enable-protein", "entmin",
    "exact-kmer-dist", "fastcmp", "fastcmp-bytes", "fastcmp-nibbles", "fastcmp-shorts", "fastcmp-words", "ffile",
    "filterset", "full", "full-setsketch", "greedy", "help", "hp-compress", "intersection", "intersection-size",
    "kmer-length", "leafcutter", "long-kmers", "mash-distance", "maxcand", "multiset", "nLSH", "nlsh", "no-canon",
    "normalize-intervals", "one-perm", "oneperm", "oneperm-setsketch", "oph", "outfile", "outprefix", "pairlist",
    "parse-by-seq", "phylip", "pmh", "pminhash", "poisson-distance", "prefix", "prob", "probminhash", "probs",
    "protein", "protein14", "protein20", "protein6", "protein8", "qfile", "refine-exact", "regbytes", "regsize",
    "save-kmercounts", "save-kmers", "seed", "seq", "set", "setsketch-ab", "sig-ram-limit", "similarity-threshold",
    "sketch-size-l2", "sketchsize", "spacing", "square", "symmetric-containment", "threads", "threshold", "top-k",
    "topk", "union-size", "verbose", "window-size", "seqs-in-ram"};

enum {
    OPT_CMPOUT = 1000, OPT_OUTPREF, OPT_BINARY, OPT_PHYLIP, OPT_ASYM, OPT_ISZ, OPT_USZ, OPT_MASH, OPT_SYMCONTAIN,
    OPT_CONTAIN, OPT_SEED, OPT_HELP, OPT_BATCH, OPT_PRESKETCHED, OPT_MULTISET, OPT_PARSEBYSEQ, OPT_FMTCOMPAT, OPT_GPUSTATS, OPT_FASTCMP, OPT_BBITSIGS, OPT_TOPK, OPT_SIMTHRESH, OPT_GREEDY, OPT_FILTERSET, OPT_SET, OPT_PROTEIN, OPT_PROTEIN6, OPT_PROTEIN8, OPT_PROTEIN14, OPT_BED, OPT_NORMIV, OPT_EDITDIST, OPT_COMPUTEEDIT, OPT_UNSUPPORTED
};

void sketch_usage() {
    std::fprintf(stderr, "dashing2 sketch <opts> [fastas... (optional)]\n"
                         "MI355X build: One-Permutation SetSketch (default) or --multiset BagMinHash of k-mers (k <= 32),\n"
                         "optional all-pairs comparison.\n"
                         "  -k/--kmer-length k   -S/--sketchsize S   -L/--sketch-size-l2 l   -p/--threads n\n"
                         "  -w/--window-size w     w > k: only the minimizer of every window of w bases (the k-mer x of its w - k + 1 with the smallest\n"
                         "                         x ^ 0xe37e28c4271b5a2d, once per window position) is sketched, counted or filtered;         \n"
                         "                         w <= k: every k-mer.  Cache and set file names carry .w<w>; at most w - k = 4095\n"
                         "  --protein/--protein20/--enable-protein   amino-acid k-mers over the 20 letters (k <= 14, the default k);\n"
                         "  --protein14 / --protein8 / --protein6    ... over the reduced alphabets SE-B(14) (k <= 16), SE-B(8) (k <= 21), SE-B(6) (k <= 24).\n"
                         "                         No canonical form (as -C); any other letter ends a run as N does; file names carry PROTEIN20 /\n"
                         "                         PROTEIN_14 / PROTEIN_3BIT / PROTEIN_6 where DNA stands.  Not with -w > k, k above the limit, several GPUs\n"
                         "  --bed                  every input is an interval file (BED: chrom<TAB>start<TAB>stop...): the element of a sketch is a genomic\n"
                         "                         position, XXH3_64bits(chrom, a leading chr/Chr dropped) ^ i for start <= i < stop, sketched on the GPU (K1i).\n"
                         "                         With --multiset a position weighs the number of lines that cover it; --normalize-intervals: each line\n"
                         "                         adds 1 / (stop - start) instead.  <input>.opss (.d2gbmh with --multiset) is always written, --cache loads it.\n"
                         "                         -k, -w, -C and -m play no part.  Not with --parse-by-seq, -s/-N, --set/--countdict, --filterset, -c, the\n"
                         "                         protein alphabets, several GPUs, gzip-compressed input; --bigwig, --leafcutter, --by-chrom: not built\n"
                         "  -F/--ffile paths.txt -Q/--qfile queries.txt  -o/--outfile stacked.bin\n"
                         "  --cmpout/--distout/--cmp-outfile out   --phylip   --binary-output   --asymmetric-all-pairs\n"
                         "  --no-canon/-C  --seed s  --cache/-W  --outprefix dir  --oph/-Z\n"
                         "  --multiset/--bagminhash/-B   --parse-by-seq (one sketch per record of ONE file)\n"
                         "  -c/--countsketch-size/--countmin-size cells   with --multiset: count the k-mers in a single-row count-sketch of that many cells\n"
                         "                         (weighted sketching with fixed memory usage at the expense of some approximation: 4 bytes per cell and input,\n"
                         "                         whatever the input's length) instead of exactly; a cell is kept when |count| >= -m c; cache names carry\n"
                         "                         .CountMinCounting<cells>; 0: exact counting.  Not with --set/--countdict, --parse-by-seq, several GPUs, cells > 2^31\n"
                         "  -m/--count-threshold c   set sketches (OPH) of whole inputs: only k-mers seen at least c times are sketched (c < 2: all);\n"
                         "                         with --multiset: only k-mers seen MORE than c times.  In set space not with --parse-by-seq or\n"
                         "                         --presketched, and only where the sketches are written (-o, --cache or --cmpout)\n"
                         "  -s/--save-kmers        with -o out: out.kmer64 (24-byte header, then per input the masked k-mer behind each of its S\n"
                         "                         registers) and out.kmer64.names.txt; set sketches (OPH) only, not with --parse-by-seq\n"
                         "  -N/--save-kmercounts   -s, and out.kmercounts.f64: how often each of those k-mers occurred in its input (float32)\n"
                         "  --filterset <paths>    skip every k-mer of these FASTA/FASTQ(.gz) files (several paths: one argument, space-separated) in all\n"
                         "                         inputs, before anything is sketched or counted: adapters, phiX, rRNA, a host genome.  Same -k and\n"
                         "                         canonicalisation as the sketch; `<paths>:K` is accepted as the reference accepts it; binary k-mer files not\n"
                         "  --set/-H               no sketch: the exact set of distinct k-mers of every input, sorted on the GPU.  Writes, per input,\n"
                         "                         <input>[.seed<s>][.rc_canon].k<k>[.ct_threshold<c>].FullMmerSet.DNA.kmerset64 ([f64 card][u64 keys]) next to it or\n"
                         "                         under --outprefix; --cmpout / cmp give the EXACT Jaccard, containment, intersection, ... of every pair\n"
                         "  --countdict/-J         the same with every k-mer's count (<...>.kmercounts.f64): exact weighted Jaccard, sum of min counts.\n"
                         "                         -m c keeps the k-mers seen MORE than c times.  Not with -o, --multiset, --parse-by-seq, -s/-N, --fastcmp <8,\n"
                         "                         --topk, --similarity-threshold, --greedy, several GPUs; cmp --presketched *.kmerset64 is --set\n"
                         "  --edit-distance --compute-edit-distance   with --parse-by-seq: the EXACT edit distance (unit-cost Levenshtein over the raw bytes:\n"
                         "                         no case folding, N a symbol like any other, qualities ignored) between every two records of ONE\n"
                         "                         FASTA/FASTQ(.gz) file, computed on the GPU (K2h); --cmpout / cmp give the triangle, --square, --phylip or\n"
                         "                         --binary-output.  Both flags are needed: --edit-distance alone is the OrderMinHash LSH similarity, which is\n"
                         "                         not built.  Records of at most 65535 symbols.  -k, -w, -S, -C and the protein flags play no part.  Not with\n"
                         "                         -o, --cache, --presketched, -Q, --topk, --similarity-threshold, --greedy, --multiset, --set/--countdict,\n"
                         "                         -s/-N, -m, -c, --filterset, --bed, --fastcmp <8, another measure, several GPUs\n"
                         "  --distance/--mash-distance --containment --symmetric-containment --intersection --union-size\n"
                         "  --fastcmp/--regsize/--regbytes <8|4|2|1>   compare registers truncated to that many bytes (8: as sketched); logarithmic\n"
                         "                         (setsketch) truncation unless --bbit-sigs selects b-bit signatures\n"
                         "  --batch-size n  -v\n"
                         "  --fmt-compat {10,11}   float text of PHYLIP/TSV output as fmt < 11 (default: fixed notation below 1e16) or\n"
                         "                         fmt >= 11 (exponent form from 1e7) prints it -- the reference's fmt is an unpinned submodule\n"
                         "  --gpu-stats file.json  one JSON object per run: device(s), kernel milliseconds, bit-plane counts, algorithmic bytes, wall phases\n"
                         "  D2G_DEVICES=all|0,1,..  spread `sketch` (inputs dealt to the GPUs) and `cmp` (rows of the matrix) over several GPUs\n");
}
void cmp_usage() {
    std::fprintf(stderr, "dashing2 cmp <opts> [fastas... (optional)]\n"
                         "--presketched\t To compute distances using a pre-sketched method (e.g., dashing2 sketch -o path), "
                         "use this flag and pass in a single positional argument.\n"
                         "--topk/--top-k K\t Nearest neighbours instead of a matrix: for every sketch its K best (all ties with the K-th best are kept;\n"
                         "\t\t a similarity of 0 is never a neighbour), best first, selected on the GPU -- always exhaustive (the reference's EXACT_KNN=1).\n"
                         "--similarity-threshold T\t ... or every pair whose similarity is at least T (with --mash-distance: whose distance is at most T).\n"
                         "\t\t Output: one line per sketch `name<TAB>neighbour:value...`, or with --binary-output CSR: u64 nids, u64 nnz,\n"
                         "\t\t u64 indptr[nids+1], u32 indices[nnz], f32 data[nnz].  Similarity and --mash-distance, full 8-byte registers, one GPU;\n"
                         "\t\t not with -Q, --square, --phylip, --fastcmp <4|2|1>.\n"
                         "--greedy T[E]\t Greedy clustering (dereplication) instead of a matrix: in input order, a sketch joins the cluster whose\n"
                         "\t\t representative is most similar to it if that similarity is at least T (T <= 0: 0.9), else it founds a cluster; it is\n"
                         "\t\t compared with representatives only.  Clustered on the GPU, always exhaustively (with or without the E suffix).\n"
                         "\t\t Output: `Cluster-c<TAB>name:id...` per cluster, representative first, or with --binary-output u64 nclusters, u64 nnz,\n"
                         "\t\t u64 indptr[nclusters+1], u32 ids[nnz].  Similarity only, full 8-byte registers, one GPU; not with the F suffix, -Q,\n"
                         "\t\t --square, --phylip, --topk, --similarity-threshold, --fastcmp <4|2|1>.\n");
    sketch_usage();
}

static bool validate_long_flags(char **argv, bool is_cmp) {
    for (char **p = argv; *p; ++p) {
        const size_t len = std::strlen(*p);
        if (len > 2 && std::memcmp(*p, "--", 2) == 0) {
            const std::string flag(*p + 2);
            if (is_cmp && flag == "presketched") continue;
            if (flag == "fmt-compat") continue;              // this build's own flag (float text generation of the fmt library)
            if (flag == "gpu-stats") continue;               // this build's own flag (machine-readable per-run record)
            bool ok = false;
            for (const char *v : VALID_LONG) if (flag == v) { ok = true; break; }
            if (!ok) {   // src/options.h:298-301
                std::fprintf(stderr, "flag %s not found in expected set. See usage.\n", flag.c_str());
                std::fprintf(stderr, "Exception Flag %s not found\n", flag.c_str());
                return false;
            }
        }
    }
    return true;
}

std::string Options::to_string() const {    // src/d2.cpp:10-43 (fields that exist in this scope)
    char buf[4096];
    int pos = std::snprintf(buf, sizeof buf, "Dashing2Options;k:%d", k);
    if (w > 0) pos += std::snprintf(buf + pos, sizeof buf - pos, ";w:%d", w);
    pos += std::snprintf(buf + pos, sizeof buf - pos, ";%s", parse_by_seq ? "parsebyseq" : "parsebyfile");
    pos += std::snprintf(buf + pos, sizeof buf - pos, ";trimchr");
    pos += std::snprintf(buf + pos, sizeof buf - pos, ";sketchsize:%zu", sketchsize);
    if (count_threshold > 0) pos += std::snprintf(buf + pos, sizeof buf - pos, ";%u", count_threshold);
    pos += std::snprintf(buf + pos, sizeof buf - pos, ";sketchtype:%s",
                         exact ? (exact == 2 ? "mmerset64,kmercountsf64" : "mmerset64")     // d2.cpp:24,26
                         : edit ? "orderminhash"                                             // d2.cpp:22, SPACE_EDIT_DISTANCE
                         : kmer_result == ONE_PERM ? "onepermsetsketch"
                         : (sspace == SPACE_SET ? "fullsetsketch" : sspace == SPACE_MULTISET ? "bagminhash" : "probminhash"));
    pos += std::snprintf(buf + pos, sizeof buf - pos, ";%s", bed ? "BED" : "Fastx");                 // to_string(dtype_), d2.cpp:28
    if (!outprefix.empty()) pos += std::snprintf(buf + pos, sizeof buf - pos, ";outprefix:%s", outprefix.c_str());
    if (cssize) pos += std::snprintf(buf + pos, sizeof buf - pos, ";counting=countsketch%zu\n", size_t(cssize));   // d2.cpp:33, with its line feed
    if (canon) pos += std::snprintf(buf + pos, sizeof buf - pos, ";canon");
    if (filterset_built) pos += std::snprintf(buf + pos, sizeof buf - pos, ";FilterSetSortedHashSet-size=%llu", (unsigned long long)filterset_size);   // d2.cpp:38-40, filterset.h:82
    return std::string(buf, pos);
}

int parse_options(int argc, char **argv, Options &o) {
    if (!validate_long_flags(argv, o.is_cmp)) return 1 + 1;
    if (o.is_cmp) o.w = 0;                                    // src/cmp_main.cpp:202
    static const struct option longopts[] = {
        {"ffile", required_argument, 0, 'F'}, {"qfile", required_argument, 0, 'Q'}, {"threads", required_argument, 0, 'p'},
        {"sketchsize", required_argument, 0, 'S'}, {"cmpout", required_argument, 0, OPT_CMPOUT},
        {"distout", required_argument, 0, OPT_CMPOUT}, {"cmp-outfile", required_argument, 0, OPT_CMPOUT},
        {"outprefix", required_argument, 0, OPT_OUTPREF}, {"prefix", required_argument, 0, OPT_OUTPREF},
        {"kmer-length", required_argument, 0, 'k'}, {"outfile", required_argument, 0, 'o'},
        {"window-size", required_argument, 0, 'w'},
        {"countsketch-size", required_argument, 0, 'c'}, {"countmin-size", required_argument, 0, 'c'},
        {"binary-output", no_argument, 0, OPT_BINARY}, {"emit-binary", no_argument, 0, OPT_BINARY}, {"binary", no_argument, 0, OPT_BINARY},
        {"intersection", no_argument, 0, OPT_ISZ}, {"intersection-size", no_argument, 0, OPT_ISZ}, {"union-size", no_argument, 0, OPT_USZ},
        {"mash-distance", no_argument, 0, OPT_MASH}, {"distance", no_argument, 0, OPT_MASH}, {"poisson-distance", no_argument, 0, OPT_MASH},
        {"symmetric-containment", no_argument, 0, OPT_SYMCONTAIN}, {"containment", no_argument, 0, OPT_CONTAIN},
        {"phylip", no_argument, 0, OPT_PHYLIP},
        {"asymmetric-all-pairs", no_argument, 0, OPT_ASYM}, {"asymmetric", no_argument, 0, OPT_ASYM}, {"square", no_argument, 0, OPT_ASYM},
        {"oneperm-setsketch", no_argument, 0, 'Z'}, {"oneperm", no_argument, 0, 'Z'}, {"one-perm", no_argument, 0, 'Z'},
        {"oph", no_argument, 0, 'Z'}, {"doph", no_argument, 0, 'Z'},
        {"cache", no_argument, 0, 'W'}, {"cache-sketches", no_argument, 0, 'W'}, {"no-canon", no_argument, 0, 'C'},
        {"seed", required_argument, 0, OPT_SEED}, {"help", no_argument, 0, OPT_HELP},
        {"batch-size", required_argument, 0, OPT_BATCH}, {"sketch-size-l2", required_argument, 0, 'L'},
        {"verbose", no_argument, 0, 'v'}, {"presketched", no_argument, 0, OPT_PRESKETCHED},
        {"multiset", no_argument, 0, OPT_MULTISET}, {"bagminhash", no_argument, 0, OPT_MULTISET}, {"bmh", no_argument, 0, OPT_MULTISET},
        {"BMH", no_argument, 0, OPT_MULTISET},
        {"count-threshold", required_argument, 0, 'm'}, {"threshold", required_argument, 0, 'm'},
        {"parse-by-seq", no_argument, 0, OPT_PARSEBYSEQ},
        {"fmt-compat", required_argument, 0, OPT_FMTCOMPAT},
        {"gpu-stats", required_argument, 0, OPT_GPUSTATS},
        {"fastcmp", required_argument, 0, OPT_FASTCMP}, {"regsize", required_argument, 0, OPT_FASTCMP}, {"regbytes", required_argument, 0, OPT_FASTCMP},
        {"bbit-sigs", no_argument, 0, OPT_BBITSIGS},
        {"save-kmers", no_argument, 0, 's'}, {"save-kmercounts", no_argument, 0, 'N'},
        {"filterset", required_argument, 0, OPT_FILTERSET},
        {"set", no_argument, 0, OPT_SET}, {"countdict", no_argument, 0, 'J'},
        {"protein", no_argument, 0, OPT_PROTEIN}, {"protein20", no_argument, 0, OPT_PROTEIN}, {"enable-protein", no_argument, 0, OPT_PROTEIN},
        {"bed", no_argument, 0, OPT_BED}, {"normalize-intervals", no_argument, 0, OPT_NORMIV},
        {"edit-distance", no_argument, 0, OPT_EDITDIST}, {"compute-edit-distance", no_argument, 0, OPT_COMPUTEEDIT},
        {"protein6", no_argument, 0, OPT_PROTEIN6}, {"protein8", no_argument, 0, OPT_PROTEIN8}, {"protein14", no_argument, 0, OPT_PROTEIN14},
        {0, 0, 0, 0}};
    // every other valid reference flag is recognised but outside the hot-path scope
    std::vector<struct option> all(longopts, longopts + sizeof(longopts) / sizeof(longopts[0]) - 1);
    if (o.is_cmp) {                                           // sparse outputs (options.h:73-75): `cmp` only in this build
        all.push_back({"topk", required_argument, 0, OPT_TOPK});
        all.push_back({"top-k", required_argument, 0, OPT_TOPK});
        all.push_back({"similarity-threshold", required_argument, 0, OPT_SIMTHRESH});
        all.push_back({"greedy", required_argument, 0, OPT_GREEDY});
    }
    int nmeasure = 0;                                         // measure flags other than --compute-edit-distance
    bool saw_square = false, saw_phylip = false, gave_topk = false, gave_thresh = false, greedy_fasta = false, gave_set = false, gave_countdict = false;
    std::set<std::string> have;
    for (auto &x : all) have.insert(x.name);
    static const std::set<std::string> with_arg = {"topk", "top-k", "similarity-threshold", "fastcmp", "regsize", "regbytes",
        "countsketch-size", "countmin-size", "count-threshold", "threshold", "downsample", "spacing", "filterset", "greedy",
        "nlsh", "nLSH", "sig-ram-limit", "maxcand", "setsketch-ab", "pairlist"};
    for (const char *v : VALID_LONG)
        if (!have.count(v)) all.push_back({v, with_arg.count(v) ? required_argument : no_argument, 0, OPT_UNSUPPORTED});
    all.push_back({0, 0, 0, 0});
    int c, idx = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "m:p:k:w:c:f:S:F:Q:o:L:CNs2BPWh?ZJGHv", all.data(), &idx)) >= 0) {
        switch (c) {
            case 'F': o.ffile = optarg; break;
            case 'Q': o.qfile = optarg; o.ok = PANEL; break;
            case 'p': o.nt = std::atoi(optarg); break;
            case 'S': o.sketchsize = size_t(std::atoi(optarg)); break;
            case 'k': o.k = std::atoi(optarg); break;
            case 'w': o.w = std::atoi(optarg); break;
            case 'c': o.cssize = std::strtoull(optarg, nullptr, 10); break;          // options.h:357
            case 'o': o.outfile = optarg; break;
            case 'C': o.canon = false; break;
            case 'W': o.cache = true; break;
            case 's': o.save_kmers = true; break;                                  // options.h:347
            case 'N': o.save_kmers = o.save_kmercounts = true; break;              // options.h:346
            case 'Z': o.kmer_result = ONE_PERM; break;
            case 'v': ++o.verbosity; break;
            case 'L': {
                const int l = std::atoi(optarg);
                if (l <= 0 || l >= 64) { std::fprintf(stderr, "Error: ssl2 is out of bounds. ssl2: %d.\n", l); return 1 + 1; }
                o.sketchsize = size_t(1) << l;
                std::fprintf(stderr, "Using log_2 sketchsize = %d, yielding sketchsize = %zu\n", l, o.sketchsize);
            } break;
            case OPT_CMPOUT: o.cmpout = optarg; break;
            case OPT_OUTPREF: o.outprefix = optarg; break;
            case OPT_BINARY: o.of = MACHINE_READABLE; break;
            case OPT_PHYLIP: o.ok = PHYLIP; saw_phylip = true; break;
            case OPT_ASYM: o.ok = ASYMMETRIC_ALL_PAIRS; saw_square = true; break;
            case OPT_ISZ: ++nmeasure; o.measure = D2G_INTERSECTION; break;
            case OPT_USZ: ++nmeasure; o.measure = D2G_UNION_SIZE; break;
            case OPT_MASH: ++nmeasure; o.measure = D2G_POISSON_LLR; break;
            case OPT_SYMCONTAIN: ++nmeasure; o.measure = D2G_SYMMETRIC_CONTAINMENT; break;
            case OPT_CONTAIN: ++nmeasure; o.measure = D2G_CONTAINMENT; break;
            case OPT_SEED: o.seedseed = std::strtoull(optarg, 0, 10); break;
            case OPT_BATCH: o.batch_size = std::strtoull(optarg, 0, 10); break;
            case OPT_PRESKETCHED: o.presketched = true; break;
            case OPT_MULTISET: case 'B': o.sspace = SPACE_MULTISET; break;         // options.h:111
            case 'm': o.count_threshold = unsigned(std::atoi(optarg)); break;      // options.h:352
            case OPT_PARSEBYSEQ: o.parse_by_seq = true; break;                     // options.h:378
            case OPT_FMTCOMPAT:
                o.fmt_compat = std::atoi(optarg);
                if (o.fmt_compat != 10 && o.fmt_compat != 11) {
                    std::fprintf(stderr, "dashing2 (MI355X): --fmt-compat takes 10 (float text of fmt < 11, default) or 11 (fmt >= 11)\n");
                    return 1 + 1;
                }
                break;
            case OPT_GPUSTATS: o.gpu_stats = optarg; break;
            case OPT_FASTCMP: {                                                     // options.h:321-327
                const double nb = std::atof(optarg);
                if (nb != 8. && nb != 4. && nb != 2. && nb != 1.) {
                    std::fprintf(stderr, "--fastcmp must have 8, 4, 2, or 1 as the argument. These are the only register sizes supported.\n");
                    std::fprintf(stderr, "Exception See usage for --fastcmp instructions.\n");
                    return 1 + 1;
                }
                o.regbytes = int(nb);
            } break;
            case OPT_TOPK: o.topk = std::atoi(optarg); gave_topk = true; break;                             // options.h:308
            case OPT_SIMTHRESH: o.min_similarity = std::atof(optarg); gave_thresh = true; break;       // options.h:309
            case OPT_GREEDY: {                                                      // options.h:310-318
                char *eptr;
                o.greedy = true; o.greedy_t = std::strtod(optarg, &eptr);
                for (; *eptr; ++eptr) if ((*eptr | 32) == 'f') greedy_fasta = true;    // 'e' (exhaustive): the only route here
            } break;
            case OPT_SET: case 'H': gave_set = true; break;                          // options.h:348
            case 'J': gave_countdict = true; break;                                 // options.h:349
            case OPT_FILTERSET: o.filterset_arg = optarg; break;                    // options.h:509-511
            // PROT_FIELD, options.h:328-331: the alphabet, canon = false, the reference's one stderr line
            case OPT_PROTEIN: o.alphabet = D2G_ALPHABET_PROTEIN20; std::fprintf(stderr, "Parsing 20-character amino acid sequences\n"); break;
            case OPT_PROTEIN6: o.alphabet = D2G_ALPHABET_PROTEIN_6; std::fprintf(stderr, "Parsing amino acid sequences with 6-letter compressed alphabet.\n"); break;
            case OPT_PROTEIN14: o.alphabet = D2G_ALPHABET_PROTEIN_14; std::fprintf(stderr, "Parsing amino acid sequences with 14-letter compressed alphabet.\n"); break;
            case OPT_PROTEIN8: o.alphabet = D2G_ALPHABET_PROTEIN_3BIT; std::fprintf(stderr, "Using 3-bit protein encoding\n"); break;
            case OPT_EDITDIST: o.edit_space = true; break;                          // options.h:134,337: sketch space SPACE_EDIT_DISTANCE
            case OPT_COMPUTEEDIT: o.compute_edit = true; break;                     // options.h:110: measure M_EDIT_DISTANCE
            case OPT_BED: o.bed = true; break;                                      // options.h:149
            case OPT_NORMIV: o.normalize_intervals = true; break;                   // options.h:150
            case OPT_BBITSIGS: o.bbit_sigs = true; break;                           // options.h:101
            case OPT_HELP: case 'h': case '?': o.is_cmp ? cmp_usage() : sketch_usage(); return 1 + 1;
            case OPT_UNSUPPORTED:
                std::fprintf(stderr, "dashing2 (MI355X): option --%s is outside the hot-path scope of this build "
                                     "(OPH sketching + dense all-pairs comparison).\n", all[idx].name);
                return 1 + 1;
            default:
                std::fprintf(stderr, "dashing2 (MI355X): option -%c is outside the hot-path scope of this build.\n", c);
                return 1 + 1;
        }
    }
    if (o.alphabet) o.canon = false;                           // whatever else was given (options.h:328-331; d2.cpp:100-102)
    if (o.k < 0) o.k = o.alphabet ? d2g_alphabet_max_k(o.alphabet) : 32;   // nregperitem(rht): sketch_main.cpp:70, options.h:474
    if (o.nt < 0) {                                            // sketch_main.cpp:71-74
        if (const char *s = std::getenv("OMP_NUM_THREADS")) o.nt = std::max(std::atoi(s), 1);
    }
    if (o.nt < 1) o.nt = 1;
    if (const char *d = std::getenv("D2G_DEVICE")) o.device = std::atoi(d);
    for (int i = optind; i < argc; ++i) o.paths.push_back(argv[i]);
    if (!o.ffile.empty()) {
        std::ifstream ifs(o.ffile);
        if (!ifs) { std::fprintf(stderr, "Exception No path found at %s\n", o.ffile.c_str()); return 1 + 1; }
        for (std::string l; std::getline(ifs, l);) o.paths.push_back(l);
    }
    const size_t nref = o.paths.size();
    if (!o.qfile.empty()) {
        std::ifstream ifs(o.qfile);
        for (std::string l; std::getline(ifs, l);) o.paths.push_back(l);
    }
    o.nq = o.paths.size() - nref;
    if (o.edit_space || o.compute_edit) {
        // K2h: the one edit-distance job this build runs is --parse-by-seq --edit-distance --compute-edit-distance with a matrix as its
        // output; everything else that names these flags is refused here, each by name, before a GPU is asked for
        const char *why = nullptr;
        const char *e = std::getenv("D2G_DEVICES");
        const char *const mode = o.edit_space ? "--edit-distance" : "--compute-edit-distance";
        if (!o.edit_space) why = "no --edit-distance (the measure is defined in the edit-distance space only)";
        else if (!o.parse_by_seq) why = "no --parse-by-seq (the reference throws there, fastxsketch.cpp:215-220,273: an edit distance is between records)";
        else if (!o.compute_edit) why = "no --compute-edit-distance (that is the OrderMinHash LSH similarity; the OrderMinHash sketch is absent from the reference's tree)";
        else if (!o.outfile.empty()) why = "-o/--outfile (the stacked file would hold OrderMinHash registers, which are not built)";
        else if (o.cache) why = "--cache (there are no sketches to cache)";
        else if (o.presketched) why = "--presketched (a sketch file holds no records)";
        else if (!o.is_cmp && o.cmpout.empty()) why = "a sketch job without --cmpout (nothing would be written: there are no OrderMinHash sketches)";
        else if (!o.qfile.empty()) why = "-Q/--qfile (a query panel)";
        else if (gave_topk || gave_thresh) why = "--topk / --similarity-threshold (nearest neighbours by edit distance)";
        else if (o.greedy) why = "--greedy (greedy clustering by edit distance)";
        else if (o.sspace != SPACE_SET) why = "--multiset (another sketch space)";
        else if (gave_set || gave_countdict) why = "--set/-H or --countdict/-J (exact k-mer sets; an edit distance has no k-mers)";
        else if (o.save_kmers) why = "-s/--save-kmers or -N/--save-kmercounts (there are no k-mers behind an edit distance)";
        else if (o.count_threshold > 0) why = "-m/--count-threshold (there are no k-mers to count)";
        else if (o.cssize) why = "-c/--countsketch-size/--countmin-size (there are no k-mers to count)";
        else if (!o.filterset_arg.empty()) why = "--filterset (a k-mer filter; an edit distance has no k-mers)";
        else if (o.bed) why = "--bed (an interval file has no records)";
        else if (o.regbytes < 8) why = "--fastcmp/--regsize/--regbytes below 8 (there are no registers to truncate)";
        else if (nmeasure) why = "a second measure flag (--compute-edit-distance is the measure)";
        else if (e && *e && (std::strcmp(e, "all") == 0 || std::strchr(e, ','))) why = "D2G_DEVICES naming several GPUs (edit distances are computed on one GPU)";
        if (why) {
            std::fprintf(stderr, "dashing2 (MI355X): %s together with %s is outside the hot-path scope of this build.\n", mode, why);
            return 1 + 1;
        }
        o.edit = true;
        o.kmer_result = FULL_SETSKETCH;                          // sketch_main.cpp:124-127
        if (o.alphabet) std::fprintf(stderr, "[d2g] the protein alphabet plays no part in an edit distance (bytes are bytes); it only shows in the options line\n");
    }
    if (o.bed && !o.presketched) {
        // K1i: what interval inputs do not combine with in this build, each named, before a GPU is asked for (with --presketched
        // nothing is sketched: --bed only shows in the options line)
        const char *why = nullptr;
        const char *e = std::getenv("D2G_DEVICES");
        if (o.parse_by_seq) why = "--parse-by-seq (an interval file has no records)";
        else if (o.save_kmers) why = "-s/--save-kmers or -N/--save-kmercounts (the registers of an interval sketch hold positions, not k-mers)";
        else if (gave_set || gave_countdict) why = "--set/-H or --countdict/-J (exact sets of positions)";
        else if (!o.filterset_arg.empty()) why = "--filterset (a k-mer filter; an interval file has no k-mers)";
        else if (o.cssize) why = "-c/--countsketch-size/--countmin-size (the reference's count-sketch arm for BED feeds signed cells to the sketch, bedsketch.cpp:77)";
        else if (o.alphabet) why = "a protein alphabet (--protein, --protein14/8/6)";
        else if (e && *e && (std::strcmp(e, "all") == 0 || std::strchr(e, ','))) why = "D2G_DEVICES naming several GPUs (interval files are sketched on one GPU)";
        if (why) {
            std::fprintf(stderr, "dashing2 (MI355X): --bed together with %s is outside the hot-path scope of this build.\n", why);
            return 1 + 1;
        }
        if (o.normalize_intervals && o.sspace == SPACE_SET) {                       // bedsketch.cpp:7-8
            std::fprintf(stderr, "Exception Can't normalize BED rows in set space. Use SPACE_MULTISET or SPACE_PSET\n");
            return 1 + 1;
        }
        if (o.count_threshold > 0)
            std::fprintf(stderr, "[d2g] -m/--count-threshold has no effect with --bed (bed2sketch never passes it to the sketch it fills)\n");
        if (std::getenv("D2G_DEVICE_PARSE") && !std::getenv("D2G_HOST_PARSE"))
            std::fprintf(stderr, "[d2g] D2G_DEVICE_PARSE ignored with --bed: the device parser reads FASTA, interval files are parsed on the host\n");
    }
    if (gave_set || gave_countdict) {
        // exact k-mer sets / count dictionaries: what they do not combine with in this build, each named
        o.exact = gave_countdict ? 2 : 1;
        const char *const mode = gave_countdict ? "--countdict/-J" : "--set/-H";
        const char *why = nullptr;
        const char *e = std::getenv("D2G_DEVICES");
        if (gave_set && gave_countdict) why = "--set/-H (one of the two, not both)";
        else if (!o.outfile.empty()) why = "-o/--outfile (the stacked file of an exact job holds bottom-k hashes that only the reference's LSH index reads, and "
                                          "its bottomk() under-runs on inputs with fewer k-mers than the sketch size; the per-input files and --cmpout are the outputs)";
        else if (o.sspace != SPACE_SET) why = "--multiset (a sketch space; an exact job sketches nothing)";
        else if (o.parse_by_seq) why = "--parse-by-seq (the reference throws \"Not yet supported\" there, cmp_core.cpp:630)";
        else if (o.save_kmers) why = "-s/--save-kmers or -N/--save-kmercounts (they save what lies behind sketch registers; an exact job has none)";
        else if (o.regbytes < 8) why = "--fastcmp/--regsize/--regbytes below 8 (there are no registers to truncate)";
        else if (gave_topk || gave_thresh) why = "--topk / --similarity-threshold (the reference routes these through an LSH index over bottom-k hashes)";
        else if (o.greedy) why = "--greedy (the reference routes it through an LSH index over bottom-k hashes)";
        else if (e && *e && (std::strcmp(e, "all") == 0 || std::strchr(e, ','))) why = "D2G_DEVICES naming several GPUs (exact sets are kept and compared on one GPU)";
        if (why) {
            std::fprintf(stderr, "dashing2 (MI355X): %s together with %s is outside the hot-path scope of this build.\n", mode, why);
            return 1 + 1;
        }
    }
    if (o.cssize && !o.presketched) {
        // K3k: what the count-sketch does not combine with in this build, each named, before a GPU is asked for.  With --presketched
        // nothing is counted: -c only shows in the options line.  In set space the reference never builds a Counter for whole inputs.
        const char *why = nullptr;
        const char *e = std::getenv("D2G_DEVICES");
        if (o.exact) why = "--set/-H or --countdict/-J (the reference's finalize(vector&...) arm writes maskfn(cell) keys for a count-sketch; that arm is not built)";
        else if (o.parse_by_seq) why = "--parse-by-seq (a count-sketch table per record)";
        else if (o.cssize > (uint64_t(1) << 31)) why = "more than 2^31 cells (a cell number is a 32-bit index on the device)";
        else if (o.sspace == SPACE_MULTISET && e && *e && (std::strcmp(e, "all") == 0 || std::strchr(e, ',')))
            why = "D2G_DEVICES naming several GPUs (count-sketch multiset sketches are made on one GPU)";
        if (why) {
            std::fprintf(stderr, "dashing2 (MI355X): -c/--countsketch-size/--countmin-size together with %s is outside the hot-path scope of this build.\n", why);
            return 1 + 1;
        }
    }
    if (o.sspace != SPACE_SET && o.kmer_result == ONE_PERM) o.kmer_result = FULL_SETSKETCH;   // sketch_main.cpp:124-127
    if (o.sspace == SPACE_SET && o.count_threshold > 0 && !o.exact && !o.bed) {
        // OPH min-count filtering (oph.h:186-205) is built for One-Permutation set sketches of whole inputs that are WRITTEN somewhere.
        // What the parent refused and this build still does not do stays refused as it was:
        const char *why = nullptr;
        int status = 1;
        if (o.presketched) why = "--presketched (nothing is sketched: the threshold belongs to the sketch job that wrote the file)";
        else if (o.parse_by_seq) {
            // under --parse-by-seq the reference replaces the cardinality of small sketches by the exact distinct count
            // (fastxsketchbyseq.cpp:415-430), which has not been worked through with a min-count
            why = "--parse-by-seq in set space (it is built for sketches of whole inputs)";
            status = 2;                                       // a combination of accepted options, not an option out of scope (those leave with 1)
        } else if (!o.is_cmp && o.outfile.empty() && o.cmpout.empty() && !o.cache)
            why = "a sketch job that writes nothing (no -o, --cache or --cmpout: the counted sketches would be dropped)";
        if (why) {
            std::fprintf(stderr, "dashing2 (MI355X): -m/--count-threshold with set sketches (OPH min-count filtering, oph.h:186-205) together with %s "
                                 "is outside this build's hot-path scope; it is supported with --multiset.\n", why);
            return status + 1;
        }
    }
    if (o.save_kmers && !o.presketched && (o.sspace != SPACE_SET || o.parse_by_seq)) {     // with --presketched nothing is sketched: ignored
        std::fprintf(stderr, "dashing2 (MI355X): %s together with %s is outside the hot-path scope of this build "
                             "(the k-mers and counts behind the registers are saved for One-Permutation set sketches of whole inputs).\n",
                     o.save_kmercounts ? "-N/--save-kmercounts" : "-s/--save-kmers",
                     o.sspace == SPACE_MULTISET ? "--multiset" : o.sspace != SPACE_SET ? "a sketch space other than the set space" : "--parse-by-seq");
        return 1 + 1;
    }
    if (!o.filterset_arg.empty() && !o.presketched) {         // Dashing2Options::filterset, d2.cpp:45-49; with --presketched nothing is sketched: ignored
        const size_t i = o.filterset_arg.find_last_of(':');
        if (i != std::string::npos && (o.filterset_arg[i + 1] & 0xdf) != 'K') {
            // the reference's binary-k-mer-file arm: for plain files it opens an EMPTY path (d2.cpp:61-63), and it wants pre-masked values
            std::fprintf(stderr, "dashing2 (MI355X): --filterset %s (a suffix after the last ':' that does not begin with K: a binary k-mer file) "
                                 "is outside the hot-path scope of this build; give the FASTA/FASTQ file(s) whose k-mers are to be skipped.\n", o.filterset_arg.c_str());
            return 1 + 1;
        }
        o.filterset = o.filterset_arg.substr(0, i);
    }
    if (o.alphabet && !o.presketched && !o.edit) {             // K1a: said here, before a GPU is asked for; the library refuses the first two as well
        const char *e = std::getenv("D2G_DEVICES");
        if (o.k > d2g_alphabet_max_k(o.alphabet)) {
            std::fprintf(stderr, "dashing2 (MI355X): k = %d > %d with %s uses the reference's rolling-hash encoder, as k > 32 does for DNA; "
                                 "it is outside this build's hot-path scope.\n", o.k, d2g_alphabet_max_k(o.alphabet), d2g_alphabet_name(o.alphabet));
            return 1 + 1;
        }
        if (o.w > o.k) {
            std::fprintf(stderr, "dashing2 (MI355X): -w %d > -k %d with %s: windowed minimizers of amino-acid k-mers are outside this build's "
                                 "hot-path scope (the windowed walker is DNA only).\n", o.w, o.k, d2g_alphabet_name(o.alphabet));
            return 1 + 1;
        }
        if (e && *e && (std::strcmp(e, "all") == 0 || std::strchr(e, ','))) {
            std::fprintf(stderr, "dashing2 (MI355X): %s together with D2G_DEVICES naming several GPUs is outside the hot-path scope of this build "
                                 "(amino-acid inputs are sketched on one GPU).\n", d2g_alphabet_name(o.alphabet));
            return 1 + 1;
        }
        if (std::getenv("D2G_DEVICE_PARSE") && !std::getenv("D2G_HOST_PARSE"))
            std::fprintf(stderr, "[d2g] D2G_DEVICE_PARSE ignored with %s: the device parser reads DNA, the host parser runs\n", d2g_alphabet_name(o.alphabet));
    }
    if (o.k > 32 && !o.edit) {
        std::fprintf(stderr, "dashing2 (MI355X): k = %d > 32 uses the reference's rolling-hash encoder "
                             "(fastxsketch.cpp:420), which is outside this build's hot-path scope.\n", o.k);
        return 1 + 1;
    }
    if (!o.edit && o.w > o.k && o.w - o.k + 1 > D2G_WINDOW_MAX_Q) {      // K1w: said here, before a GPU is asked for; the library refuses it too
        std::fprintf(stderr, "dashing2 (MI355X): -w %d with -k %d: a window of more than %d k-mers (w - k > %d) is outside this build's "
                             "hot-path scope.\n", o.w, o.k, D2G_WINDOW_MAX_Q, D2G_WINDOW_MAX_Q - 1);
        return 1 + 1;
    }
    if (o.is_cmp && o.greedy) {
        const char *why = nullptr;
        if (greedy_fasta) why = "--greedy with the F suffix (FASTA output of the representatives' sequences)";
        else if (gave_topk || gave_thresh) why = "--greedy together with --topk / --similarity-threshold";
        else if (!o.qfile.empty()) why = "greedy clustering of a query panel (-Q)";
        else if (saw_square) why = "--greedy together with --square / --asymmetric-all-pairs";
        else if (saw_phylip) why = "--greedy together with --phylip";
        else if (o.regbytes < 8) why = "greedy clustering of truncated registers (--fastcmp <4|2|1>)";
        else if (o.measure == D2G_POISSON_LLR)
            why = "greedy clustering by --mash-distance (with a distance the reference founds a new cluster when the nearest representative is closer than T)";
        else if (o.measure != D2G_SIMILARITY)
            why = "greedy clustering by a cardinality-dependent measure (containment, symmetric containment, intersection, union size): its value is not a function of the equality count";
        else if (!o.presketched && o.sspace == SPACE_SET && (o.sketchsize & (o.sketchsize - 1)) != 0)
            why = "greedy clustering with a sketch size that is not a power of two in set space: its value needs (gt, lt) counts, not the equality count";
        if (why) {
            std::fprintf(stderr, "dashing2 (MI355X): %s is outside the hot-path scope of this build "
                                 "(--greedy T or TE; similarity; 8-byte registers; one matrix).\n", why);
            return 1 + 1;
        }
        o.ok = DEDUP;
    }
    if (o.is_cmp && (gave_topk || gave_thresh)) {
        if (o.topk > 0 && o.min_similarity > 0.) {             // Dashing2DistOptions::validate, cmp_main.h:102-104
            std::fprintf(stderr, "Exception invalid: nn > 0 and minsim > 0. Pick either top-k or minimum similarity. (Can't do both.)\n");
            return 1 + 1;
        }
        const char *why = nullptr;
        if (gave_topk && gave_thresh) why = "--topk and --similarity-threshold together, one of them without a positive argument";
        else if (gave_topk && o.topk < 1) why = "--topk needs K >= 1";
        else if (gave_thresh && !(o.min_similarity > 0.)) why = "--similarity-threshold needs T > 0";
        else if (!o.qfile.empty()) why = "nearest neighbours of a query panel (-Q)";
        else if (saw_square) why = "nearest neighbours together with --square / --asymmetric-all-pairs";
        else if (saw_phylip) why = "nearest neighbours together with --phylip";
        else if (o.regbytes < 8) why = "nearest neighbours of truncated registers (--fastcmp <4|2|1>)";
        else if (o.measure != D2G_SIMILARITY && o.measure != D2G_POISSON_LLR)
            why = "nearest neighbours by a cardinality-dependent measure (containment, symmetric containment, intersection, union size): its value is not a function of the equality count";
        else if (!o.presketched && o.sspace == SPACE_SET && (o.sketchsize & (o.sketchsize - 1)) != 0)
            why = "nearest neighbours with a sketch size that is not a power of two in set space: its value needs (gt, lt) counts, not the equality count";
        if (why) {
            std::fprintf(stderr, "dashing2 (MI355X): %s is outside the hot-path scope of this build "
                                 "(--topk K >= 1 or --similarity-threshold T > 0; similarity or --mash-distance; 8-byte registers; one matrix).\n", why);
            return 1 + 1;
        }
        o.ok = gave_topk ? KNN_GRAPH : NN_GRAPH_THRESHOLD;
    }
    return 0;
}

}  // namespace d2h


namespace d2h {

static unsigned usable_cpus() {
    static const unsigned cached = [] {
        unsigned n = std::max(1u, std::thread::hardware_concurrency());
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) n = std::min(n, unsigned(c)); }
        {   // cgroup v2: "<quota> <period>" or "max <period>"
            std::ifstream f("/sys/fs/cgroup/cpu.max");
            std::string q; long long per = 0;
            if (f >> q >> per && q != "max" && per > 0) {
                const long long quota = std::atoll(q.c_str());
                if (quota > 0) n = std::min(n, unsigned(std::max<long long>(1, (quota + per / 2) / per)));
            }
        }
        {   // cgroup v1
            std::ifstream fq("/sys/fs/cgroup/cpu/cpu.cfs_quota_us"), fp("/sys/fs/cgroup/cpu/cpu.cfs_period_us");
            long long quota = -1, per = 0;
            if (fq >> quota && fp >> per && quota > 0 && per > 0) n = std::min(n, unsigned(std::max<long long>(1, (quota + per / 2) / per)));
        }
        return std::max(1u, n);
    }();
    return cached;
}

unsigned Options::workers() const {
    const unsigned req = nthreads();
    if (const char *e = std::getenv("D2G_NO_CPU_CAP")) if (e[0] == '1') return req;
    return std::min(req, usable_cpus());
}

}  // namespace d2h
