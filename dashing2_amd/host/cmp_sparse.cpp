// cmp_sparse.cpp -- the sparse outputs of `dashing2 cmp`: nearest neighbours (--topk, --similarity-threshold) and greedy
// clustering (--greedy).  Both run on one GPU over a cmp set whose values are a table of the equality count; only the lists come back.
//   emit_neighbors           src/emitnn.cpp:12-52          build_exact_graph   src/index_build.cpp:166-228
//   dedup_emit               src/dedup_core.cpp:400-451    dedup_core          src/dedup_core.cpp:262-283
#include "cli_common.h"
#include "fmtfloat.h"

namespace d2h {

const char *sparse_job_name(const Options &o) {
    return o.ok == KNN_GRAPH || o.ok == NN_GRAPH_THRESHOLD ? "nearest neighbours" : o.ok == DEDUP ? "greedy clustering" : nullptr;
}

// Why a sparse job is outside this build's scope, as far as only the inputs tell (the sketch space and size of --presketched files).
// Flag combinations are refused while the options are parsed (d2_options.cpp).
void refuse_sparse_job_out_of_scope(const char *job, const Options &o, size_t S) {
    if (o.sspace == SPACE_SET && (S & (S - 1)) != 0)
        refuse_out_of_scope(std::string(job) + " with a sketch size that is not a power of two in set space: its value needs (gt, lt) counts, not the equality count");
    if (o.sspace == SPACE_PSET) refuse_out_of_scope(std::string(job) + " of ProbMinHash sketches");
}

namespace {

// the output of a sparse format: --cmpout or stdout, checked once when it is closed
struct SparseOut {
    std::string path;
    std::FILE *fp;
    bool good = true;
    explicit SparseOut(const Options &o) : path((o.cmpout.empty() || o.cmpout.front() == '-') ? "/dev/stdout" : o.cmpout) {
        fp = path == "/dev/stdout" ? stdout : std::fopen(path.c_str(), "wb");
        if (!fp) die("Failed to open file " + path + " for writing");
    }
    void write(const void *p, size_t size, size_t n) { good = good && std::fwrite(p, size, n, fp) == n; }
    // text is written in pieces of 4 MiB: `flush_all` writes what is left
    void text(std::string &t, bool flush_all) {
        if (t.empty() || (!flush_all && t.size() < (size_t(1) << 22))) return;
        write(t.data(), 1, t.size());
        t.clear();
    }
    void close(const char *what) {
        good = good && std::fflush(fp) == 0;
        if (fp != stdout) std::fclose(fp);
        if (!good) die(std::string("Failed to write ") + what + " to " + path);
    }
};

// emit_neighbors, src/emitnn.cpp:12-52: CSR (u64 nids, u64 nnz, u64 indptr[nids+1], u32 indices[nnz], f32 data[nnz]) or one text line
// per sketch.  fmt's "{:0.8g}" of a float is printf's "%.8g" of the same value by fmt's documented semantics (PARITY UNPINNED: the
// reference's fmt submodule is absent).
void emit_neighbors(const Options &o, const Result &res, const std::vector<uint64_t> &indptr, const std::vector<uint32_t> &indices,
                    const std::vector<float> &data) {
    SparseOut out(o);
    const size_t ns = indptr.size() - 1, nnz = indices.size();
    if (o.of == HUMAN_READABLE) {
        std::string text = "#Collection\tNeighbor lists -- name:distance, separated by tabs\n";
        char buf[64];
        for (size_t i = 0; i < ns; ++i) {
            text += res.names[i];
            for (uint64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
                text += '\t'; text += res.names[indices[e]]; text += ':';
                text.append(buf, size_t(std::snprintf(buf, sizeof buf, "%.8g", double(data[e]))));
            }
            text += '\n';
            out.text(text, false);
        }
        out.text(text, true);
    } else {
        const uint64_t dims[2] = {uint64_t(ns), uint64_t(nnz)};
        out.write(dims, 8, 2); out.write(indptr.data(), 8, indptr.size()); out.write(indices.data(), 4, nnz); out.write(data.data(), 4, nnz);
    }
    out.close("neighbor lists");
}

// dedup_emit, src/dedup_core.cpp:400-451 (text and binary forms; the FASTA form is out of scope).  The two doubles of the header are
// fmt's "{}" (format_double; PARITY UNPINNED like the other fmt rows).
void emit_clusters(const Options &o, const Result &res, const std::vector<uint64_t> &indptr, const std::vector<uint32_t> &indices, size_t nclusters) {
    SparseOut out(o);
    const size_t ns = res.names.size();
    if (o.of == HUMAN_READABLE) {
        char avg[64], thr[64];
        avg[format_double(double(ns) / double(nclusters), avg)] = 0;     // 0 items: 0 / 0 = "nan" (fmt prints -nan as "-nan"; x86 gives the negative one)
        thr[format_double(o.greedy_t, thr)] = 0;
        std::string text = "#Clustering " + std::to_string(ns) + " items yielded " + std::to_string(nclusters) + " clusters of average size " + avg +
                           ", separated by minimum similarity " + thr + "\n";
        for (size_t c = 0; c < nclusters; ++c) {
            text += "Cluster-" + std::to_string(c);
            for (uint64_t e = indptr[c]; e < indptr[c + 1]; ++e) { text += '\t'; text += res.names[indices[e]]; text += ':'; text += std::to_string(indices[e]); }
            text += '\n';
            out.text(text, false);
        }
        out.text(text, true);
    } else {
        const uint64_t dims[2] = {uint64_t(nclusters), uint64_t(ns)};    // nnz = every item once
        out.write(dims, 8, 2); out.write(indptr.data(), 8, nclusters + 1); out.write(indices.data(), 4, ns);
    }
    out.close("clusters");
}

d2g_cmp_set *upload_set(const Result &res, d2g_ctx *ctx, size_t S) {
    d2g_cmp_set *set = nullptr;
    check(ctx, d2g_cmp_set_create(ctx, reinterpret_cast<const uint64_t *>(res.sigs()), res.names.size(), S, int(D2G_CMP_AUTO), &set), "d2g_cmp_set_create");
    return set;
}
const char *algo_name(const d2g_cmp_set *set) { return d2g_cmp_set_algo(set) == D2G_CMP_BITSLICE ? "bitslice" : "direct"; }

}  // namespace

// cmp_core.cpp:776-799 with build_exact_graph (index_build.cpp:166-228): the selection runs on the GPU (d2g_cmp_set_knn), only the
// neighbours come back.  Always exhaustive; all ties with the K-th best are kept.
void cmp_core_knn(const Options &o, const Result &res, d2g_ctx *ctx, const std::vector<float> &lut, double t_densify) {
    const size_t ns = res.names.size(), S = o.sketchsize;
    const bool isdist = o.measure == D2G_POISSON_LLR;          // distance(measure), cmp_main.h:44-49, for the two measures in scope
    const bool topk = o.ok == KNN_GRAPH;
    const size_t K = topk ? size_t(o.topk) : 0;
    const double T = topk ? 0. : o.min_similarity;
    const double t0 = now();
    d2g_cmp_set *set = upload_set(res, ctx, S);
    const double t_set = now();
    std::vector<uint64_t> indptr(ns + 1, 0), ip;
    std::vector<uint32_t> indices;
    std::vector<float> data;
    constexpr size_t ROWS = 16384;                             // rows per call: a chunk whose lists outgrow the guess is the only thing run twice
    size_t nnz = 0, reruns = 0;
    for (size_t r0 = 0; r0 < ns; r0 += ROWS) {
        const size_t r1 = std::min(ns, r0 + ROWS), n = r1 - r0;
        size_t room = n * (topk ? 2 * std::min(K, ns) + 16 : 64), need = 0;
        ip.resize(n + 1);
        for (int attempt = 0;; ++attempt) {
            indices.resize(nnz + room); data.resize(nnz + room);
            const int rc = d2g_cmp_set_knn(ctx, set, r0, r1, lut.data(), isdist, K, T, 0, 0, ip.data(), indices.data() + nnz, data.data() + nnz, room, &need);
            if (rc == D2G_ERR_NOMEM && attempt == 0 && need > room) { room = need; ++reruns; continue; }
            check(ctx, rc, "d2g_cmp_set_knn");
            break;
        }
        for (size_t i = 0; i < n; ++i) indptr[r0 + i + 1] = nnz + ip[i + 1];
        nnz += need;
    }
    indices.resize(nnz); data.resize(nnz);
    const double t_sel = now();
    emit_neighbors(o, res, indptr, indices, data);
    const double t_emit = now();
    if (o.verbosity) std::fprintf(stderr, "[d2g] cmp %s: %zu sketches x S=%zu: upload+prepare %.3fs, selection %.3fs (%zu neighbours, %zu chunk(s) run twice), emit %.3fs\n",
                                  topk ? "--topk" : "--similarity-threshold", ns, S, t_set - t0, t_sel - t_set, nnz, reruns, t_emit - t_sel);
    if (g_stats.on) {
        Json dev = device_json(o.device), devs = Json::array();
        dev.raw("k2", kernel_json(ctx, "k2")).raw("knn", kernel_json(ctx, "knn")).raw("k2prep", kernel_json(ctx, "k2prep"));
        g_stats.nest("cmp", Json::object().integer("sketches", ns).integer("sketchsize", S).integer("values", nnz).str("shape", topk ? "topk" : "similarity threshold")
                     .raw("topk", topk ? std::to_string(K) : "null").raw("threshold", topk ? "null" : Json::numstr(T)).str("algo", algo_name(set))
                     .integer("neighbours", nnz).integer("chunks_run_twice", reruns).num("bytes_to_host", 8.0 * double(nnz) + 4.0 * double(ns)).nest("devices", devs.push(dev))
                     .nest("wall_s", Json::object().num("densify_scan", t_densify).num("upload_prepare", t_set - t0).num("count_select_d2h_finish", t_sel - t_set)
                           .num("emit", t_emit - t_sel)));
    }
    if (g_release_at_exit) d2g_cmp_set_destroy(set);
}

// cmp_core.cpp:800-805 with the exhaustive branch of dedup_core (dedup_core.cpp:262-283): clustered on the GPU (d2g_cmp_set_dedup), only
// the representative of every sketch comes back.
void cmp_core_dedup(const Options &o, const Result &res, d2g_ctx *ctx, const std::vector<float> &lut, double t_densify) {
    const size_t ns = res.names.size(), S = o.sketchsize;
    const double t0 = now();
    d2g_cmp_set *set = upload_set(res, ctx, S);
    const double t_set = now();
    std::vector<uint32_t> assign(ns), indices(ns);
    std::vector<uint64_t> indptr(ns + 1, 0);
    check(ctx, d2g_cmp_set_dedup(ctx, set, lut.data(), o.greedy_t, 0, assign.data()), "d2g_cmp_set_dedup");
    size_t nclusters = 0;
    if (d2g_dedup_clusters(assign.data(), ns, indptr.data(), indices.data(), &nclusters) != D2G_OK) die("dashing2 (MI355X): the clustering came back malformed");
    const double t_sel = now();
    emit_clusters(o, res, indptr, indices, nclusters);
    const double t_emit = now();
    if (o.verbosity) std::fprintf(stderr, "[d2g] cmp --greedy: %zu sketches x S=%zu: upload+prepare %.3fs, clustering %.3fs (%zu clusters), emit %.3fs\n",
                                  ns, S, t_set - t0, t_sel - t_set, nclusters, t_emit - t_sel);
    if (g_stats.on) {
        const std::string resolve_json = kernel_json(ctx, "dedup_resolve", false);     // a part of "dedup": read before that one clears both
        Json dev = device_json(o.device), devs = Json::array();
        dev.raw("k2", kernel_json(ctx, "k2")).raw("dedup_resolve", resolve_json).raw("dedup", kernel_json(ctx, "dedup")).raw("k2prep", kernel_json(ctx, "k2prep"));
        g_stats.nest("cmp", Json::object().integer("sketches", ns).integer("sketchsize", S).str("shape", "greedy").num("threshold", o.greedy_t).integer("clusters", nclusters)
                     .str("algo", algo_name(set)).num("bytes_to_host", 4.0 * double(ns)).nest("devices", devs.push(dev))
                     .nest("wall_s", Json::object().num("densify_scan", t_densify).num("upload_prepare", t_set - t0).num("count_cluster_d2h", t_sel - t_set).num("emit", t_emit - t_sel)));
    }
    if (g_release_at_exit) d2g_cmp_set_destroy(set);
}

}  // namespace d2h
