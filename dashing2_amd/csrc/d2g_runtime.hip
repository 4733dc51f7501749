// d2g_runtime.hip -- context, device memory and timing plumbing of libd2g.
#include "d2g_internal.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

// the library's run-time switches (DESIGN.md section 4 lists what each one does).  Host-side switches that need no context
// (D2G_MAX_RUN and D2G_NO_AVX512 in d2g_seqpack.cpp, D2G_RCCL_LIB, D2G_COMM_LOOPBACK) are read where they apply.
static const char *const kTuningNames[] = {
    "D2G_BS_SORT", "D2G_BS_NSPLIT", "D2G_BS_TAGBITS", "D2G_BS_ID16", "D2G_K2_MERGE",
    "D2G_BS_SPARSE", "D2G_BS_SPARSE_MIN_N", "D2G_SP_LINK", "D2G_SP_TILE_FRAC", "D2G_SP_LIST_DIV", "D2G_SP_LONG_LIST", "D2G_SP_LIST_FORM", "D2G_SP_PREDICT", "D2G_SP_REMEMBER", "D2G_SP_EMIT_BIG", "D2G_SP_OLINK", "D2G_SP_RIDE", "D2G_SP_RANK_SHARE",
    "D2G_MGPU_CHUNKS",
    "D2G_K3_COMPACT", "D2G_K3_L1BITS", "D2G_K3_BUCKET_KEYS", "D2G_K3_SUB_KEYS", "D2G_K3_SPLIT_MIN", "D2G_K3_SUBBATCH", "D2G_K3_ROUND_KEYS",
    "D2G_K3_GUESS_SCALE", "D2G_K3_GRID_PER_CU", "D2G_K3_LIGHT", "D2G_K3_GQ_SCALE",
    "D2G_K3S_RANGE_KEYS", "D2G_KSET_SPLIT", "D2G_KSET_PBITS",
    "D2G_CS_TABLE_BYTES", "D2G_CS_LDS_CELLS",
    "D2G_EDIT_STRIP", "D2G_EDIT_TILE", "D2G_EDIT_NEAR_ROUTE", "D2G_EDIT_DEDUP_ROUTE", "D2G_EDIT_DEDUP_REVERSE",
    "D2G_KNN_CHUNK_SLOTS", "D2G_EDIT_KNN_CHUNK_SLOTS", "D2G_INTERVAL_LIST_POSITIONS", "D2G_SCREEN_RESULT_PAIRS", "D2G_EDIT_GRID_MAX", "D2G_EDIT_DEDUP_CHUNK", "D2G_EDIT_DEDUP_MAX_CHUNKS",
};
void d2g_tuning_load(d2g_tuning &t) {
    t.kv.clear();
    for (const char *n : kTuningNames)
        if (const char *v = std::getenv(n)) t.kv.emplace_back(n, v);
}

d2g_k2_tuning d2g_k2_tuning_resolve(const d2g_tuning &t) {
    d2g_k2_tuning v;
    if (const char *e = t.get("D2G_BS_SPARSE")) v.sparse = !(e[0] == '0');
    if (const char *e = t.get("D2G_BS_SPARSE_MIN_N")) v.min_n = (size_t)std::atoll(e);
    if (const char *e = t.get("D2G_SP_LINK")) v.link = std::atoi(e) != 0;
    if (const char *e = t.get("D2G_SP_TILE_FRAC")) { const double f = std::atof(e); if (f > 0 && f <= 1) v.tile_frac = f; }
    if (const char *e = t.get("D2G_SP_OLINK")) v.olink = std::atoi(e) != 0;
    if (const char *e = t.get("D2G_K2_MERGE")) { const int d = std::atoi(e); v.merge = d <= 0 ? 0 : d >= 2 ? 2 : 1; }
    if (const char *e = t.get("D2G_SP_EMIT_BIG")) v.emit_big = std::atoi(e) != 0;
    if (const char *e = t.get("D2G_SP_REMEMBER")) v.remember = std::atoi(e) != 0;
    if (const char *e = t.get("D2G_SP_RIDE")) v.ride = std::atoi(e) & 127;
    if (const char *e = t.get("D2G_SP_RANK_SHARE")) { const int d = std::atoi(e); if (d >= 0 && d <= 35) v.rank_share = d; }
    if (const char *e = t.get("D2G_SP_LONG_LIST")) { const long long d = std::atoll(e); if (d >= 0) v.long_list = (size_t)d; }
    if (const char *e = t.get("D2G_SP_PREDICT")) v.predict = std::atoi(e) != 0;
    if (const char *e = t.get("D2G_SP_LIST_FORM")) { const int d = std::atoi(e); if (d >= 0 && d <= 2) v.list_form = d; }
    if (const char *e = t.get("D2G_SP_LIST_DIV")) { const long d = std::atol(e); if (d >= 1 && d <= (1 << 20)) v.list_div = (size_t)d; }
    if (const char *e = t.get("D2G_BS_SORT")) v.sort = !(e[0] == '0');
    if (const char *e = t.get("D2G_BS_TAGBITS")) { const int d = std::atoi(e); if (d >= 0 && d < 31) v.tagbits_max = d; }
    if (const char *e = t.get("D2G_BS_ID16")) v.id16 = std::atoi(e) != 0;
    if (const char *e = t.get("D2G_BS_NSPLIT")) { const int d = std::atoi(e); if (d == 1 || d == 2 || d == 4) v.nsplit_req = d; }
    return v;
}

d2g_k3_tuning d2g_k3_tuning_resolve(const d2g_tuning &t) {
    d2g_k3_tuning v;
    if (const char *e = t.get("D2G_K3_COMPACT")) v.compact = e[0] == '1';
    if (const char *e = t.get("D2G_K3_LIGHT")) v.light = !(e[0] == '0');
    if (const char *e = t.get("D2G_K3_L1BITS")) { const int d = std::atoi(e); if (d >= 0 && d <= K3_MAXBBITS) v.l1bits = (uint32_t)d; }
    if (const char *e = t.get("D2G_K3_BUCKET_KEYS")) { const long d = std::atol(e); if (d >= 1) v.bucket_keys = (uint64_t)d; }
    if (const char *e = t.get("D2G_K3_SUB_KEYS")) { const long d = std::atol(e); if (d >= 1) v.sub_keys = (uint64_t)d; }
    if (const char *e = t.get("D2G_K3_SPLIT_MIN")) { const long d = std::atol(e); if (d >= 1) v.split_min = (uint64_t)d; }
    if (const char *e = t.get("D2G_K3_SUBBATCH")) { const int d = std::atoi(e); if (d >= 1 && d <= 8) v.subbatch = (size_t)d; }
    if (const char *e = t.get("D2G_K3_ROUND_KEYS")) { const int d = std::atoi(e); if (d >= 1 && d <= K3_ROUND_KEYS) v.round_keys = (uint32_t)d; }
    if (const char *e = t.get("D2G_K3_GUESS_SCALE")) { const double d = std::atof(e); if (d > 0.) v.guess_scale = d; }
    if (const char *e = t.get("D2G_K3_GRID_PER_CU")) { const int d = std::atoi(e); if (d >= 1 && d <= 256) v.grid_per_cu = (size_t)d; }
    if (const char *e = t.get("D2G_K3_GQ_SCALE")) { v.gq_scale_set = true; v.gq_scale = std::max(0.0, std::atof(e)); }
    v.gq_slack = v.gq_scale_set ? 1 : v.grid_per_cu > 24 ? 256 : 1024;
    if (const char *e = t.get("D2G_K3S_RANGE_KEYS")) { const long d = std::atol(e); if (d >= 1 && d <= K3_TARGET) v.sort_keys = (uint64_t)d; }
    if (const char *e = t.get("D2G_CS_TABLE_BYTES")) { const long long d = std::atoll(e); if (d >= 1) v.cs_table_bytes = (uint64_t)d; }
    if (const char *e = t.get("D2G_CS_LDS_CELLS")) { const int d = std::atoi(e); if (d >= 0 && d <= 40960) v.cs_lds_cells = d; }
    return v;
}

void d2g_tuning_resolve(d2g_ctx *c) {
    d2g_tuning_load(c->tune);
    c->k2 = d2g_k2_tuning_resolve(c->tune);
    c->k3_tune = d2g_k3_tuning_resolve(c->tune);
    c->kset = d2g_kset_tuning();
    if (const char *e = c->tune.get("D2G_KSET_SPLIT")) { const int v = std::atoi(e); if (v >= 1 && v <= 65535) c->kset.split = v; }
    if (const char *e = c->tune.get("D2G_KSET_PBITS")) { const int v = std::atoi(e); if (v >= 0 && v <= 20) c->kset.pbits = v; }
    c->edit = d2g_edit_tuning();
    if (const char *e = c->tune.get("D2G_EDIT_STRIP")) { const int v = std::atoi(e); if (v >= 1 && v <= 64) c->edit.strip = v; }
    if (const char *e = c->tune.get("D2G_EDIT_TILE")) { const int v = std::atoi(e); if (v >= 1 && v <= 65536) c->edit.tile = v; }
    if (const char *e = c->tune.get("D2G_EDIT_NEAR_ROUTE")) { const int v = std::atoi(e); if (v >= 0 && v <= 2) c->edit.near_route = v; }
    if (const char *e = c->tune.get("D2G_EDIT_DEDUP_ROUTE")) { const int v = std::atoi(e); if (v >= 0 && v <= 2) c->edit.dedup_route = v; }
    if (const char *e = c->tune.get("D2G_EDIT_DEDUP_REVERSE")) c->edit.dedup_reverse = std::atoi(e) != 0;
    c->limits = d2g_limits_tuning_resolve(c->tune);
    c->mgpu_chunks = 0;
    if (const char *e = c->tune.get("D2G_MGPU_CHUNKS")) { const int v = std::atoi(e); if (v >= 1 && v <= MG_MAX_CHUNKS) c->mgpu_chunks = v; }
}

extern "C" {

int d2g_ctx_reload_tuning(d2g_ctx *c) {
    if (!c) return D2G_ERR_INVALID;
    d2g_tuning_resolve(c);
    return D2G_OK;
}

// {"D2G_X": "value", ...} of the switches this context resolved; returns the length needed (excluding the terminator)
int d2g_ctx_tuning(const d2g_ctx *c, char *buf, size_t cap) {
    if (!c) return D2G_ERR_INVALID;
    std::string j = "{";
    for (size_t i = 0; i < c->tune.kv.size(); ++i) {
        if (i) j += ", ";
        j += "\"" + c->tune.kv[i].first + "\": \"";
        for (char ch : c->tune.kv[i].second) { if (ch == '"' || ch == '\\') j += '\\'; if ((unsigned char)ch >= 0x20) j += ch; }
        j += "\"";
    }
    // ... and what the switches that select K2's kernels and thresholds RESOLVED to, set or not (the bench line's `tuning` names the defaults)
    // ... and to the limits of d2g_limits.h (tests compute a loop's piece count from them)
    std::string res = d2g_k2_tuning_json(c);
    const d2g_limits_tuning &l = c->limits;
    char lb[512];
    std::snprintf(lb, sizeof lb, ", \"D2G_KNN_CHUNK_SLOTS\": %zu, \"D2G_EDIT_KNN_CHUNK_SLOTS\": %zu, \"D2G_INTERVAL_LIST_POSITIONS\": %llu, \"D2G_SCREEN_RESULT_PAIRS\": %llu, "
                  "\"D2G_EDIT_GRID_MAX\": %u, \"D2G_EDIT_DEDUP_CHUNK\": %u, \"D2G_EDIT_DEDUP_MAX_CHUNKS\": %u}",
                  l.knn_chunk_slots, l.edit_knn_chunk_slots, (unsigned long long)l.interval_list_positions, (unsigned long long)l.screen_result_pairs,
                  l.edit_grid_max, l.edit_dedup_chunk, l.edit_dedup_max_chunks);
    res.replace(res.rfind('}'), 1, lb);
    j += std::string(c->tune.kv.empty() ? "" : ", ") + "\"resolved\": " + res;
    j += "}";
    if (buf && cap) { std::snprintf(buf, cap, "%s", j.c_str()); }
    return (int)j.size();
}

int d2g_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int d2g_ctx_create(int device, d2g_ctx **out) {
    if (!out) return D2G_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return D2G_ERR_NODEVICE;
    if (device < 0 || device >= n) return D2G_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return D2G_ERR_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return D2G_ERR_NODEVICE;
    // this library carries gfx950 code objects only
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return D2G_ERR_NODEVICE;
    d2g_ctx *c = new (std::nothrow) d2g_ctx();
    if (!c) return D2G_ERR_NOMEM;
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    d2g_tuning_resolve(c);
    *out = c;
    return D2G_OK;
}

void d2g_ctx_destroy(d2g_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->k3) d2g_k3_state_destroy(c->k3);
    delete c;
}

const char *d2g_last_error(const d2g_ctx *c) { return c ? c->last_error.c_str() : "null ctx"; }
int d2g_ctx_device(const d2g_ctx *c) { return c ? c->device : -1; }

int d2g_sync(d2g_ctx *c, void *stream) {
    if (!c) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    D2G_HIP(c, hipStreamSynchronize(as_stream(stream)));
    return D2G_OK;
}

int d2g_malloc(d2g_ctx *c, size_t nbytes, void **dptr) {
    if (!c || !dptr) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    D2G_HIP(c, hipMalloc(dptr, nbytes ? nbytes : 1));
    return D2G_OK;
}
int d2g_free(d2g_ctx *c, void *dptr) {
    if (!c) return D2G_ERR_INVALID;
    if (!dptr) return D2G_OK;
    D2G_HIP(c, hipSetDevice(c->device));
    D2G_HIP(c, hipFree(dptr));
    return D2G_OK;
}
int d2g_mem_info(d2g_ctx *c, size_t *free_bytes, size_t *total_bytes) {
    if (!c) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    size_t f = 0, t = 0;
    D2G_HIP(c, hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return D2G_OK;
}
int d2g_malloc_host(d2g_ctx *c, size_t nbytes, void **hptr) {
    if (!c || !hptr) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    D2G_HIP(c, hipHostMalloc(hptr, nbytes ? nbytes : 1, hipHostMallocDefault));
    return D2G_OK;
}
// page-lock memory the caller already owns (e.g. staging buffers that were being filled before the context existed)
int d2g_host_register(d2g_ctx *c, void *hptr, size_t nbytes) {
    if (!c || !hptr || !nbytes) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    D2G_HIP(c, hipHostRegister(hptr, nbytes, hipHostRegisterDefault));
    return D2G_OK;
}
int d2g_host_unregister(d2g_ctx *c, void *hptr) {
    if (!c || !hptr) return D2G_ERR_INVALID;
    D2G_HIP(c, hipHostUnregister(hptr));
    return D2G_OK;
}
int d2g_free_host(d2g_ctx *c, void *hptr) {
    if (!c) return D2G_ERR_INVALID;
    if (!hptr) return D2G_OK;
    D2G_HIP(c, hipHostFree(hptr));
    return D2G_OK;
}
int d2g_memcpy_h2d(d2g_ctx *c, void *dst, const void *src, size_t n, void *stream) {
    if (!c || (n && (!dst || !src))) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    D2G_HIP(c, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, as_stream(stream)));
    D2G_HIP(c, hipStreamSynchronize(as_stream(stream)));
    return D2G_OK;
}
int d2g_memcpy_d2h(d2g_ctx *c, void *dst, const void *src, size_t n, void *stream) {
    if (!c || (n && (!dst || !src))) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    D2G_HIP(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, as_stream(stream)));
    D2G_HIP(c, hipStreamSynchronize(as_stream(stream)));
    return D2G_OK;
}

// see d2g.h
int d2g_warmup(d2g_ctx *c, int what) {
    if (!c) return D2G_ERR_INVALID;
    D2G_HIP(c, hipSetDevice(c->device));
    if (what & D2G_WARM_COPY) {
        // the first host<->device copy of a process sets up the runtime's copy machinery (~30 ms on MI355X / ROCm 7: measured with any
        // size and with pinned or pageable memory alike; a 4 KB copy leaves part of it to the first large one, 1 MB does not)
        std::vector<char> src((size_t)1 << 20);                 // per call: two helper threads may warm two contexts at once
        d2g_dev<char> d;
        if (int rc = d.alloc(c, src.size(), "warmup alloc")) return rc;
        hipError_t e = hipMemcpy(d, src.data(), src.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(src.data(), d, 4096, hipMemcpyDeviceToHost);
        D2G_HIP(c, e);
    }
    if (what & D2G_WARM_K0) d2g_warm_k0();
    if (what & D2G_WARM_K1) d2g_warm_k1();
    if (what & D2G_WARM_K1I) d2g_warm_k1i();
    if (what & D2G_WARM_K2) { d2g_warm_k2(); d2g_warm_k2_bitslice(); d2g_warm_k2_planes(); d2g_warm_knn(); d2g_warm_dedup(); }
    if (what & D2G_WARM_K3) d2g_warm_k3();
    if (what & D2G_WARM_KSET) d2g_warm_kset();
    if (what & D2G_WARM_SCREEN) d2g_warm_screen();
    if (what & D2G_WARM_EDIT) { d2g_warm_edit(); d2g_warm_edit_near(); d2g_warm_edit_dedup(); }
    return D2G_OK;
}
int d2g_device_name(int device, char *buf, size_t cap) {
    if (!buf || !cap) return D2G_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return D2G_ERR_NODEVICE;
    std::snprintf(buf, cap, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return D2G_OK;
}

int d2g_set_timing(d2g_ctx *c, int enabled) {
    if (!c) return D2G_ERR_INVALID;
    c->timing = enabled == 1 ? (D2G_TIME_K1 | D2G_TIME_K2 | D2G_TIME_K2PREP | D2G_TIME_K3 | D2G_TIME_KNN | D2G_TIME_DEDUP | D2G_TIME_FILTER | D2G_TIME_KSET | D2G_TIME_SCREEN | D2G_TIME_EDIT | D2G_TIME_EDIT_NEAR | D2G_TIME_EDIT_DEDUP) : (enabled & ~1);
    return D2G_OK;
}

int d2g_kernel_ms(d2g_ctx *c, const char *which, int reset, int *count, float *avg_ms, float *last_ms) {
    if (!c || !which) return D2G_ERR_INVALID;
    d2g_evlog *e = nullptr, *e2 = nullptr;                   // e2: a second log summed under the same name
    if (!std::strcmp(which, "k1")) e = &c->ev_k1;
    else if (!std::strcmp(which, "k1count")) e = &c->ev_k1count;
    else if (!std::strcmp(which, "k1i")) e = &c->ev_k1i;
    else if (!std::strcmp(which, "k1iexpand")) e = &c->ev_k1iexpand;
    else if (!std::strcmp(which, "k1ibmh")) e = &c->ev_k1ibmh;
    else if (!std::strcmp(which, "filter")) e = &c->ev_filter;
    else if (!std::strcmp(which, "k2")) e = &c->ev_k2;
    else if (!std::strcmp(which, "k2prep")) e = &c->ev_k2prep;
    else if (!std::strcmp(which, "k3")) e = &c->ev_k3;
    else if (!std::strcmp(which, "k3s")) e = &c->ev_k3s;
    else if (!std::strcmp(which, "k3k")) e = &c->ev_k3k;
    else if (!std::strcmp(which, "k3kcompact")) e = &c->ev_k3kcompact;
    else if (!std::strcmp(which, "k3kbmh")) e = &c->ev_k3kbmh;
    else if (!std::strcmp(which, "kset")) e = &c->ev_kset;
    else if (!std::strcmp(which, "ksetprep")) e = &c->ev_ksetprep;
    else if (!std::strcmp(which, "edit")) e = &c->ev_edit;
    else if (!std::strcmp(which, "editprep")) e = &c->ev_editprep;
    else if (!std::strcmp(which, "editnear")) e = &c->ev_editnear;
    else if (!std::strcmp(which, "editdedup")) e = &c->ev_editdedup;
    else if (!std::strcmp(which, "editdedup_list")) e = &c->ev_editdedup_list;
    else if (!std::strcmp(which, "editdedup_resolve")) e = &c->ev_editdedup_resolve;
    else if (!std::strcmp(which, "screen")) e = &c->ev_screen;
    else if (!std::strcmp(which, "screenreduce")) e = &c->ev_screenreduce;
    else if (!std::strcmp(which, "screenbuild")) e = &c->ev_screenbuild;
    else if (!std::strcmp(which, "k0")) e = &c->ev_k0;
    else if (!std::strcmp(which, "knn")) e = &c->ev_knn;
    else if (!std::strcmp(which, "dedup")) { e = &c->ev_dedup; e2 = &c->ev_dedup_resolve; }
    else if (!std::strcmp(which, "dedup_resolve")) e = &c->ev_dedup_resolve;
    D2G_CHECK(c, e != nullptr, "d2g_kernel_ms: unknown kernel name");
    D2G_HIP(c, hipSetDevice(c->device));
    double sum = 0;
    float last = 0.f;
    int n = 0;
    for (d2g_evlog *l : {e, e2}) {
        if (!l) continue;
        for (size_t i = 0; i < l->a.size(); ++i) {
            D2G_HIP(c, hipEventSynchronize(l->b[i]));
            D2G_HIP(c, hipEventElapsedTime(&last, l->a[i], l->b[i]));
            sum += last;
        }
        n += (int)l->a.size();
    }
    if (count) *count = n;
    if (avg_ms) *avg_ms = n ? (float)(sum / n) : 0.f;
    if (last_ms) *last_ms = last;
    if (reset) for (d2g_evlog *l : {e, e2}) if (l) { l->a.clear(); l->b.clear(); }
    return D2G_OK;
}

}  // extern "C"
