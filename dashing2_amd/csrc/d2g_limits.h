// d2g_limits.h -- the snapshot of the library's D2G_* switches, and the limits that cut a large call into pieces (plain C++: the
// host self-tests include it without a GPU tool chain).
//
// Each limit below sizes a host loop that runs its body once at any shape a test can afford: the chunks of rows of d2g_cmp_set_knn and
// d2g_edit_knn, the groups of files of d2g_interval_bmh_sketch, the passes of d2g_screen_result, the launches of the edit-distance
// kernels, the workgroups of d2g_edit_dedup_dev's compaction.  A switch shrinks one limit so that a small input enters the second
// piece; unset or out of range it is the constant, and no kernel knows about it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

// Every D2G_* switch that selects a kernel, a threshold or a test hook inside the library is read from the environment ONCE per context
// (d2g_ctx_create; again only on d2g_ctx_reload_tuning) and used from this snapshot: a run's timing does not depend on who changed
// the environment in between, d2g_ctx_tuning reports the resolved set, and the multi-GPU engine compares it across ranks.
struct d2g_tuning {
    std::vector<std::pair<std::string, std::string>> kv;      // the switches that were set, in the order of d2g_tuning_names()
    const char *get(const char *name) const {                 // nullptr = not set
        for (const auto &p : kv) if (p.first == name) return p.second.c_str();
        return nullptr;
    }
};

constexpr size_t KNN_CHUNK_SLOTS = (size_t)1 << 24;         // d2g_cmp_set_knn: candidate slots per chunk of rows (2 x 64 MB on the device)
constexpr size_t NEAR_CHUNK_SLOTS = (size_t)1 << 24;        // d2g_edit_knn: candidate slots per chunk of rows
constexpr uint64_t SCREEN_RESULT_PAIRS = 1ull << 30;        // d2g_screen_result: (row, reference) pairs per launch, a wave each
constexpr uint32_t EDIT_GRID_MAX = 0x7fffffffu;             // the edit-distance kernels: workgroups per launch
constexpr uint32_t EDD_THREADS_HOST = 256;                  // d2g_edit_dedup.hip's EDD_THREADS: a compaction workgroup walks a multiple of it
constexpr uint32_t EDD_CHUNK = 1024, EDD_MAX_CHUNKS = 1024; // d2g_edit_dedup_dev's compaction: positions of the order per workgroup, at most so many workgroups

struct d2g_limits_tuning {
    size_t knn_chunk_slots = KNN_CHUNK_SLOTS;           // D2G_KNN_CHUNK_SLOTS: >= 1; the chunk of rows and the budget of a re-run group of d2g_cmp_set_knn
    size_t edit_knn_chunk_slots = NEAR_CHUNK_SLOTS;     // D2G_EDIT_KNN_CHUNK_SLOTS: >= 1; the same two of d2g_edit_knn, at every level of its escalation
    uint64_t interval_list_positions = 0;               // D2G_INTERVAL_LIST_POSITIONS: >= 1 covered positions per group of files of d2g_interval_bmh_sketch; 0 = a third of the free device memory at 16 bytes each
    uint64_t screen_result_pairs = SCREEN_RESULT_PAIRS; // D2G_SCREEN_RESULT_PAIRS: 1 .. 2^30; below a row's pairs: one row per pass
    uint32_t edit_grid_max = EDIT_GRID_MAX;             // D2G_EDIT_GRID_MAX: 1 .. 2^31 - 1; below a row's tiles: one row per launch
    uint32_t edit_dedup_chunk = EDD_CHUNK;              // D2G_EDIT_DEDUP_CHUNK: a multiple of 256 in 256 .. 2^20: the fewest positions per compaction workgroup
    uint32_t edit_dedup_max_chunks = EDD_MAX_CHUNKS;    // D2G_EDIT_DEDUP_MAX_CHUNKS: 1 .. EDD_MAX_CHUNKS compaction workgroups at most (the scratch keeps room for EDD_MAX_CHUNKS counts)
};

inline d2g_limits_tuning d2g_limits_tuning_resolve(const d2g_tuning &t) {
    d2g_limits_tuning v;
    // a whole decimal number in [lo, hi], or nothing: "12x", "", "-3" and what does not fit 64 bits leave the default
    auto num = [&](const char *name, uint64_t lo, uint64_t hi, uint64_t *out) {
        const char *e = t.get(name);
        if (!e || *e < '0' || *e > '9') return false;
        uint64_t x = 0;
        for (; *e >= '0' && *e <= '9'; ++e) { const uint64_t d = (uint64_t)(*e - '0'); if (x > (UINT64_MAX - d) / 10) return false; x = x * 10 + d; }
        if (*e || x < lo || x > hi) return false;
        *out = x;
        return true;
    };
    uint64_t x = 0;
    if (num("D2G_KNN_CHUNK_SLOTS", 1, SIZE_MAX, &x)) v.knn_chunk_slots = (size_t)x;
    if (num("D2G_EDIT_KNN_CHUNK_SLOTS", 1, SIZE_MAX, &x)) v.edit_knn_chunk_slots = (size_t)x;
    if (num("D2G_INTERVAL_LIST_POSITIONS", 1, UINT64_MAX / 16, &x)) v.interval_list_positions = x;
    if (num("D2G_SCREEN_RESULT_PAIRS", 1, SCREEN_RESULT_PAIRS, &x)) v.screen_result_pairs = x;
    if (num("D2G_EDIT_GRID_MAX", 1, EDIT_GRID_MAX, &x)) v.edit_grid_max = (uint32_t)x;
    if (num("D2G_EDIT_DEDUP_CHUNK", EDD_THREADS_HOST, 1u << 20, &x) && x % EDD_THREADS_HOST == 0) v.edit_dedup_chunk = (uint32_t)x;
    if (num("D2G_EDIT_DEDUP_MAX_CHUNKS", 1, EDD_MAX_CHUNKS, &x)) v.edit_dedup_max_chunks = (uint32_t)x;
    return v;
}

// positions of the order per compaction workgroup of d2g_edit_dedup_dev over N records: a multiple of 256, so that at most
// max_chunks workgroups cover N
inline uint32_t d2g_edit_dedup_chunk(uint32_t N, const d2g_limits_tuning &t) {
    const uint32_t per = (N + t.edit_dedup_max_chunks - 1) / t.edit_dedup_max_chunks;
    const uint32_t need = (per + EDD_THREADS_HOST - 1) / EDD_THREADS_HOST * EDD_THREADS_HOST;
    return need > t.edit_dedup_chunk ? need : t.edit_dedup_chunk;
}
