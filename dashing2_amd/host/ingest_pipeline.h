// ingest_pipeline.h -- the host ingest of `dashing2 sketch`: the one owner of the reader threads, the recycled
// d2g_seqpack pool, the staging buffers with their free list, and the queue of groups that are ready for a device thread.
// Header-only over include/d2g.h's d2g_seqpack_* (host code) and the standard library: no GPU, no d2g_ctx, no OpenMP, and no
// environment variable is read here -- the caller passes every choice in, so `make tsan` (dashing2_amd/csrc) drives this very code.
//
// Reader threads take whole groups of input lines.  A group whose files are all regular files starting with '>' is read raw
// into a staging buffer for the device parser (K0) -- if a buffer is free at that moment; readers never wait for one.  Every
// other group is parsed and 2-bit-packed by the reader itself (d2g_seqpack).  A group that fails is still queued, empty, so that
// no consumer stalls; the first error is kept and the caller ends the run with it.
#pragma once
#include "../../include/d2g.h"
#include "bounded_queue.h"
#include "fileutil.h"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace d2h {

struct FileRef { std::string path; size_t size; };

// groups of input lines bounded by input bytes: read in parallel on the host, sketched one group per launch
struct GroupPlan {
    std::vector<std::vector<FileRef>> files_of;         // the space-separated paths of every input line, with their sizes
    std::vector<std::pair<size_t, size_t>> groups;      // [begin, end) into the lines
    std::vector<size_t> group_bytes;                    // sizes rounded up to 16, summed per group
};
// A line is split on spaces; a group closes when the next line would take it past `limit`, but never while it is empty.
inline GroupPlan plan_groups(const std::vector<std::string> &lines, size_t limit,
                             const std::function<size_t(const std::string &)> &size_of = filesize) {
    GroupPlan p;
    p.files_of.resize(lines.size());
    size_t b = 0, acc = 0;
    for (size_t t = 0; t < lines.size(); ++t) {
        size_t fs = 0;
        const std::string &line = lines[t];
        for (size_t s = 0; s <= line.size();) {
            size_t e = line.find(' ', s);
            if (e == std::string::npos) e = line.size();
            if (e > s) { const std::string f = line.substr(s, e - s); const size_t z = size_of(f); p.files_of[t].push_back({f, z}); fs += (z + 15) / 16 * 16; }
            s = e + 1;
        }
        if (acc && acc + fs > limit) { p.groups.emplace_back(b, t); p.group_bytes.push_back(acc); b = t; acc = 0; }
        acc += fs;
    }
    if (b < lines.size()) { p.groups.emplace_back(b, lines.size()); p.group_bytes.push_back(acc); }
    return p;
}

struct IngestConfig { int k; size_t readers, nbufs, buf_bytes, max_ready; int alphabet = 0; };    // alphabet: D2G_ALPHABET_* of the host packers
// The sizes `dashing2 sketch` runs with.  (A byte-bounded queue deep enough to parse all of 1000 x 5 Mbp before the first launch,
// with four device threads to drain it, was measured: the 112 freshly allocated packers fault in 1.3 GB and the pipeline went
// 0.21 -> 0.34 s.  The recycled pool stays.)
inline IngestConfig ingest_config(const GroupPlan &plan, int k, size_t workers, bool host_parser_only, int alphabet = 0) {
    IngestConfig c;
    c.k = k; c.alphabet = alphabet;
    c.readers = std::max<size_t>(1, std::min<size_t>({workers, plan.groups.size(), size_t(192)}));
    c.max_ready = 2 * c.readers + 2;
    size_t max_group = 16;
    for (size_t gb : plan.group_bytes) max_group = std::max(max_group, gb);
    c.buf_bytes = (max_group + 4095) / 4096 * 4096 + 4096;
    c.nbufs = host_parser_only ? 0 : std::min<size_t>(plan.groups.size(), std::max<size_t>(3, std::min<size_t>(c.readers + 2, (size_t(1) << 30) / c.buf_bytes)));
    return c;
}

// One group as a consumer gets it: raw bytes in staging buffer `buf` (file i at foff[i] .. foff[i] + flen[i], the files of input
// line j are gfo[j] .. gfo[j + 1]), or the packed stream `sp`, or neither: the group failed and only passes through.
struct IngestGroup {
    size_t g = 0;
    d2g_seqpack *sp = nullptr;
    int buf = -1;
    const uint8_t *raw = nullptr;
    size_t raw_bytes = 0;
    std::vector<uint64_t> foff, flen, gfo;
    bool failed() const { return !sp && buf < 0; }
};

class IngestPipeline {
    const std::vector<std::string> &lines_;             // read-only once the readers run
    const GroupPlan &plan_;                             // read-only
    const IngestConfig cfg_;
    std::vector<uint8_t *> bufs_;                       // written by the constructing thread only, before the readers start
    BoundedQueue<IngestGroup> ready_;                   // its own lock
    std::vector<std::thread> readers_;                  // constructing thread only
    std::mutex mu_;
    std::vector<d2g_seqpack *> pool_;                   // guarded by mu_: recycled packers (allocations kept)
    std::vector<int> free_bufs_;                        // guarded by mu_
    size_t next_group_ = 0;                             // guarded by mu_
    std::string error_;                                 // guarded by mu_; read by the caller after join()
    double t_read_raw_ = 0, t_host_pack_ = 0, t_readers_ = 0;   // guarded by mu_; read by the caller after join()

    // eligible for the device parser: every file of the group is a plain file whose first byte is '>'
    bool device_parsable(size_t g) const {
        for (size_t x = plan_.groups[g].first; x < plan_.groups[g].second; ++x)
            for (const FileRef &fr : plan_.files_of[x]) {
                if (!isfile(fr.path)) return false;     // missing / not a regular file (FIFO, ...): the host path reports or reads it
                if (fr.size == 0) continue;
                char c0 = 0;
                std::FILE *fp = std::fopen(fr.path.c_str(), "rb");
                const bool ok = fp && std::fread(&c0, 1, 1, fp) == 1 && c0 == '>';
                if (fp) std::fclose(fp);
                if (!ok) return false;
            }
        return true;
    }
    int read_raw(IngestGroup &r, std::string &bad) const {
        uint8_t *dst = bufs_[r.buf];
        size_t pos = 0;
        int rc = D2G_OK;
        r.raw = dst;
        r.gfo.push_back(0);
        for (size_t x = plan_.groups[r.g].first; rc == D2G_OK && x < plan_.groups[r.g].second; ++x) {
            for (const FileRef &fr : plan_.files_of[x]) {
                r.foff.push_back(pos); r.flen.push_back(fr.size);
                if (fr.size) {
                    std::FILE *fp = std::fopen(fr.path.c_str(), "rb");
                    // a file that changed size since the stat goes to the host parser's error handling
                    if (!fp || pos + fr.size > cfg_.buf_bytes || std::fread(dst + pos, 1, fr.size, fp) != fr.size) { rc = D2G_ERR_IO; bad = fr.path; }
                    if (fp) std::fclose(fp);
                }
                pos += (fr.size + 15) / 16 * 16;
            }
            r.gfo.push_back(r.foff.size());
        }
        r.raw_bytes = pos;
        return rc;
    }
    int pack(IngestGroup &r, std::string &bad) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!pool_.empty()) { r.sp = pool_.back(); pool_.pop_back(); }
        }
        int rc = r.sp ? int(D2G_OK) : d2g_seqpack_create_alphabet(cfg_.k, cfg_.alphabet, &r.sp);
        for (size_t x = plan_.groups[r.g].first; rc == D2G_OK && x < plan_.groups[r.g].second; ++x) {
            rc = d2g_seqpack_add_path(r.sp, lines_[x].c_str());
            if (rc) bad = lines_[x];
        }
        if (rc == D2G_OK) (void)d2g_seqpack_packed_bytes(r.sp);   // pad now, off the device thread
        return rc;
    }
    void reader() {
        for (;;) {
            IngestGroup r;
            bool dev = cfg_.nbufs > 0;
            { std::lock_guard<std::mutex> lk(mu_); r.g = next_group_++; }
            if (r.g >= plan_.groups.size()) break;
            const double t0 = now();
            dev = dev && device_parsable(r.g);
            if (dev) {
                // a staging buffer that is free RIGHT NOW, else this thread packs the group itself: while the GPU context is still
                // being created (or the device threads are behind) the host cores keep producing sketchable groups instead of waiting
                std::lock_guard<std::mutex> lk(mu_);
                if (!free_bufs_.empty()) { r.buf = free_bufs_.front(); free_bufs_.erase(free_bufs_.begin()); } else dev = false;
            }
            std::string bad;
            const int rc = dev ? read_raw(r, bad) : pack(r, bad);
            const double t_work = now() - t0;
            {
                std::lock_guard<std::mutex> lk(mu_);
                (dev ? t_read_raw_ : t_host_pack_) += t_work;
                if (rc && error_.empty()) error_ = "Failed to open " + bad;
            }
            if (rc) {                                    // queued all the same, empty, so that the consumers do not stall
                if (r.sp) d2g_seqpack_destroy(r.sp);
                r.sp = nullptr;
                release_buffer(r);
            }
            ready_.push(std::move(r));
            std::lock_guard<std::mutex> lk(mu_);
            t_readers_ += now() - t0;
        }
        ready_.producer_done();
    }
public:
    // `lines`: the input lines still to sketch; `plan` = plan_groups(lines, ...).  Both outlive the pipeline.  The readers start at once.
    IngestPipeline(const std::vector<std::string> &lines, const GroupPlan &plan, const IngestConfig &cfg)
        : lines_(lines), plan_(plan), cfg_(cfg), bufs_(cfg.nbufs, nullptr), ready_(cfg.max_ready, std::max<size_t>(cfg.readers, 1)) {
        for (size_t i = 0; i < cfg_.nbufs; ++i) {
            void *p = nullptr;
            if (posix_memalign(&p, 4096, cfg_.buf_bytes) != 0) throw std::bad_alloc();
            bufs_[i] = static_cast<uint8_t *>(p);
            free_bufs_.push_back(int(i));
        }
        for (size_t t = 0; t < std::max<size_t>(cfg_.readers, 1); ++t) readers_.emplace_back([this] { reader(); });
    }
    IngestPipeline(const IngestPipeline &) = delete;
    IngestPipeline &operator=(const IngestPipeline &) = delete;
    // joins; frees the packers and whatever staging the caller has not taken over with abandon_buffers()
    ~IngestPipeline() {
        join();
        for (d2g_seqpack *p : pool_) d2g_seqpack_destroy(p);
        for (uint8_t *b : bufs_) std::free(b);
    }
    // (pointer, bytes) of every staging buffer: plain page-aligned memory the readers fill at once; the caller may page-lock it later
    std::vector<std::pair<uint8_t *, size_t>> buffers() const {
        std::vector<std::pair<uint8_t *, size_t>> v;
        for (uint8_t *b : bufs_) v.emplace_back(b, cfg_.buf_bytes);
        return v;
    }
    // the staging memory stays allocated past the pipeline (a process that leaves page-locked memory to its exit); after join()
    void abandon_buffers() { bufs_.clear(); }
    const IngestConfig &config() const { return cfg_; }
    // the next ready group, in no particular order; false: every group has been handed out.  Any number of threads may call it.
    bool next(IngestGroup &r) { return ready_.pop(r); }
    // gives the staging buffer back as soon as its bytes are no longer needed ...
    void release_buffer(IngestGroup &r) {
        if (r.buf < 0) return;
        std::lock_guard<std::mutex> lk(mu_);
        free_bufs_.push_back(r.buf);
        r.buf = -1; r.raw = nullptr;
    }
    // ... and everything the group still holds: the packer returns to the pool, cleared (one the consumer made itself is adopted)
    void release(IngestGroup &r) {
        release_buffer(r);
        if (!r.sp) return;
        d2g_seqpack_clear(r.sp);
        std::lock_guard<std::mutex> lk(mu_);
        pool_.push_back(r.sp);
        r.sp = nullptr;
    }
    // Once next() has returned false the readers are about to exit: join them, then the fields below are stable.
    void join() { for (auto &th : readers_) if (th.joinable()) th.join(); }
    const std::string &error() const { return error_; }     // "Failed to open <path>" of the first group that failed, or empty
    double t_read_raw() const { return t_read_raw_; }       // seconds the readers spent reading raw groups, summed
    double t_host_pack() const { return t_host_pack_; }     // ... reading + packing
    double t_readers() const { return t_readers_; }         // ... in all, the wait for queue space included
};

}  // namespace d2h
