// bounded_queue.h -- a closable FIFO with a size bound, for many producers and many consumers.
// push() blocks while the queue is full; pop() blocks until an item arrives, or reports the end once the queue is closed and
// empty.  The queue closes when the last of its `producers` calls producer_done(), or on an explicit close().
// `dashing2 sketch` uses two: reader threads -> device threads (ingest_pipeline.h), device threads -> finisher (sketch_cmd.cpp).
// Exercised under ThreadSanitizer by `make tsan` in dashing2_amd/csrc.
#pragma once
#include <condition_variable>
#include <cstddef>
#include <deque>
#include <mutex>
#include <utility>

namespace d2h {

template <class T>
class BoundedQueue {
    std::mutex m_;
    std::condition_variable cv_item_, cv_space_;
    std::deque<T> q_;                                 // guarded by m_
    size_t producers_;                                // guarded by m_: producers that have not called producer_done() yet
    bool closed_ = false;                             // guarded by m_
    const size_t bound_;
public:
    explicit BoundedQueue(size_t bound, size_t producers = 0) : producers_(producers), bound_(bound ? bound : 1) {}
    BoundedQueue(const BoundedQueue &) = delete;
    BoundedQueue &operator=(const BoundedQueue &) = delete;
    void push(T v) {                                  // blocks while the queue is full
        std::unique_lock<std::mutex> lk(m_);
        cv_space_.wait(lk, [&] { return q_.size() < bound_; });
        q_.push_back(std::move(v));
        cv_item_.notify_one();
    }
    bool pop(T &out) {                                // false: closed and empty, nothing more will come
        std::unique_lock<std::mutex> lk(m_);
        cv_item_.wait(lk, [&] { return closed_ || !q_.empty(); });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        cv_space_.notify_one();
        return true;
    }
    void close() {
        { std::lock_guard<std::mutex> lk(m_); closed_ = true; }
        cv_item_.notify_all();
    }
    void producer_done() {                            // the last producer to finish closes the queue
        bool last;
        { std::lock_guard<std::mutex> lk(m_); last = producers_ && --producers_ == 0; closed_ = closed_ || last; }
        if (last) cv_item_.notify_all();
    }
};

}  // namespace d2h
