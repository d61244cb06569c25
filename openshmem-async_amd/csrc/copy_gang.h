// The CPU side of host staging (staging.cpp), free of HIP so that it builds
// and runs alone (tests/native/test_copy_gang.cpp): a byte copy with optional
// streaming stores, and a gang of pinned threads that splits one copy at a
// time among its workers.
#pragma once

#include <immintrin.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace shmx {

// A copy whose stores bypass the caches (32-byte non-temporal stores, then a
// store fence): a destination that is only read again by a DMA engine or,
// much later, by the program gains nothing from being cached, and the
// streaming stores skip the read-for-ownership of every destination line that
// a cached store pays (one memory read fewer per byte).  AVX2 when the CPU
// has it, memcpy otherwise.
__attribute__((target("avx2"))) inline void nt_copy_avx2(char *dst, const char *src, size_t n) {
    const size_t head = std::min(n, (size_t)((32 - ((uintptr_t)dst & 31)) & 31));
    if (head) std::memcpy(dst, src, head);
    size_t i = head;
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 32));
        const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 64));
        const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), a);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 64), c);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 96), d);
    }
    if (i < n) std::memcpy(dst + i, src + i, n - i);
    _mm_sfence();
}

inline void copy_bytes(char *dst, const char *src, size_t n, bool nt) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (nt && avx2) nt_copy_avx2(dst, src, n);
    else std::memcpy(dst, src, n);
}

// confine a thread to `cpus` (empty: wherever the scheduler puts it)
inline void pin_thread(std::thread &t, const std::vector<int> &cpus) {
    if (cpus.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int c : cpus) CPU_SET(c, &set);
    (void)pthread_setaffinity_np(t.native_handle(), sizeof set, &set);
}

// A gang of CPU threads that runs one copy at a time, cut into pieces of
// bytes / pieces rounded up to 64 bytes, one piece per thread.  Two uses:
// - start / wait, by one owner thread: the workers copy in the background
//   while the owner does other work (the pageable staging pipeline has two
//   gangs, one filling the page-locked ring and one emptying it, at the same
//   time: one pool doing both in turn left each copy waiting for the other,
//   DESIGN.md §6);
// - copy, from any thread: the caller takes the first piece itself and
//   returns when every piece is done (parallel_copy).
// A gang serves one of the two uses, not both at once.
class CopyGang {
  public:
    // below this size, copy() is not worth waking the workers for
    static constexpr size_t kAloneBelow = size_t(4) << 20;

    // one worker per entry, on that entry's CPUs (empty: unpinned)
    explicit CopyGang(const std::vector<std::vector<int>> &worker_cpus) {
        for (unsigned i = 0; i < worker_cpus.size(); ++i) {
            workers_.emplace_back([this, i] { run(i); });
            pin_thread(workers_.back(), worker_cpus[i]);
        }
    }
    ~CopyGang() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    CopyGang(const CopyGang &) = delete;
    CopyGang &operator=(const CopyGang &) = delete;

    // nt: streaming stores (copy_bytes).  Waits for the previous copy first;
    // a gang without workers copies here and now.
    void start(void *dst, const void *src, size_t bytes, bool nt) {
        wait();
        if (workers_.empty()) copy_bytes(static_cast<char *>(dst), static_cast<const char *>(src), bytes, nt);
        else post(dst, src, bytes, nt, 0);
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
    }
    // One caller at a time: a second concurrent caller (the mirrored heap's
    // fault handler on another thread) copies on its own.
    void copy(void *dst, const void *src, size_t bytes) {
        if (bytes < kAloneBelow || workers_.empty() || busy_.exchange(true, std::memory_order_acquire)) {
            std::memcpy(dst, src, bytes);
            return;
        }
        post(dst, src, bytes, false, 1);
        piece(0);
        wait();
        busy_.store(false, std::memory_order_release);
    }

  private:
    // a new copy for the workers: worker i takes piece first + i
    void post(void *dst, const void *src, size_t bytes, bool nt, unsigned first) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            dst_ = static_cast<char *>(dst);
            src_ = static_cast<const char *>(src);
            bytes_ = bytes;
            nt_ = nt;
            first_ = first;
            pending_ = (unsigned)workers_.size();
            ++gen_;
        }
        cv_.notify_all();
    }
    void piece(unsigned i) {
        const size_t n = workers_.size() + first_;
        // (the quotient rounded up: rounded down, n pieces fall short of the
        // end when it is a multiple of 64 and bytes_ is no multiple of n)
        const size_t per = ((bytes_ + n - 1) / n + 63) & ~size_t(63);
        const size_t lo = std::min(bytes_, per * i), hi = std::min(bytes_, per * (i + 1));
        if (hi > lo) copy_bytes(dst_ + lo, src_ + lo, hi - lo, nt_);
    }
    void run(unsigned i) {
        unsigned long long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            piece(first_ + i);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> workers_;
    std::atomic<bool> busy_{false};
    std::mutex mu_;
    std::condition_variable cv_, done_;
    bool stop_ = false;
    unsigned long long gen_ = 0;
    unsigned pending_ = 0;     // workers that have not finished the posted copy
    char *dst_ = nullptr;
    const char *src_ = nullptr;
    size_t bytes_ = 0;
    unsigned first_ = 0;
    bool nt_ = false;
};

}  // namespace shmx
