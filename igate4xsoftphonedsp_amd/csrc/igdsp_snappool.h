// igdsp_snappool.h — the helper threads that share out a flush's host-side snapshot at many channels, for both flushes: the RX
// flush (igdsp_flush_begin, csrc/igdsp_rxstage.h) and the TX flush (igdsp_tx_flush, csrc/igdsp_txstage.h).  Host-only C++17, no
// HIP include: igdsp_capi_ctx.hip and igdsp_capi_tx.hip use it, and tests/san/rx_stage_tsan.cpp drives it under ThreadSanitizer.
//
// A pool is sized once, when its owner is created (pool_threads), and is only ever run by that owner's flush, one run at a time.
// for_each_part splits a channel range into the parts a run hands out; every part is a contiguous range of its own, so the
// workers never share a channel.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

namespace igdsp {

inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield");
#endif
}

constexpr uint32_t kPoolMinChannels = 16384;            // below this one thread snapshots faster than a pool wakes up
constexpr uint32_t kPoolMaxThreads = 16;               // (8 threads: 0.44-0.53 ms of owner time at 65 536 calls depending on the box; 16: below)
constexpr uint32_t kMaxParts = 64;                      // parts one snapshot is split into at most

// A few persistent helper threads for the flush's snapshot at many channels.  run() hands part i to thread i (the caller takes
// part 0) and returns when all are done.
struct SnapshotPool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_go, cv_done;
    uint64_t epoch = 0;
    uint32_t pending = 0;
    bool quit = false;
    std::function<void(uint32_t)> job;

    explicit SnapshotPool(uint32_t helpers)
    {
        try {
            for (uint32_t i = 0; i < helpers; ++i)
                threads.emplace_back([this, i] {
                    uint64_t seen = 0;
                    for (;;) {
                        std::unique_lock<std::mutex> lk(m);
                        cv_go.wait(lk, [&] { return quit || epoch != seen; });
                        if (quit) return;
                        seen = epoch;
                        lk.unlock();
                        job(i + 1);
                        lk.lock();
                        if (--pending == 0) cv_done.notify_one();
                    }
                });
        } catch (...) {                                // a thread could not be started: stop the ones that were, then report it
            stop();
            throw;
        }
    }
    ~SnapshotPool() { stop(); }
    void run(const std::function<void(uint32_t)> &fn)
    {
        { std::lock_guard<std::mutex> lk(m); job = fn; pending = (uint32_t)threads.size(); ++epoch; }
        cv_go.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return pending == 0; });
    }

private:
    void stop()
    {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv_go.notify_all();
        for (auto &t : threads) t.join();
    }
};

// Threads (the caller's included) the snapshot of `channels` channels is shared out to: none below kPoolMinChannels, else at
// least 4 096 channels per thread, at most kPoolMaxThreads and half the hardware threads; IGDSP_FLUSH_THREADS overrides (1..64).
inline uint32_t pool_threads(uint32_t channels)
{
    if (channels < kPoolMinChannels) return 1;
    const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
    uint32_t threads = std::min(std::min(kPoolMaxThreads, std::max(1u, hw / 2u)), channels / (kPoolMinChannels / 4u));
    if (const char *e = std::getenv("IGDSP_FLUSH_THREADS")) threads = (uint32_t)std::max(1, std::min(64, std::atoi(e)));
    return threads;
}

// The pool for `channels` channels, or nullptr when one thread is to snapshot alone — also when the pool cannot be allocated or
// its threads cannot be started: the snapshot then runs on the caller's thread.
inline std::unique_ptr<SnapshotPool> make_pool(uint32_t channels)
{
    const uint32_t threads = pool_threads(channels);
    if (threads < 2u) return nullptr;
    try {
        return std::unique_ptr<SnapshotPool>(new (std::nothrow) SnapshotPool(threads - 1u));
    } catch (const std::system_error &) {
        return nullptr;
    }
}

// Split [0, n) into parts i = [n * i / parts, n * (i + 1) / parts) — one per pool thread, capped at kMaxParts; one part without a
// pool — and call fn(i, lo, hi) for each: on the caller's thread without a pool, else through pool->run.  Returns the part count.
template <typename Fn>
inline uint32_t for_each_part(SnapshotPool *pool, uint32_t n, Fn &&fn)
{
    const uint32_t parts = pool ? std::min<uint32_t>((uint32_t)pool->threads.size() + 1u, kMaxParts) : 1u;
    auto part = [&](uint32_t i) {
        if (i < parts) fn(i, (uint32_t)((uint64_t)n * i / parts), (uint32_t)((uint64_t)n * (i + 1) / parts));
    };
    if (parts == 1) part(0);
    else pool->run(part);
    return parts;
}

}  // namespace igdsp
