// plan_pool.h -- the process-wide workers that plan a batch's distinct states in parallel (header only, standard library only).
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace rsmp {

// Process-wide workers for planning batches of streams in distinct states (rsmp_fir_batch_resample_bulk_device): the
// items of a run are claimed from an atomic counter by the pool's threads and by the caller; one run at a time.
// Everything a run shares with the workers lives in ONE object per run (its function, its item count, its claim
// counter, its completion count), handed over under the mutex: a worker that wakes up late holds either the finished
// run (nothing left to claim) or the current one -- never one run's counter with another run's bounds.
class PlanPool {
public:
    PlanPool() { ensure_threads(64); }   // (at library load: creating up to 63 threads inside the first timed launch cost it milliseconds)
    ~PlanPool() {
        {
            std::lock_guard<std::mutex> lock(mu_);
            stop_ = true;
        }
        cv_work_.notify_all();
        for (std::thread& t : threads_) t.join();
    }
    template <class F>
    void run(size_t total, F&& fn) {
        std::lock_guard<std::mutex> one_run(run_mu_);
        auto job = std::make_shared<Job>();
        job->fn = fn;
        job->total = total;
        {
            std::lock_guard<std::mutex> lock(mu_);
            job_ = job;
            ++generation_;
        }
        cv_work_.notify_all();
        drain(*job);
        std::unique_lock<std::mutex> lock(mu_);
        cv_done_.wait(lock, [&] { return job->done == job->total; });
        job_.reset();
    }

private:
    struct Job {
        std::function<void(size_t)> fn;
        size_t total = 0;
        std::atomic<size_t> next{0};
        size_t done = 0;   // (under mu_)
    };
    void ensure_threads(size_t total) {
        unsigned hw = std::thread::hardware_concurrency();
        const size_t want = std::min<size_t>(total - 1, std::min<size_t>(hw > 1 ? hw - 1 : 0, 63));
        while (threads_.size() < want) threads_.emplace_back([this] { loop(); });
    }
    void drain(Job& job) {
        for (;;) {
            const size_t m = job.next.fetch_add(1, std::memory_order_relaxed);
            if (m >= job.total) break;
            job.fn(m);
            std::lock_guard<std::mutex> lock(mu_);
            if (++job.done == job.total) cv_done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::shared_ptr<Job> job;
            {
                std::unique_lock<std::mutex> lock(mu_);
                cv_work_.wait(lock, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                job = job_;   // (null: the run this wake-up was for has finished)
            }
            if (job) drain(*job);
        }
    }
    std::mutex mu_, run_mu_;
    std::condition_variable cv_work_, cv_done_;
    std::vector<std::thread> threads_;
    std::shared_ptr<Job> job_;
    uint64_t generation_ = 0;
    bool stop_ = false;
};
inline PlanPool& plan_pool() {
    static PlanPool* pool = new PlanPool();   // (leaked on purpose: joining workers from a static destructor at exit races the runtime's teardown)
    return *pool;
}
// (the workers must not be created inside the first launch that needs them; ADVICE r04: nor from a
// static initialiser at dlopen, for every user of the library.  They are created by the first ResamplerFir constructor
// of the process -- rsmp_fir_new_from_hz, fir_api.cpp -- and idle on a condition variable from then on: at most 63 threads,
// hardware_concurrency() - 1 if that is less.)

}  // namespace rsmp
