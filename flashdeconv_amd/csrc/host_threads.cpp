// host_threads.h: the CPU budget, and the part of the pool that starts, parks and ends its threads.
#include "host_threads.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <system_error>

namespace fdx {

unsigned host_cpu_budget() {
    static const unsigned budget = [] {
        unsigned hw = std::thread::hardware_concurrency();
        if (hw == 0) hw = 1;
        double cpus = (double)hw;
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[64] = {0};
            long long period = 0;
            if (std::fscanf(f, "%63s %lld", q, &period) == 2 && period > 0 && std::strcmp(q, "max") != 0) cpus = std::min(cpus, atof(q) / (double)period);
            std::fclose(f);
        } else {
            long long quota = -1, period = 0;
            if (FILE* fq = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (std::fscanf(fq, "%lld", &quota) != 1) quota = -1; std::fclose(fq); }
            if (FILE* fp = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(fp, "%lld", &period) != 1) period = 0; std::fclose(fp); }
            if (quota > 0 && period > 0) cpus = std::min(cpus, (double)quota / (double)period);
        }
        return (unsigned)std::max(1.0, std::floor(cpus + 0.5));
    }();
    return budget;
}

void KdPool::want(int members) {
    members = std::max(1, std::min(members, 32));
    if (pid_.load() != getpid()) {
        // A fork()ed child has the object but not the threads, and the mutex / condition variable in whatever state the
        // parent's threads had them in at that instant (a worker about to sleep holds the condition variable's internal
        // lock: the child's first notify would wait for it for ever).  Everything is made anew; the old thread objects are
        // left alone (they cannot be joined).  The first caller in the child does this before anything else runs here.
        new std::vector<std::thread>(std::move(th_));
        new (&th_) std::vector<std::thread>();
        new (&m_) std::mutex();
        new (&cv_) std::condition_variable();
        new (&q_) std::deque<Task>();
        n_queued_.store(0);
        active_.store(1);
        pid_.store(getpid());
    }
    std::lock_guard<std::mutex> lk(m_);
    while ((int)th_.size() + 1 < members) {
        const int wid = (int)th_.size();
        try { th_.emplace_back([this, wid] { loop(wid); }); } catch (const std::system_error&) { break; }
    }
    active_.store(std::min(members, (int)th_.size() + 1));
}

KdPool::~KdPool() {
    if (pid_.load() != getpid()) { new std::vector<std::thread>(std::move(th_)); return; }
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : th_) if (t.joinable()) t.join();
}

void KdPool::loop(int wid) {
    for (;;) {
        if (wid + 1 < active_.load(std::memory_order_relaxed) && run_one()) continue;
        // nothing to do: a short spin (the next pass of a node usually follows within microseconds), then sleep
        bool got = false;
        for (int s = 0; s < 1500 && !got; ++s) {
            __builtin_ia32_pause();
            got = wid + 1 < active_.load(std::memory_order_relaxed) && n_queued_.load(std::memory_order_acquire) != 0;
        }
        if (got) continue;
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return stop_ || (wid + 1 < active_.load(std::memory_order_relaxed) && !q_.empty()); });
        if (stop_) return;
    }
}

}  // namespace fdx
